"""Measure the super-resolution operators with a rigid pose per slice (t2fit_sr_slice_forward_dev / _adjoint_dev) beside
the stack-wise ones at the headline size -- three 256 x 256 x 57 stacks of 1 x 1 x 4.5 mm, 8 echoes -> 256^3 x 8:

    (a) the stack-wise path (t2fit_sr_forward_dev / t2fit_sr_adjoint_dev), the yardstick;
    (b) the slice path with every slice at its stack's pose (same bits as (a));
    (c) the slice path with a pose per slice, components uniform in +-3 degrees / +-2 mm;
    (d) the adjoint of (c) with each stack padded to four times the slices, the extra ones posed off the grid: the
        check that culling works, reported as a ratio to (c).

For each of (a) (b) (c): one forward call per stack, the adjoint of all three, one whole iteration and a default call;
every figure also as a ratio to (a), measured in the same process.  The result of (c) is compared with the numpy statement
on sample boxes; the mismatch count must be 0.

    python tools/sr_slice_bench.py [--out profiles/r15_sr_slice_bench.json] [--repeats 7]

Times are HIP events around a call on an otherwise idle stream, after a warm-up; the median of the repeats is reported.
The operator calls are timed below the Python wrappers (tables uploaded once, as reconstruct_sr does)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from recon_bench import geometries, timed  # noqa: E402  (same stacks as the merge's benchmark)


def median_ms(fn, repeats):
    fn()
    return float(np.median([timed(fn)[0] for _ in range(repeats)]))


def motion(lz, deg, mm, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1.0, 1.0, size=(lz, 6))
    p[:, :3] *= np.deg2rad(deg)
    p[:, 3:] *= mm
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--side", type=int, default=256, help="in-plane size of the stacks (default 256, the headline size)")
    ap.add_argument("--slices", type=int, default=57)
    ap.add_argument("--echoes", type=int, default=8)
    args = ap.parse_args()
    side, n_sl, thick, n_vol = args.side, args.slices, 4.5, args.echoes

    import torch

    import fetal_t2mapping_amd as t2
    from fetal_t2mapping_amd import _abi, _gpu_sr as G, _sr as S
    from fetal_t2mapping_amd._gpu import require

    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: this tool measures on the GPU")
    lib = require(*(_abi.SR_SYMBOLS + _abi.SR_SLICE_SYMBOLS))
    dev = torch.device("cuda", 0)
    geoms = geometries(side, n_sl, thick)
    g = torch.Generator(device="cuda").manual_seed(0)
    stacks = {o: torch.rand((n_vol, n_sl, side, side), generator=g, device="cuda") * 1000.0 for o in geoms}
    order, hi, B, rels = S.sr_plan(geoms)
    hr, lr = hi.shape, (n_sl, side, side)
    n_l = n_sl * side * side
    x = t2.reconstruct_stacks(stacks, geoms)[0].reshape(-1)
    y = [stacks[o].reshape(-1) for o in order]
    pid = S.BOX
    poses = {o: S.compose_slice_transforms(None, motion(n_sl, 3.0, 2.0, 10 + i), geoms[o]) for i, o in enumerate(order)}
    same = {o: np.repeat(np.eye(4)[None], n_sl, axis=0) for o in order}
    affines = {"b": S.slice_plan(order, hi, geoms, B, [lr] * 3, same), "c": S.slice_plan(order, hi, geoms, B, [lr] * 3, poses)}
    tables = {k: [G._table(G.sr_slice_table(v[s], pid, rels[s]), dev, n_sl) for s in range(3)] for k, v in affines.items()}
    boxes = [G.sr_box(B[s], pid, rels[s]) for s in range(3)]
    rec = {"size": {"stacks": [n_vol, n_sl, side, side], "spacing": [1.0, 1.0, thick], "grid": list(hr)},
           "poses": "components uniform in +-3 degrees / +-2 mm about each slice's centre", "profile": "box"}
    rows = []

    def row(what, variant, ms, base=None, **more):
        r = {"what": what, "variant": variant, "ms_median": ms, **({} if base is None else {"ratio": ms / base}), **more}
        rows.append(r)
        print(json.dumps(r), flush=True)
        return ms

    res = {k: [torch.empty(n_vol * n_l, dtype=torch.float32, device=dev) for _ in range(3)] for k in "abc"}
    N = {k: [torch.empty(n_l, dtype=torch.float64, device=dev) for _ in range(3)] for k in "abc"}
    z = torch.empty_like(x)

    def forward(k, s, n_out):
        if k == "a":
            G._forward(lib, x, hr, n_vol, B[s], boxes[s], pid, rels[s], y[s], None, lr, res[k][s], n_out)
        else:
            G._forward_slices(lib, x, hr, n_vol, tables[k][s], pid, rels[s], y[s], None, lr, res[k][s], n_out)

    def adjoint(k):
        if k == "a":
            G._adjoint(lib, res[k], N[k], [None] * 3, [lr] * 3, B, [pid] * 3, rels, x, 0.5, z, hr, n_vol)
        else:
            G._adjoint_slices(lib, res[k], N[k], [None] * 3, tables[k], [lr] * 3, [pid] * 3, rels, x, 0.5, z, hr, n_vol)

    names = {"a": "(a) stack-wise", "b": "(b) slices at the stack's pose", "c": "(c) slices at +-3 deg / +-2 mm"}
    base = {}
    for k in "abc":
        for s, o in enumerate(order):
            forward(k, s, N[k][s])  # the normalisers, once
            ms = median_ms(lambda: forward(k, s, None), args.repeats)
            base.setdefault(("fwd", o), ms)
            row(f"forward / residual, stack {o}", names[k], ms, base[("fwd", o)])
        ms = median_ms(lambda: adjoint(k), args.repeats)
        base.setdefault("adj", ms)
        row("adjoint / update, three stacks", names[k], ms, base["adj"])
    rec["b_equals_a_bit_for_bit"] = bool(all(torch.equal(res["a"][s], res["b"][s]) and torch.equal(N["a"][s], N["b"][s]) for s in range(3)))
    adjoint("a")
    za = z.clone()
    adjoint("b")
    rec["b_equals_a_bit_for_bit"] = rec["b_equals_a_bit_for_bit"] and bool(torch.equal(za, z))
    # (d): (c) with each stack padded to four times the slices, the extra ones posed off the grid
    far = np.eye(4)
    far[:3, 3] = (5000.0, -4000.0, 3000.0)
    pad_lr = (4 * n_sl, side, side)
    pad_tables, pad_res, pad_n = [], [], []
    for s, o in enumerate(order):
        gp = type(geoms[o])((side, side, 4 * n_sl), geoms[o].GetSpacing(), geoms[o].GetOrigin(), geoms[o].GetDirection())
        t = np.concatenate([poses[o], np.repeat(far[None], 3 * n_sl, axis=0)])
        pad_tables.append(G._table(G.sr_slice_table(S.slice_affines(hi, gp, t), pid, rels[s]), dev, 4 * n_sl))
        r = torch.zeros((n_vol, 4 * n_sl, side, side), dtype=torch.float32, device=dev)
        r[:, :n_sl] = res["c"][s].reshape(n_vol, n_sl, side, side)
        n = torch.zeros(4 * n_l, dtype=torch.float64, device=dev)
        n[:n_l] = N["c"][s]
        pad_res.append(r.reshape(-1)), pad_n.append(n)
    zd = torch.empty_like(x)
    padded = lambda: G._adjoint_slices(lib, pad_res, pad_n, [None] * 3, pad_tables, [pad_lr] * 3, [pid] * 3, rels, x, 0.5, zd, hr, n_vol)
    ms_c = median_ms(lambda: adjoint("c"), args.repeats)
    ms_d = median_ms(padded, args.repeats)
    row("adjoint / update, three stacks of 4 x the slices, the extra ones off the grid", "(d) ratio to (c), same moment", ms_d, ms_c,
        c_ms_median=ms_c)
    adjoint("c")
    rec["d_equals_c_bit_for_bit"] = bool(torch.equal(z, zd))
    # one iteration and a default call
    x0 = x.reshape((n_vol,) + hr)
    for k, st in (("a", None), ("b", same), ("c", poses)):
        kw = {} if st is None else {"slice_transforms": st}
        t1 = median_ms(lambda: t2.reconstruct_sr(stacks, geoms, n_iter=1, x0=x0, **kw), args.repeats)
        t4 = median_ms(lambda: t2.reconstruct_sr(stacks, geoms, n_iter=4, x0=x0, **kw), args.repeats)
        base.setdefault("iter", (t4 - t1) / 3.0)
        row(f"one iteration (3 forwards, update, TV prox of {S.DEFAULT_PROX_ITER} iterations)", names[k], (t4 - t1) / 3.0, base["iter"])
        ms = median_ms(lambda: t2.reconstruct_sr(stacks, geoms, **kw), max(3, args.repeats // 2))
        base.setdefault("call", ms)
        row(f"default call: merge, set-up, {S.DEFAULT_N_ITER} iterations, weight {S.DEFAULT_WEIGHT}", names[k], ms, base["call"])
    # (c) against the statement on sample boxes
    for s in range(3):
        forward("c", s, None)
    adjoint("c")
    torch.cuda.synchronize()
    xh = x0.cpu().numpy()
    resh = [r.cpu().numpy().reshape((n_vol,) + lr) for r in res["c"]]
    nh = [n.cpu().numpy().reshape(lr) for n in N["c"]]
    zh = z.cpu().numpy().reshape((n_vol,) + hr)
    rng = np.random.default_rng(1)
    bits = lambda a, b: int(np.sum(np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)))
    mismatches, compared = 0, 0
    for s, o in enumerate(order):
        bz, by, bx = int(rng.integers(0, n_sl - 4)), int(rng.integers(0, side - 12)), int(rng.integers(0, side - 12))
        want, wn = S.forward_slices(xh, affines["c"][s], lr, "box", rels[s], y=stacks[o].cpu().numpy(), start=(bx, by, bz), shape=(4, 12, 12))
        mismatches += int(np.sum(nh[s][bz:bz + 4, by:by + 12, bx:bx + 12] != wn)) + bits(resh[s][:, bz:bz + 4, by:by + 12, bx:bx + 12], want)
        compared += wn.size + want.size
    for _ in range(2):
        bz, by, bx = (int(rng.integers(0, n - 12)) for n in hr)
        want = S.adjoint_slices(resh, nh, affines["c"], "box", rels, hr, x=xh, tau=0.5, start=(bx, by, bz), shape=(12, 12, 12))
        mismatches += bits(zh[:, bz:bz + 12, by:by + 12, bx:bx + 12], want)
        compared += want.size
    rec["statement_sample_boxes"] = {"values_compared": compared, "mismatches": mismatches}
    print(json.dumps(rec["statement_sample_boxes"]), flush=True)
    rec["rows"] = rows
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    if mismatches or not rec["b_equals_a_bit_for_bit"] or not rec["d_equals_c_bit_for_bit"]:
        raise SystemExit("the device result differs from what it must equal")


if __name__ == "__main__":
    main()
