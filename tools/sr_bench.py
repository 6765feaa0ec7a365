"""Measure the super-resolution reconstruction (t2map.reconstruct_sr) at the headline size -- three 256 x 256 x 57
stacks of 1 x 1 x 4.5 mm, 8 echoes -> 256^3 x 8 -- beside the unchanged averaged merge (the chain): one forward call per
stack, the adjoint of all three, one whole iteration (three forwards, the update, the 3-D TV prox) and a default call; and
the numpy statement (_sr.py) on the host at the phantom's size (three 48 x 48 x 12 stacks, 3 echoes).

    python tools/sr_bench.py [--out profiles/r14_sr_bench.json] [--quick]

Times are HIP events around a call on an otherwise idle stream, after a warm-up; the median of the repeats is reported.
Bytes are arithmetic ("logical"): every array a call reads or writes counted once."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from recon_bench import COPY_TB_S, geometries, timed  # noqa: E402  (same stacks as the merge's benchmark)


def host_statement(n_iter=2):
    """Seconds of the statement's loop per iteration at the phantom's size, and of its set-up (normalisers, step size)."""
    from fetal_t2mapping_amd import _sr as S

    geoms = geometries(48, 12, 4.0)
    rng = np.random.default_rng(0)
    stacks = {o: rng.uniform(0, 1000, size=(3, 12, 48, 48)).astype(np.float32) for o in geoms}
    t0 = time.perf_counter()
    S.reconstruct_sr(stacks, geoms, n_iter=0)
    t_setup = time.perf_counter() - t0
    t0 = time.perf_counter()
    S.reconstruct_sr(stacks, geoms, n_iter=n_iter)
    return {"size": "3 stacks (3, 12, 48, 48) -> (3, 48, 48, 48)", "setup_s": t_setup,
            "s_per_iteration": (time.perf_counter() - t0 - t_setup) / n_iter, "default_iterations": S.DEFAULT_N_ITER}


def median_ms(fn, repeats):
    fn()
    return float(np.median([timed(fn)[0] for _ in range(repeats)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="skip the host statement")
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    side, n_sl, thick, n_vol = 256, 57, 4.5, 8
    geoms = geometries(side, n_sl, thick)
    rec = {"size": {"stacks": [n_vol, n_sl, side, side], "spacing": [1.0, 1.0, thick], "copy_TB_per_s": COPY_TB_S}}
    if not args.quick:
        rec["host_statement"] = host_statement()
        print(json.dumps({"host_statement": rec["host_statement"]}), flush=True)

    import torch

    import fetal_t2mapping_amd as t2
    from fetal_t2mapping_amd import _sr as S

    g = torch.Generator(device="cuda").manual_seed(0)
    stacks = {o: torch.rand((n_vol, n_sl, side, side), generator=g, device="cuda") * 1000.0 for o in geoms}
    order, hi, B, rels = S.sr_plan(geoms)
    n_h, n_l = n_vol * int(np.prod(hi.shape)), n_vol * n_sl * side * side
    x, _ = t2.reconstruct_stacks(stacks, geoms)
    rows = []

    def row(what, ms, nbytes, **more):
        r = {"what": what, "ms_median": ms, "logical_bytes": nbytes, "logical_GB_per_s": nbytes / ms / 1e6, **more}
        rows.append(r)
        print(json.dumps(r), flush=True)

    row("averaged merge (chain), the unchanged default", median_ms(lambda: t2.reconstruct_stacks(stacks, geoms), args.repeats),
        4 * (3 * n_l + n_h))
    res, N = [], []
    for profile in ("box", "bspline3"):
        res, N = [], []
        for s, o in enumerate(order):
            ms = median_ms(lambda: t2.sr_forward(x, B[s], (n_sl, side, side), profile=profile, rel_thickness=rels[s], y=stacks[o]),
                           args.repeats)
            r_s, n_s = t2.sr_forward(x, B[s], (n_sl, side, side), profile=profile, rel_thickness=rels[s], y=stacks[o])
            res.append(r_s), N.append(n_s)
            row(f"forward / residual, stack {o}, {profile}", ms, 4 * (n_h + 2 * n_l) + 8 * n_l // n_vol,
                radius=list(t2.sr_box(B[s], profile, rels[s])[1]))
        ms = median_ms(lambda: t2.sr_adjoint(res, N, B, profile, rels, hi.shape, x=x, tau=0.5), args.repeats)
        row(f"adjoint / update, three stacks, {profile}", ms, 4 * (2 * n_h + 3 * n_l) + 3 * 8 * n_l // n_vol)
    for profile in ("box", "bspline3"):
        kw = dict(profile=profile, x0=x)
        t0 = median_ms(lambda: t2.reconstruct_sr(stacks, geoms, n_iter=0, **kw), args.repeats)
        t1 = median_ms(lambda: t2.reconstruct_sr(stacks, geoms, n_iter=1, **kw), args.repeats)
        t4 = median_ms(lambda: t2.reconstruct_sr(stacks, geoms, n_iter=4, **kw), args.repeats)
        row(f"set-up (normalisers, column sums, step size read back), {profile}", t0, 0)
        row(f"one iteration (3 forwards, update, TV prox of {S.DEFAULT_PROX_ITER} iterations), {profile}", (t4 - t1) / 3.0, 0,
            weight=S.DEFAULT_WEIGHT)
    ms = median_ms(lambda: t2.reconstruct_sr(stacks, geoms), args.repeats)
    row(f"default call: merge, set-up, {S.DEFAULT_N_ITER} iterations, weight {S.DEFAULT_WEIGHT}, prox {S.DEFAULT_PROX_ITER}, box", ms, 0)
    a, _ = t2.reconstruct_sr(stacks, geoms)
    b, _ = t2.reconstruct_sr(stacks, geoms)
    rec["repeat_bit_equal"] = bool(torch.equal(a, b))
    rec["rows"] = rows
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
