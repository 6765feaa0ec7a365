"""Measure the orthogonal-stack reconstruction (t2map.reconstruct_stacks): the fused kernel against the chain of
single-stage passes at the headline size (three 256 x 256 x 57 stacks of 1 x 1 x 4.5 mm, 8 echoes -> 256^3 x 8), the
single stage per orientation, and the numpy statement (_resample.py) on the host as the baseline.

    python tools/recon_bench.py [--out profiles/recon_bench.json] [--quick]

Times are HIP events around a call on an otherwise idle stream, after a warm-up; the median of the repeats is reported,
the two forms alternate inside one process.  Bytes are arithmetic ("logical"): every stack read once and the output
written once for the fused form; the chain adds the write and the read of the two moving intermediates and of the two
resampled volumes, and the merge's read-modify-write."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_TB_S = 6.29  # measured device copy rate of this project's benchmarks (profiles/README.md)


def geometries(side, n_sl, thick):
    from fetal_t2mapping_amd import _resample as R

    ax = np.eye(3)
    cor = np.array([[1, 0, 0], [0, 0, 1], [0, 1, 0.0]])
    sag = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0.0]])
    out = {}
    for o, d in (("ax", ax), ("cor", cor), ("sag", sag)):
        extent = d @ (np.array([1.0, 1.0, thick]) * (np.array([side, side, n_sl]) - 1) / 2.0)
        out[o] = R.Geometry((side, side, n_sl), (1.0, 1.0, thick), -extent, d.ravel())
    return out


def host_baseline(geoms, n_sl, side, slabs=16, threads=16):
    """_resample.reconstruct's arithmetic on `slabs` z-slabs of one echo's output, `threads` at a time: seconds per
    256^3 echo of wall time (stage 2 and the merge are evaluated slab by slab)."""
    from fetal_t2mapping_amd import _resample as R

    rng = np.random.default_rng(0)
    host = {o: rng.uniform(0, 1000, size=(n_sl, side, side)).astype(np.float32) for o in geoms}
    order, hi, a1, a2 = R.plan(geoms)
    H = {}
    t0 = time.perf_counter()
    for m in (1, 2):
        H[m] = R.resample(host[order[m]], a1[m], hi[m].shape)
    t_stage1 = time.perf_counter() - t0
    nz = hi[0].shape[0]
    step = nz // slabs

    def slab(k):
        Hf = R.resample(host[order[0]], a1[0], (step, side, side), start=(0, 0, k * step))
        Rm = [R.resample(H[m], a2[m - 1], (step, side, side), start=(0, 0, k * step)) for m in (1, 2)]
        return R.merge(Hf, Rm[0], Rm[1]).shape

    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(slab, range(slabs)))
    return t_stage1 + (time.perf_counter() - t0)


def timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="skip the host baseline")
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    side, n_sl, thick, n_vol = 256, 57, 4.5, 8
    geoms = geometries(side, n_sl, thick)
    rec = {"size": {"stacks": [n_vol, n_sl, side, side], "spacing": [1.0, 1.0, thick], "copy_TB_per_s": COPY_TB_S}}
    if not args.quick:
        s = host_baseline(geoms, n_sl, side)
        rec["host"] = {"threads": 16, "s_per_echo": s, "s_8_echoes": s * n_vol}
        print(json.dumps({"host": rec["host"]}), flush=True)

    import torch

    import fetal_t2mapping_amd as t2
    from fetal_t2mapping_amd import _resample as R

    g = torch.Generator(device="cuda").manual_seed(0)
    stacks = {o: torch.rand((n_vol, n_sl, side, side), generator=g, device="cuda") * 1000.0 for o in geoms}
    order, hi, a1, a2 = R.plan(geoms)
    n_out = n_vol * int(np.prod(hi[0].shape))
    n_in = sum(int(stacks[o].numel()) for o in geoms)
    n_mid = sum(n_vol * int(np.prod(hi[m].shape)) for m in (1, 2))
    logical = {"fused": 4 * (n_in + n_out),
               # stage 1: stacks in, three H out; stage 2: two H in, two R out; merge: H_0 and two R in, out
               "chain": 4 * (n_in + n_out + n_mid + n_mid + 2 * n_out + 3 * n_out + n_out)}
    forms = ("fused", "chain")
    for f in forms:  # warm-up: code objects, allocator
        t2.reconstruct_stacks(stacks, geoms, form=f)
    torch.cuda.synchronize()
    ms = {f: [] for f in forms}
    for _ in range(args.repeats):
        for f in forms:
            ms[f].append(timed(lambda: t2.reconstruct_stacks(stacks, geoms, form=f))[0])
    rec["reconstruct"] = []
    for f in forms:
        med = float(np.median(ms[f]))
        row = {"form": f, "ms_median": med, "ms_min": float(min(ms[f])), "ms_max": float(max(ms[f])), "repeats": args.repeats,
               "logical_bytes": logical[f], "logical_GB_per_s": logical[f] / med / 1e6,
               "share_of_copy_rate": logical[f] / med / 1e9 / COPY_TB_S,
               "fused_bytes_GB_per_s": logical["fused"] / med / 1e6}
        rec["reconstruct"].append(row)
        print(json.dumps(row), flush=True)
    a, _ = t2.reconstruct_stacks(stacks, geoms, form="fused")
    b, _ = t2.reconstruct_stacks(stacks, geoms, form="chain")
    rec["forms_bit_equal"] = bool(torch.equal(a, b))
    del a, b
    rec["stage"] = []
    for o in ("ax", "cor", "sag"):  # one stage onto the ax grid: the lane axis differs per orientation
        for label, src, sg in (("stage1", stacks[o], geoms[o]), ):
            t2.resample_volume(src, sg, like=hi[0])
            t = [timed(lambda: t2.resample_volume(src, sg, like=hi[0]))[0] for _ in range(args.repeats)]
            nbytes = 4 * (int(src.numel()) + n_out)
            row = {"stack": o, "what": "thick-slice stack -> ax 1 mm grid", "ms_median": float(np.median(t)),
                   "logical_bytes": nbytes, "logical_GB_per_s": nbytes / float(np.median(t)) / 1e6}
            rec["stage"].append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
