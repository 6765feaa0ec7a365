"""Measure the outlier weighting of the super-resolution loop (t2fit_sr_robust_dev, reconstruct_sr(robust=True)) at the
headline size -- three 256 x 256 x 57 stacks of 1 x 1 x 4.5 mm, 8 echoes -> 256^3 x 8: the robust step alone (slice sums,
scale, apply: three launches on the residuals of all stacks), one iteration and a default call with and without it, all in
one run, so that the ratios compare like with like.

    python tools/sr_robust_bench.py [--out profiles/r17_sr_robust_bench.json]

Times are HIP events around a call on an otherwise idle stream, after a warm-up; the median of the repeats is reported.
Bytes are arithmetic ("logical"): the sums read r (4 B per sample and echo) and N (8 B per sample and chunk of 4 echoes), the
apply reads and writes r (8 B per sample and echo) and reads N once per chunk; no masks here.  The step works in place, so
the repeats see residuals that were already weighted: the traffic is the same."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from recon_bench import COPY_TB_S, geometries, timed  # noqa: E402  (same stacks as the merge's benchmark)

CHUNK = 4  # kRobustChunk of csrc/t2fit_sr_robust.hip


def median_ms(fn, repeats):
    fn()
    return float(np.median([timed(fn)[0] for _ in range(repeats)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    side, n_sl, thick, n_vol = 256, 57, 4.5, 8
    geoms = geometries(side, n_sl, thick)

    import torch

    import fetal_t2mapping_amd as t2
    from fetal_t2mapping_amd import _abi, _gpu_sr
    from fetal_t2mapping_amd import _sr as S
    from fetal_t2mapping_amd._gpu import require

    lib = require(*_abi.SR_ROBUST_SYMBOLS)
    g = torch.Generator(device="cuda").manual_seed(0)
    stacks = {o: torch.rand((n_vol, n_sl, side, side), generator=g, device="cuda") * 1000.0 for o in geoms}
    order, hi, B, rels = S.sr_plan(geoms)
    x, _ = t2.reconstruct_stacks(stacks, geoms)
    rec = {"size": {"stacks": [n_vol, n_sl, side, side], "spacing": [1.0, 1.0, thick], "copy_TB_per_s": COPY_TB_S}}
    rows = []

    def row(what, ms, nbytes, **more):
        r = {"what": what, "ms_median": ms, "logical_bytes": nbytes, "logical_GB_per_s": nbytes / ms / 1e6, **more}
        rows.append(r)
        print(json.dumps(r), flush=True)

    res, N = [], []
    for s, o in enumerate(order):
        r_s, n_s = t2.sr_forward(x, B[s], (n_sl, side, side), rel_thickness=rels[s], y=stacks[o])
        res.append(r_s.reshape(-1)), N.append(n_s.reshape(-1))
    n_slices, lr = 3 * n_sl, [(n_sl, side, side)] * 3
    sums = torch.empty((n_vol, n_slices, 2), dtype=torch.float64, device="cuda")
    weights = torch.empty((n_vol, n_slices), dtype=torch.float64, device="cuda")
    sigma2 = torch.empty(n_vol, dtype=torch.float64, device="cuda")
    par = _gpu_sr.robust_struct(S.robust_params(True))
    samples = 3 * n_sl * side * side
    chunks = -(-n_vol // CHUNK)
    nbytes = samples * (4 * n_vol + 8 * chunks) + samples * (8 * n_vol + 8 * chunks)
    ms = median_ms(lambda: _gpu_sr._robust(lib, res, N, [None] * 3, lr, n_vol, par, sums, weights, sigma2), args.repeats)
    row("robust step alone: slice sums, scale, apply (3 launches, three stacks)", ms, nbytes, sigma2_on=int((sigma2 > 0).sum()))
    step_ms = ms
    per_iter = {}
    for robust in (None, True):
        kw = dict(x0=x, robust=robust)
        t1 = median_ms(lambda: t2.reconstruct_sr(stacks, geoms, n_iter=1, **kw), args.repeats)
        t4 = median_ms(lambda: t2.reconstruct_sr(stacks, geoms, n_iter=4, **kw), args.repeats)
        per_iter[robust] = (t4 - t1) / 3.0
        row(f"one iteration (3 forwards, update, TV prox of {S.DEFAULT_PROX_ITER} iterations), robust={robust}", per_iter[robust], 0)
    calls = {}
    for robust in (None, True):
        calls[robust] = median_ms(lambda: t2.reconstruct_sr(stacks, geoms, robust=robust), args.repeats)
        row(f"default call: merge, set-up, {S.DEFAULT_N_ITER} iterations, robust={robust}", calls[robust], 0)
    rec["ratios"] = {"step_over_plain_iteration": step_ms / per_iter[None], "robust_iteration_over_plain": per_iter[True] / per_iter[None],
                     "robust_call_over_plain": calls[True] / calls[None]}
    print(json.dumps(rec["ratios"]), flush=True)
    a, _ = t2.reconstruct_sr(stacks, geoms, robust=True)
    b, _ = t2.reconstruct_sr(stacks, geoms, robust=True)
    rec["repeat_bit_equal"] = bool(torch.equal(a, b))
    rec["rows"] = rows
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
