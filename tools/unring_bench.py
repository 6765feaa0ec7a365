"""Measure the Gibbs-ringing removal (t2map.unring) on one MI355X, in one process:

    python tools/unring_bench.py [--out profiles/r23_unring_bench.json] [--quick]

Two blocks of 256 x 256 slices: three stacks of 57 slices x 8 echoes (1368 slices) and 256^3 x 8 echoes (2048 slices); --quick:
64 and 128 slices.  For each: the split, the row pass along x, the row pass along y and the whole call (K 20, window 1 .. 3),
HIP events around each, the median of 5 after a warm-up.  Beside them: the matrix-instruction bound 2 n^2 rows (2K+1) per
axis at 64 FLOP/clk/SIMD x 4 x 256 CUs x 2.4 GHz (the rate DESIGN.md section 8r uses; the products of the split, 2 x (2 nx +
8 ny + 2 nx) n-long chains per sample, are counted the same way), the HBM time of reading and writing the block once at
8 TB/s, a joint-TV call on the 256^3 x 8 block of the same run, and the float64 reference of tests/unring_cases.py on the
host for one stack of 57 slices."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

REPEATS = 5
MFMA_FLOPS = 64 * 4 * 256 * 2.4e9
HBM_BYTES_PER_S = 8.0e12


def median_ms(fn):
    import torch

    fn()  # warm-up
    times = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()

    import torch

    import fetal_t2mapping_amd as t2

    dev = torch.device("cuda", 0)
    ny = nx = 256
    K, window = 20, (1, 3)
    tables = t2.unring.unring_tables(ny, nx, K)
    rec = {"repeats": REPEATS, "statistic": "median", "device": torch.cuda.get_device_name(dev), "K": K, "window": list(window),
           "mfma_flops_per_s": MFMA_FLOPS, "hbm_bytes_per_s": HBM_BYTES_PER_S, "blocks": []}
    g = torch.Generator(device="cuda").manual_seed(23)
    for name, slices in (("3 stacks of 256x256x57x8", 64 if args.quick else 3 * 57 * 8), ("256^3 x 8", 128 if args.quick else 2048)):
        x = torch.rand((slices, ny, nx), generator=g, device=dev) * 1000.0
        x[:, 64:192, 80:200] += 400.0
        out = torch.empty_like(x)
        rows = slices * ny
        row = {"block": name, "slices": slices,
               "split_ms": median_ms(lambda: t2.unring.unring_split(x, tables)),
               "rows_x_ms": median_ms(lambda: t2.unring.unring_rows(x, "x", K, *window, tables=tables, details=False)),
               "rows_y_ms": median_ms(lambda: t2.unring.unring_rows(x, "y", K, *window, tables=tables, details=False)),
               "whole_ms": median_ms(lambda: t2.unring.unring_slices(x, K, *window, tables=tables, out=out)),
               "bound_rows_ms_per_axis": 2.0 * nx * nx * rows * (2 * K + 1) / MFMA_FLOPS * 1e3,
               "bound_split_ms": 2.0 * (2 * nx + 4 * ny + 4 * ny + 2 * nx) * slices * ny * nx / MFMA_FLOPS * 1e3,
               "hbm_ms": 2.0 * x.numel() * 4 / HBM_BYTES_PER_S * 1e3}
        row["fraction_of_bound_rows_x"] = row["bound_rows_ms_per_axis"] / row["rows_x_ms"]
        row["fraction_of_bound_rows_y"] = row["bound_rows_ms_per_axis"] / row["rows_y_ms"]
        row["fraction_of_bound_split"] = row["bound_split_ms"] / row["split_ms"]
        rec["blocks"].append(row)
        print(json.dumps(row), flush=True)
        del x, out
    # the house yardstick: a joint-TV call on 256^3 x 8 of the same run
    from fetal_t2mapping_amd import synth

    shape, n_te = ((64, 256, 256) if args.quick else (256, 256, 256)), 8
    echoes, mask, _ = synth.brain_volume_torch(shape, n_te, seed=synth.SEED_BASE, device=dev)
    echoes, mask = echoes.reshape((n_te,) + shape), mask.reshape(shape)
    sigma, _ = t2.estimate_background_sigma(echoes, mask)
    buf = torch.empty_like(echoes)
    rec["tv_joint_call_ms"] = median_ms(lambda: t2.denoise_tv(echoes, sigma, out=buf, joint=True))
    print(json.dumps({"tv_joint_call_ms": rec["tv_joint_call_ms"]}), flush=True)
    # the float64 reference on the host, one stack
    import unring_cases

    stack = (np.random.default_rng(23).random((8 if args.quick else 57, ny, nx)) * 1000.0).astype(np.float32)
    t0 = time.time()
    unring_cases.ref_unring(stack, K, *window)
    rec["host_float64_reference_s"] = {"slices": int(stack.shape[0]), "seconds": time.time() - t0}
    print(json.dumps(rec["host_float64_reference_s"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
