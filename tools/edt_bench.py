"""Measure the exact Euclidean distance transform (t2map.distance) on one MI355X, in one process:

    python tools/edt_bench.py [--out profiles/r25_edt_bench.json] [--quick] [--no_scipy]

256^3 voxels (--quick: 64 x 256 x 256), four site sets: the benchmark's brain mask with the sites outside it
(invert = 1: the distance from every brain voxel to the background), the same mask with invert = 0 (the sites are the
brain), 1 % random sites, and a single site (the worst case: every row is scanned end to end).  Each with unit and with
(4.5, 1, 1) spacing.  What is timed is t2fit_edt_dev itself -- three launches into buffers allocated beforehand, both
outputs -- between two HIP events, the median of 5 after a warm-up; the kernels are not timed apart.  Beside them, in the
same run: scipy.ndimage.distance_transform_edt on the host for the same input (one run, and whether sqrt(d2) equals it
in every element), and the HBM time of reading the uint8 volume once and writing d2 and index once at 8 TB/s.  At 96^3:
dilate_mm(15.5) beside binary_dilate(ball(15)) on the brain mask, the two results asserted equal."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

REPEATS = 5
HBM_BYTES_PER_S = 8.0e12
SPACINGS = ((1.0, 1.0, 1.0), (4.5, 1.0, 1.0))


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
    ap.add_argument("--no_scipy", action="store_true", help="skip the host transforms")
    args = ap.parse_args()

    import torch

    import fetal_t2mapping_amd as t2
    from fetal_t2mapping_amd import _abi, _morph, synth
    from fetal_t2mapping_amd._gpu import current_stream, require, workspace
    from fetal_t2mapping_amd._lib import check

    lib = require(*_abi.EDT_SYMBOLS)
    dev = torch.device("cuda", 0)
    shape = (64, 256, 256) if args.quick else (256, 256, 256)
    n_vox = int(np.prod(shape))
    _, mask, _ = synth.brain_volume_torch(shape, 2, seed=synth.SEED_BASE, device=dev)
    brain = (mask.reshape(shape) != 0).to(torch.uint8)
    g = torch.Generator(device="cuda").manual_seed(25)
    sparse = (torch.rand(shape, generator=g, device=dev) < 0.01).to(torch.uint8)
    single = torch.zeros(shape, dtype=torch.uint8, device=dev)
    single[shape[0] // 3, shape[1] // 2, shape[2] // 5] = 1

    need = C.c_size_t(0)
    check(lib.t2fit_edt_workspace_bytes(*shape, C.byref(need)))
    ws, ws_ptr = workspace(need.value, dev)
    d2 = torch.empty(shape, dtype=torch.float64, device=dev)
    index = torch.empty(shape, dtype=torch.int32, device=dev)
    rec = {"repeats": REPEATS, "statistic": "median", "device": torch.cuda.get_device_name(dev), "shape": list(shape),
           "workspace_bytes": need.value, "hbm_bytes_per_s": HBM_BYTES_PER_S, "hbm_ms": 13.0 * n_vox / HBM_BYTES_PER_S * 1e3,
           "timed": "t2fit_edt_dev, both outputs, buffers allocated beforehand", "inputs": []}
    for name, vol, invert in (("brain mask, sites outside (invert = 1)", brain, 1), ("brain mask, sites inside (invert = 0)", brain, 0),
                              ("1 % random sites", sparse, 0), ("a single site", single, 0)):
        for spacing in SPACINGS:
            s = (C.c_double * 3)(*spacing)

            def call():
                check(lib.t2fit_edt_dev(vol.data_ptr(), invert, *shape, s, d2.data_ptr(), index.data_ptr(), ws_ptr, need.value,
                                        current_stream()))

            row = {"input": name, "spacing": list(spacing), "sites": float(((vol != 0) != bool(invert)).float().mean()),
                   "edt_ms": median_ms(call)}
            row["mean_distance"] = float(torch.sqrt(d2).mean())
            if not args.no_scipy:
                from scipy import ndimage

                host = (vol.cpu().numpy() != 0) != bool(invert)  # True at a site
                t0 = time.time()
                ref = ndimage.distance_transform_edt(~host, sampling=spacing)
                row["scipy_edt_ms"] = (time.time() - t0) * 1e3
                row["sqrt_equal_to_scipy"] = bool(np.array_equal(ref, np.sqrt(d2.cpu().numpy())))
                del host, ref
            rec["inputs"].append(row)
            print(json.dumps(row), flush=True)

    small = (96, 96, 96)
    _, mask, _ = synth.brain_volume_torch(small, 2, seed=synth.SEED_BASE, device=dev)
    m = (mask.reshape(small) != 0).to(torch.uint8)
    ball = _morph.ball(15)
    by_distance, by_runs = t2.distance.dilate_mm(m, 15.5), t2.binary_dilate(m, ball)
    assert torch.equal(by_distance, by_runs), "dilate_mm(15.5) differs from binary_dilate(ball(15))"
    rec["dilate_96"] = {"shape": list(small), "radius": 15, "equal": True, "dilate_mm_ms": median_ms(lambda: t2.distance.dilate_mm(m, 15.5)),
                        "binary_dilate_ball_ms": median_ms(lambda: t2.binary_dilate(m, ball))}
    print(json.dumps(rec["dilate_96"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
