#!/usr/bin/env python3
"""Times the in-vivo ROI statistics (t2map.roi_erode / roi_stats) on the GPU, with the scipy / numpy loop they replace
(utils/ada_utils.py:160-189) timed on the host beside them.  One JSON line per size:

    python tools/roi_bench.py [--sizes 180x256x256 360x512x512] [--labels 120] [--reps 20] [--host_labels 8]

erode_ms / stats_ms: HIP-event time per call (mean over --reps after a warm-up) of the erosion of all labels
(connectivity 3, one iteration, inside one tissue) and of mean / std / median / counts of one map.  erode_gbps: the
12 B per voxel the pass has to move (label + tissue read, ROI written) over erode_ms; erode_frac_hbm: that over the
8 TB/s peak.  host_*: binary_erosion + gather + mean / std / median per label on the CPU for --host_labels labels
(0 = all), and that time scaled to all labels.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # B/s, MI355X


def volume(shape, n_labels, seed, device):
    """Blocky atlas (labels 0..n_labels, blocks of 12 x 16 x 16), a two-tissue volume, a float32 map with ties."""
    import torch

    g = torch.Generator(device=device).manual_seed(seed)
    z, y, x = shape
    small = torch.randint(0, n_labels + 1, (-(-z // 12), -(-y // 16), -(-x // 16)), generator=g, device=device, dtype=torch.int32)
    lab = small.repeat_interleave(12, 0).repeat_interleave(16, 1).repeat_interleave(16, 2)[:z, :y, :x].contiguous()
    tis = torch.randint(2, 4, (-(-z // 60), -(-y // 64), -(-x // 64)), generator=g, device=device, dtype=torch.int32)
    tis = tis.repeat_interleave(60, 0).repeat_interleave(64, 1).repeat_interleave(64, 2)[:z, :y, :x].contiguous()
    m = (torch.round(torch.randn(shape, generator=g, device=device) * 80.0) * 0.25 + 150.0).to(torch.float32)
    return lab, tis, m


def timed(fn, reps):
    import torch

    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps, out


def host_loop(lab, tis, m, labels):
    from scipy.ndimage import binary_erosion, generate_binary_structure

    st = generate_binary_structure(3, 3)
    t = time.perf_counter()
    out = {}
    for L in labels:
        sel = binary_erosion(np.logical_and(tis == 3, lab == L), structure=st)
        v = m[sel].flatten()
        with np.errstate(all="ignore"):
            out[L] = (len(v), np.mean(v) if len(v) else np.nan, np.std(v) if len(v) else np.nan,
                      np.median(v) if len(v) else np.nan)
    return time.perf_counter() - t, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["180x256x256", "360x512x512"])
    ap.add_argument("--labels", type=int, default=120)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host_labels", type=int, default=8, help="labels the host loop is timed on (0 = all)")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("roi_bench: no HIP device (timings are taken on the GPU only)")
    import ctypes as C

    import fetal_t2mapping_amd as t2
    from fetal_t2mapping_amd._lib import check, require_gpu

    lib = require_gpu()
    for size in args.sizes:
        shape = tuple(int(v) for v in size.split("x"))
        n_vox = int(np.prod(shape))
        lab, tis, m = volume(shape, args.labels, 7, torch.device("cuda", 0))
        # the library calls themselves, on buffers made once (the Python mirror adds label remapping and the copy
        # of the statistics to the host; its calls are checked against the host loop below)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        roi = torch.empty_like(lab)
        f64 = torch.empty((3, args.labels), dtype=torch.float64, device=lab.device)
        i64 = torch.empty((2, args.labels), dtype=torch.int64, device=lab.device)

        def erode():
            check(lib.t2fit_roi_erode_dev(lab.data_ptr(), tis.data_ptr(), 3, *shape, args.labels, 3, 1, roi.data_ptr(), st))

        def stats(median=True):
            check(lib.t2fit_roi_stats_dev(m.data_ptr(), roi.data_ptr(), n_vox, args.labels, f64[0].data_ptr(), f64[1].data_ptr(),
                                          f64[2].data_ptr() if median else None, i64[0].data_ptr(), i64[1].data_ptr(), st))

        erode_ms, _ = timed(erode, args.reps)
        stats_ms, _ = timed(stats, args.reps)
        nomed_ms, _ = timed(lambda: stats(False), args.reps)
        s = t2.roi_stats(m, t2.roi_erode(lab, tis, 3, labels=range(1, args.labels + 1)), args.labels)
        assert np.array_equal(s.count, i64[0].cpu().numpy())
        k = args.host_labels or args.labels
        picks = [int(v) for v in np.linspace(1, args.labels, k).round()]
        host_s, ref = host_loop(lab.cpu().numpy(), tis.cpu().numpy(), m.cpu().numpy(), picks)
        same = all(s.count[L - 1] == ref[L][0] and (ref[L][0] == 0 or np.float32(s.median[L - 1]) == np.float32(ref[L][3]))
                   for L in picks)
        print(json.dumps({
            "tool": "roi_bench", "shape": list(shape), "n_vox": n_vox, "labels": args.labels, "reps": args.reps,
            "roi_voxels": int(s.count.sum()), "largest_region": int(s.count.max()),
            "erode_ms": round(erode_ms, 4), "erode_gbps": round(12.0 * n_vox / (erode_ms * 1e-3) / 1e9, 1),
            "erode_frac_hbm": round(12.0 * n_vox / (erode_ms * 1e-3) / HBM_PEAK, 4),
            "stats_ms": round(stats_ms, 4), "stats_no_median_ms": round(nomed_ms, 4),
            "host_labels_timed": len(picks), "host_s": round(host_s, 3),
            "host_s_all_labels_scaled": round(host_s * args.labels / len(picks), 2), "host_matches_gpu": bool(same),
        }), flush=True)


if __name__ == "__main__":
    main()
