"""Measure the mask-building stage (csrc/t2fit_morph.hip) at 256^3: one ball-15 dilation, phantom_mask and build_mask
whole, 3-D fill_holes on a shell phantom (with its sweep count) and phantom_labels for 14 seeds; and the scipy statement
of the same steps on the host at a smaller cube (--host_side, default 64: the ball-15 steps grow with the volume times
15 515), with the device time at that size next to it.

    python tools/morph_bench.py [--out profiles/morph_bench.json] [--quick] [--host_side 64]

Device times are HIP events around a call on an otherwise idle stream after a warm-up, the median of the repeats.  The
calls include what the Python wrappers do (workspace allocation from torch's cache, the run-list upload)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def phantom(side, seed=0):
    """A bright cylinder with dark vials inside a dim, noisy background (float32), and a hollow-shell mask."""
    rng = np.random.default_rng(seed)
    ax = np.arange(side, dtype=np.float32)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij", sparse=True)
    c = side / 2.0
    r = np.hypot(y - c, x - c)
    vol = np.where((r < side * 0.33) & (z > side * 0.1) & (z < side * 0.9), 400.0, 5.0).astype(np.float32)
    for k in range(14):
        vy, vx = c + side * 0.2 * np.cos(k * 0.45), c + side * 0.2 * np.sin(k * 0.45)
        vol[np.broadcast_to(np.hypot(y - vy, x - vx) < side * 0.03, vol.shape)] = 20.0
    vol += rng.normal(0.0, 3.0, vol.shape).astype(np.float32)
    rr = np.sqrt((z - c) ** 2 + (y - c) ** 2 + (x - c) ** 2)
    shell = ((rr > side * 0.3) & (rr < side * 0.32)) | ((rr > side * 0.1) & (rr < side * 0.12))
    return vol, shell


def timed(fn, repeats):
    import torch

    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)), "repeats": repeats}


def device_rows(side, repeats):
    import torch

    import fetal_t2mapping_amd as t2
    from fetal_t2mapping_amd import _morph as M

    vol_h, shell_h = phantom(side)
    vol = torch.from_numpy(vol_h).cuda()
    shell = torch.from_numpy(shell_h.astype(np.uint8)).cuda()
    mask = t2.binary_threshold(vol, 100.0)
    seeds = [[int(side / 2 + side * 0.2 * np.sin(k * 0.45)), int(side / 2 + side * 0.2 * np.cos(k * 0.45)), side // 2] for k in range(14)]
    ball15 = M.footprint_runs(M.ball(15))
    rows = {"dilate_ball15": timed(lambda: t2.binary_dilate(mask, ball15), repeats),
            "phantom_mask": timed(lambda: t2.phantom_mask(vol), repeats),
            "build_mask": timed(lambda: t2.build_mask(vol), repeats),
            "fill_holes_3d_shells": timed(lambda: t2.fill_holes(shell), repeats),
            "phantom_labels_14_seeds": timed(lambda: t2.phantom_labels((side,) * 3, seeds), repeats)}
    rows["fill_holes_3d_shells"]["sweeps"] = t2.fill_holes(shell, return_sweeps=True)[1]
    rows["fill_holes_3d_shells"]["filled_voxels"] = int(t2.fill_holes(shell).sum().item() - shell.sum().item())
    return rows


def host_rows(side):
    from scipy import ndimage as ndi

    from fetal_t2mapping_amd import _morph as M

    vol, shell = phantom(side)
    mask = vol >= 100
    out = {}

    def clock(name, fn):
        t0 = time.perf_counter()
        fn()
        out[name] = {"s": time.perf_counter() - t0}
        print(json.dumps({"host": name, **out[name]}), flush=True)

    def phantom_mask():
        m = np.pad(ndi.binary_fill_holes(mask), 15)
        m = ndi.binary_erosion(ndi.binary_dilation(m, M.ball(15)), M.ball(15))[15:-15, 15:-15, 15:-15]
        return ndi.binary_dilation(m, M.ball(10))

    def build_mask():
        for i in range(vol.shape[2]):
            bw = ndi.binary_fill_holes(vol[:, :, i] > 1.0)
            ndi.binary_erosion(ndi.binary_dilation(bw, structure=np.ones((5, 5))), structure=np.ones((5, 5)))

    clock("dilate_ball15", lambda: ndi.binary_dilation(mask, M.ball(15)))
    clock("phantom_mask", phantom_mask)
    clock("build_mask", build_mask)
    clock("fill_holes_3d_shells", lambda: ndi.binary_fill_holes(shell))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="skip the host baseline")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--host_side", type=int, default=64)
    args = ap.parse_args()
    rec = {"device": {"side": args.side, **device_rows(args.side, args.repeats)}}
    print(json.dumps(rec["device"]), flush=True)
    if not args.quick:
        rec["device_at_host_side"] = {"side": args.host_side, **device_rows(args.host_side, args.repeats)}
        print(json.dumps(rec["device_at_host_side"]), flush=True)
        rec["host_scipy"] = {"side": args.host_side, **host_rows(args.host_side)}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
