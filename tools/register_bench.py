"""Timing of the rigid registration on one MI355X -> profiles/r10_register_bench.json (record only, no bar).

    python tools/register_bench.py [--side 256] [--repeats 9] [--out profiles/r10_register_bench.json] [--skip_host]

HIP events around the calls after a warm-up, median of ``--repeats``:
  * one t2fit_register_sums_dev call at side^3 against side^3 with an oblique transform: ms and logical GB/s over the
    fixed volume, the two masks and the moving volume (each read once: 2 x 4 + 2 x 1 bytes per voxel);
  * a whole (4, 2, 1) registration of a blob phantom moved by a known transform: wall time, iterations per level, and
    the share of the wall time that is not the sums kernels (the 43-double copy, the synchronisation and the host
    arithmetic of every iteration), from the kernels' event time;
  * the numpy statement of the same sums call on the host (threads as OMP_NUM_THREADS / the machine allows).
No device, no number: the tool fails without a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--side", type=int, default=256)
    p.add_argument("--repeats", type=int, default=9)
    p.add_argument("--out", default="profiles/r10_register_bench.json")
    p.add_argument("--skip_host", action="store_true", help="do not time the numpy statement (minutes at 256^3)")
    args = p.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("register_bench needs a HIP device: nothing is measured without one")
    from fetal_t2mapping_amd import _register as G
    from fetal_t2mapping_amd import _resample as R
    from fetal_t2mapping_amd import t2map
    from fetal_t2mapping_amd._gpu_register import DevicePyramid

    n = args.side
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device="cuda").manual_seed(41)
    fixed = torch.rand((n, n, n), generator=gen, device=dev) * 1000.0
    moving = torch.rand((n, n, n), generator=gen, device=dev) * 1000.0
    ones = torch.ones((n, n, n), dtype=torch.uint8, device=dev)
    g = R.Geometry((n, n, n), (1, 1, 1), (-(n - 1) / 2.0,) * 3)
    t = G.compose([0.05, -0.04, 0.06, 1.3, -0.8, 0.6], np.zeros(3))
    a = R.index_affine(g, g, t)
    pyramid = DevicePyramid(fixed, ones, moving, ones, dev)
    level = pyramid.level(1)

    def timed_sums():
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        s = pyramid.sums(level, a)
        end.record()
        end.synchronize()
        return start.elapsed_time(end), s

    for _ in range(3):
        timed_sums()
    ms = sorted(timed_sums()[0] for _ in range(args.repeats))
    sums = timed_sums()[1]
    logical = n ** 3 * (2 * 4 + 2 * 1)
    record = {"device": torch.cuda.get_device_name(0), "side": n, "repeats": args.repeats,
              "sums_call": {"ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1], "includes": "kernels + 43-double copy",
                            "logical_bytes": logical, "logical_GBps": logical / (ms[len(ms) // 2] * 1e-3) / 1e9, "N": float(sums[0])}}

    # a whole registration: blobs moved by a known transform
    rng = np.random.default_rng(42)
    side = min(n, 128)
    gg = R.Geometry((side,) * 3, (1, 1, 1), (-(side - 1) / 2.0,) * 3)
    zz, yy, xx = np.meshgrid(*[np.arange(side) - (side - 1) / 2.0] * 3, indexing="ij")
    vol = np.zeros((side,) * 3)
    for c, s, amp in zip(rng.uniform(-0.25, 0.25, (9, 3)) * side, rng.uniform(0.05, 0.1, 9) * side, rng.uniform(300, 900, 9)):
        vol += amp * np.exp(-((xx - c[0]) ** 2 + (yy - c[1]) ** 2 + (zz - c[2]) ** 2) / (2 * s * s))
    vol = vol.astype(np.float32)
    true = G.compose(np.deg2rad([4.0, 3.0, -5.0]).tolist() + [2.5, -1.5, 2.0], np.zeros(3))
    mov, _ = t2map.resample_volume(torch.from_numpy(vol).to(dev), gg, like=gg, transform=np.linalg.inv(true))
    fx = torch.from_numpy(vol).to(dev)
    kernel_ms = [0.0]
    inner = DevicePyramid.sums

    def counted(self, lv, A):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = inner(self, lv, A)
        end.record()
        end.synchronize()
        kernel_ms[0] += start.elapsed_time(end)
        return out

    t2map.register.register_rigid(fx, mov, gg, gg)  # warm-up
    DevicePyramid.sums = counted
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    found = t2map.register.register_rigid(fx, mov, gg, gg)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    DevicePyramid.sums = inner
    mask = t2map.build_mask(fx).cpu().numpy()
    record["registration"] = {"side": side, "levels": [4, 2, 1], "iterations": list(found.iterations), "stops": list(found.stops),
                              "wall_ms": wall, "sums_calls_ms": kernel_ms[0],
                              "share_outside_the_sums_calls": 1.0 - kernel_ms[0] / wall,
                              "tre_mm": G.target_registration_error(found.transform, true, mask, gg), "metric": found.metric}
    if not args.skip_host:
        f_host, m_host = fixed.cpu().numpy(), moving.cpu().numpy()
        t0 = time.perf_counter()
        want = G.registration_sums(f_host, m_host, a)
        record["numpy_statement"] = {"s": time.perf_counter() - t0, "threads": os.environ.get("OMP_NUM_THREADS"),
                                     "bit_equal_to_device": bool(np.array_equal(want.view(np.uint64), sums.view(np.uint64)))}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
    print(json.dumps(record))


if __name__ == "__main__":
    main()
