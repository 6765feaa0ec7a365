"""Timing of the Mattes mutual-information registration on one MI355X -> profiles/r13_mi_bench.json (record only, no bar).

    python tools/mi_bench.py [--part evaluation|registration|all] [--repeats 9] [--out profiles/r13_mi_bench.json]

``evaluation``: a 256^3 moving volume against a 256^3 fixed one at full resolution, 32 x 32 and 64 x 64 bins.  HIP events
around the launches after a warm-up, median of ``--repeats``:
  * t2fit_register_joint_hist_dev and t2fit_register_mi_gradient_dev, each alone; their sum is the device time of one
    evaluation, and ``evaluation_wall_ms`` the whole evaluation as the optimizer runs it (histogram, copy back, metric
    and table on the host, upload, gradient sums, copy back);
  * the histogram again with a moving volume of one value (every voxel adds to the same four entries of its row) and of
    white noise (the entries spread): what same-address serialisation of the LDS atomics costs;
  * beside them, in the same session, one evaluation of the unchanged correlation ratio (t2fit_register_binned_sums_dev
    and t2fit_register_sums_lut_dev) and of the unchanged 43 sums.
``registration``: a whole ``register_rigid`` call (6 parameters, levels 4 / 2 / 1) on a remapped smooth phantom at 128^3,
metric 'mattes' and, on the same pair, 'corr': wall time, iterations per level, target registration error.
Each part updates its own keys of the JSON file, so the parts may run as separate steps.  No device, no number."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from atlas_bench import blobs, centred  # noqa: E402  (the phantom of tools/atlas_bench.py)

SHAPE = (256, 256, 256)


def evaluation(args, record):
    import torch

    from fetal_t2mapping_amd import _register as G
    from fetal_t2mapping_amd import _resample as R
    from fetal_t2mapping_amd._gpu import current_stream
    from fetal_t2mapping_amd._gpu_register import DeviceAffinePyramid

    dev = torch.device("cuda", 0)
    fixed = torch.from_numpy(blobs(SHAPE, 51, width=(0.06, 0.12))).to(dev)
    moving = torch.from_numpy(blobs(SHAPE, 52, width=(0.06, 0.12))).to(dev)
    g = centred(SHAPE)
    fmask, mmask = (fixed > 20).to(torch.uint8), (moving > 20).to(torch.uint8)
    p0 = np.array([0.05, -0.04, 0.06, 1.3, -0.8, 0.6, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    a = np.ascontiguousarray(R.index_affine(g, g, G.compose_affine(p0, np.zeros(3)))).reshape(12)
    a_ptr = a.ctypes.data_as(C.POINTER(C.c_double))
    pyramid = DeviceAffinePyramid(fixed, fmask, moving, mmask, dev)
    lib = pyramid.lib
    level = pyramid.level(1)
    _, _, _, _, _, ptr, nbytes = level
    geo = (fmask.data_ptr(), *fmask.shape, moving.data_ptr(), mmask.data_ptr(), *moving.shape)

    def median_ms(fn, events=True):
        for _ in range(3):
            fn()
        out = []
        for _ in range(args.repeats):
            if events:
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                fn()
                end.record()
                end.synchronize()
                out.append(start.elapsed_time(end))
            else:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                out.append((time.perf_counter() - t0) * 1e3)
        return sorted(out)[len(out) // 2]

    record["evaluation"] = {"fixed": list(SHAPE), "moving": list(SHAPE), "fixed_mask_voxels": int(fmask.sum().item()), "pairs": []}
    flat = torch.full(SHAPE, 400.0, dtype=torch.float32, device=dev)
    noise = torch.from_numpy(np.random.default_rng(7).uniform(0.0, 900.0, SHAPE).astype(np.float32)).to(dev)
    for n_f, n_m in ((32, 32), (64, 64)):
        bins = pyramid.bins(level, n_f)
        lo_m, scale_m = pyramid.moving_range(level, n_m)
        hist, table_dev, sums, _, mptr, mbytes = pyramid._mi_buffers(fmask.shape, n_f, n_m)

        def joint_hist(vol=moving, lo=lo_m, scale=scale_m):
            assert lib.t2fit_register_joint_hist_dev(bins.data_ptr(), fmask.data_ptr(), *fmask.shape, vol.data_ptr(), mmask.data_ptr(),
                                                     *vol.shape, a_ptr, n_f, n_m, lo, scale, hist.data_ptr(), current_stream()) == 0

        def gradient():
            assert lib.t2fit_register_mi_gradient_dev(bins.data_ptr(), table_dev.data_ptr(), n_f, n_m, lo_m, scale_m, *geo, a_ptr,
                                                      sums.data_ptr(), mptr, mbytes, current_stream()) == 0

        def whole():
            h = pyramid.joint_hist(level, bins, n_f, n_m, lo_m, scale_m, a)
            cost, table = G.mattes_metric(h, n_f, n_m, scale_m)
            pyramid.mi_sums(level, bins, table, n_m, lo_m, scale_m, a)
            return cost

        cost = whole()
        out, _, bptr, bbytes = pyramid._buffers(fmask.shape, n_f)
        binned, lut, s43 = out.data_ptr(), out.data_ptr() + 16 * n_f, out.data_ptr() + 24 * n_f

        def cr():
            assert lib.t2fit_register_binned_sums_dev(bins.data_ptr(), *geo, a_ptr, n_f, binned, lut, bptr, bbytes, current_stream()) == 0
            assert lib.t2fit_register_sums_lut_dev(bins.data_ptr(), lut, n_f, *geo, a_ptr, s43, ptr, nbytes, current_stream()) == 0

        def ncc():
            assert lib.t2fit_register_sums_dev(fixed.data_ptr(), *geo, a_ptr, pyramid.out.data_ptr(), ptr, nbytes, current_stream()) == 0

        ms = {"n_f": n_f, "n_m": n_m, "joint_hist_ms": median_ms(joint_hist), "mi_gradient_ms": median_ms(gradient),
              "evaluation_wall_ms": median_ms(whole, events=False),
              "joint_hist_constant_moving_ms": median_ms(lambda: joint_hist(flat, 0.0, 0.0)),
              "joint_hist_noise_moving_ms": median_ms(lambda: joint_hist(noise, 0.0, (n_m - 4) / 900.0)),
              "cr_ms": median_ms(cr), "ncc_ms": median_ms(ncc), "cost": cost}
        ms["device_ms"] = ms["joint_hist_ms"] + ms["mi_gradient_ms"]
        ms["device_over_cr"] = ms["device_ms"] / ms["cr_ms"]
        record["evaluation"]["pairs"].append(ms)


def registration(args, record):
    import torch

    from fetal_t2mapping_amd import _register as G
    from fetal_t2mapping_amd import t2map

    dev = torch.device("cuda", 0)
    shape = (128, 128, 128)
    g = centred(shape)
    subject = blobs(shape, 53)
    remapped = ((900.0 - 700.0 * np.abs(subject / subject.max() - 0.45) / 0.55) * (subject > 20)).astype(np.float32)
    true = G.compose([0.07, 0.05, -0.09, 2.5, -1.5, 2.0], np.zeros(3))
    moving, _ = t2map.resample_volume(torch.from_numpy(remapped).to(dev), g, like=g, transform=np.linalg.inv(true))
    fixed = torch.from_numpy(subject).to(dev)
    masks = dict(fixed_mask=(fixed > 20).to(torch.uint8), moving_mask=(moving > 0).to(torch.uint8))
    fmask_host = masks["fixed_mask"].cpu().numpy()
    record["registration"] = {"shape": list(shape), "levels": [4, 2, 1], "parameters": 6,
                              "start_tre_mm": G.target_registration_error(np.eye(4), true, fmask_host, g)}
    for metric in ("mattes", "corr"):
        t2map.register.register_rigid(fixed, moving, g, g, metric=metric, levels=(4,), max_iter=2, **masks)  # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        found = t2map.register.register_rigid(fixed, moving, g, g, metric=metric, **masks)
        torch.cuda.synchronize()
        record["registration"][metric] = {"wall_ms": (time.perf_counter() - t0) * 1e3, "iterations": list(found.iterations),
                                          "stops": list(found.stops), "metric": found.metric,
                                          "tre_mm": G.target_registration_error(found.transform, true, fmask_host, g)}


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--part", choices=["evaluation", "registration", "all"], default="all")
    p.add_argument("--repeats", type=int, default=9)
    p.add_argument("--out", default="profiles/r13_mi_bench.json")
    args = p.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("mi_bench needs a HIP device: nothing is measured without one")
    record = {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            record = json.load(fh)
    record.update(device=torch.cuda.get_device_name(0), repeats=args.repeats)
    if args.part in ("evaluation", "all"):
        evaluation(args, record)
    if args.part in ("registration", "all"):
        registration(args, record)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
    print(json.dumps(record))


if __name__ == "__main__":
    main()
