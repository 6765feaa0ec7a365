"""Timing of the non-rigid alignment (B-spline FFD under Mattes MI) on one MI355X -> profiles/r21_ffd_bench.json (record only,
no bar).

    python tools/ffd_bench.py [--part evaluation|registration|statement|all] [--repeats 9] [--out profiles/r21_ffd_bench.json]

``evaluation``: a 256^3 fixed volume against a 182 x 218 x 182 moving one (the MNI152 1 mm grid) at full resolution, 32 x 32
bins, lattice sides 7 and 11.  HIP events around the launches after a warm-up, median of ``--repeats``:
  * t2fit_ffd_joint_hist_dev and t2fit_ffd_gradient_dev, each alone; their sum is the device time of one evaluation;
  * beside them, in the same session, the unchanged affine Mattes evaluation (t2fit_register_joint_hist_dev and
    t2fit_register_mi_gradient_dev) and the ratios to it;
  * t2fit_ffd_warp_dev (linear) beside t2fit_resample_dev for the same A, and the ratio; t2fit_ffd_jacobian_dev.
``registration``: a whole default ``register_ffd`` on a deformed, remapped smooth phantom at 128^3: wall time, iterations.
``statement``: the numpy statement's evaluation on a 32^3 crop of that phantom (host time, for scale).
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

FIXED, MOVING = (256, 256, 256), (182, 218, 182)
P0 = np.array([0.05, -0.04, 0.06, 1.3, -0.8, 0.6, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])


def lattice(side, amplitude=1.5):
    return np.random.default_rng(side).uniform(-amplitude, amplitude, (3, side, side, side))


def median_ms(fn, repeats, events=True):
    import torch

    for _ in range(3):
        fn()
    out = []
    for _ in range(repeats):
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


def evaluation(args, record):
    import torch

    from fetal_t2mapping_amd import _abi
    from fetal_t2mapping_amd import _register as G
    from fetal_t2mapping_amd import _resample as R
    from fetal_t2mapping_amd._gpu import current_stream
    from fetal_t2mapping_amd._gpu_ffd import DeviceFFDPyramid

    dev = torch.device("cuda", 0)
    fixed = torch.from_numpy(blobs(FIXED, 51, width=(0.06, 0.12))).to(dev)
    moving = torch.from_numpy(blobs(MOVING, 52, width=(0.06, 0.12))).to(dev)
    fg, mg = centred(FIXED), centred(MOVING)
    fmask, mmask = (fixed > 20).to(torch.uint8), (moving > 20).to(torch.uint8)
    a = np.ascontiguousarray(R.index_affine(fg, mg, G.compose_affine(P0, np.zeros(3)))).reshape(12)
    a_ptr = a.ctypes.data_as(C.POINTER(C.c_double))
    pyramid = DeviceFFDPyramid(fixed, fmask, moving, mmask, dev)
    lib, level = pyramid.lib, pyramid.level(1)
    n_f = n_m = 32
    bins = pyramid.bins(level, n_f)
    lo_m, scale_m = pyramid.moving_range(level, n_m)
    hist, table_dev, sums, _, mptr, mbytes = pyramid._mi_buffers(fmask.shape, n_f, n_m)
    geo = (fmask.data_ptr(), *fmask.shape, moving.data_ptr(), mmask.data_ptr(), *moving.shape)
    cost, table = G.mattes_metric(pyramid.joint_hist(level, bins, n_f, n_m, lo_m, scale_m, a), n_f, n_m, scale_m)
    table_dev.copy_(torch.from_numpy(table.ravel()))
    out_f = torch.empty(FIXED, dtype=torch.float32, device=dev)
    jac = torch.empty(2, dtype=torch.float64, device=dev)

    def affine_hist():
        assert lib.t2fit_register_joint_hist_dev(bins.data_ptr(), *geo, a_ptr, n_f, n_m, lo_m, scale_m, hist.data_ptr(), current_stream()) == 0

    def affine_gradient():
        assert lib.t2fit_register_mi_gradient_dev(bins.data_ptr(), table_dev.data_ptr(), n_f, n_m, lo_m, scale_m, *geo, a_ptr,
                                                  sums.data_ptr(), mptr, mbytes, current_stream()) == 0

    def resample():
        assert lib.t2fit_resample_dev(moving.data_ptr(), _abi.RESAMPLE_F32, *moving.shape, a_ptr, out_f.data_ptr(), *FIXED, 1,
                                      _abi.INTERP_LINEAR, 0.0, 0, current_stream()) == 0

    base = {"affine_joint_hist_ms": median_ms(affine_hist, args.repeats), "affine_mi_gradient_ms": median_ms(affine_gradient, args.repeats),
            "resample_ms": median_ms(resample, args.repeats)}
    record["evaluation"] = {"fixed": list(FIXED), "moving": list(MOVING), "n_f": n_f, "n_m": n_m, "cost_affine": cost,
                            "fixed_mask_voxels": int(fmask.sum().item()), **base, "sides": []}
    for side in (7, 11):
        lat = torch.from_numpy(lattice(side)).to(dev)
        grad = torch.empty((3, side, side, side), dtype=torch.float64, device=dev)
        _, wptr, wbytes = pyramid._workspace(fmask.shape, side)

        def ffd_hist():
            assert lib.t2fit_ffd_joint_hist_dev(bins.data_ptr(), *geo, a_ptr, lat.data_ptr(), side, n_f, n_m, lo_m, scale_m, hist.data_ptr(),
                                                wptr, wbytes, current_stream()) == 0

        def ffd_gradient():
            assert lib.t2fit_ffd_gradient_dev(bins.data_ptr(), table_dev.data_ptr(), n_f, n_m, lo_m, scale_m, *geo, a_ptr, lat.data_ptr(),
                                              side, grad.data_ptr(), wptr, wbytes, current_stream()) == 0

        def ffd_warp():
            assert lib.t2fit_ffd_warp_dev(moving.data_ptr(), _abi.RESAMPLE_F32, *moving.shape, a_ptr, lat.data_ptr(), side, out_f.data_ptr(),
                                          *FIXED, _abi.INTERP_LINEAR, 0.0, wptr, wbytes, current_stream()) == 0

        def ffd_jacobian():
            assert lib.t2fit_ffd_jacobian_dev(lat.data_ptr(), side, fmask.data_ptr(), *FIXED, jac.data_ptr(), jac.data_ptr() + 8, wptr, wbytes,
                                              current_stream()) == 0

        def whole():
            phi = lat.cpu().numpy()
            h = pyramid.hist(level, bins, n_f, n_m, lo_m, scale_m, a, phi)
            _, t = G.mattes_metric(h, n_f, n_m, scale_m)
            pyramid.gradient(level, bins, t, n_m, lo_m, scale_m, a, phi)

        ms = {"side": side, "joint_hist_ms": median_ms(ffd_hist, args.repeats), "gradient_ms": median_ms(ffd_gradient, args.repeats),
              "warp_ms": median_ms(ffd_warp, args.repeats), "jacobian_ms": median_ms(ffd_jacobian, args.repeats),
              "evaluation_wall_ms": median_ms(whole, args.repeats, events=False)}
        ms["device_ms"] = ms["joint_hist_ms"] + ms["gradient_ms"]
        ms["hist_over_affine"] = ms["joint_hist_ms"] / base["affine_joint_hist_ms"]
        ms["gradient_over_affine"] = ms["gradient_ms"] / base["affine_mi_gradient_ms"]
        ms["device_over_affine"] = ms["device_ms"] / (base["affine_joint_hist_ms"] + base["affine_mi_gradient_ms"])
        ms["warp_over_resample"] = ms["warp_ms"] / base["resample_ms"]
        record["evaluation"]["sides"].append(ms)


def _phantom(shape):
    from fetal_t2mapping_amd import _ffd as F
    from fetal_t2mapping_amd import _register as G
    from fetal_t2mapping_amd import _resample as R

    g = centred(shape)
    base = blobs(shape, 53)
    remapped = ((900.0 - 700.0 * np.abs(base / base.max() - 0.45) / 0.55) * (base > 20)).astype(np.float32)
    true = G.compose([0.02, 0.015, -0.03, 1.0, -0.5, 0.8], np.zeros(3))
    moving = R.resample(remapped, R.index_affine(g, g, np.linalg.inv(true)), shape)
    fixed = F.warp(base, np.eye(3, 4), lattice(5, 3.5 * shape[0] / 32.0), shape)
    return fixed, moving, g, true


def registration(args, record):
    import torch

    from fetal_t2mapping_amd import t2map

    shape = (128, 128, 128)
    fixed, moving, g, true = _phantom(shape)
    masks = dict(fixed_mask=(fixed > 20).astype(np.uint8), moving_mask=(moving > 0).astype(np.uint8))
    d = [torch.from_numpy(v).cuda() for v in (fixed, moving)]
    dm = {k: torch.from_numpy(v).cuda() for k, v in masks.items()}

    class Start:  # the affine the deformation starts from: the true one
        transform = true

    t2map.register.register_ffd(d[0], d[1], g, g, affine=Start, schedule=((4, 4),), max_iter=2, **dm)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    found = t2map.register.register_ffd(d[0], d[1], g, g, affine=Start, **dm)
    torch.cuda.synchronize()
    record["registration"] = {"shape": list(shape), "schedule": [list(s) for s in found.schedule], "wall_ms": (time.perf_counter() - t0) * 1e3,
                              "iterations": list(found.iterations), "stops": list(found.stops), "cost": found.cost,
                              "min_jacobian": found.min_jacobian, "n_folded": found.n_folded}


def statement(args, record):
    from fetal_t2mapping_amd import _ffd as F
    from fetal_t2mapping_amd import _register as G
    from fetal_t2mapping_amd import _resample as R

    shape = (32, 32, 32)
    fixed, moving, g, true = _phantom(shape)
    fmask, mmask = (fixed > 20).astype(np.uint8), (moving > 0).astype(np.uint8)
    a = R.index_affine(g, g, true)
    lo_f, scale_f = G.bin_range(fixed, fmask, 32)
    bins = G.bin_volume(fixed, lo_f, scale_f, 32)
    lo_m, scale_m = G.moving_bin_range(moving, mmask, 32)
    phi = lattice(7, 0.5)
    t0 = time.perf_counter()
    h = F.joint_histogram(bins, moving, a, phi, 32, 32, lo_m, scale_m, fmask, mmask)
    t1 = time.perf_counter()
    _, table = G.mattes_metric(h, 32, 32, scale_m)
    t2 = time.perf_counter()
    F.gradient(bins, table, moving, a, phi, 32, lo_m, scale_m, fmask, mmask)
    t3 = time.perf_counter()
    record["statement"] = {"shape": list(shape), "side": 7, "joint_hist_ms": (t1 - t0) * 1e3, "gradient_ms": (t3 - t2) * 1e3}


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--part", choices=["evaluation", "registration", "statement", "all"], default="all")
    p.add_argument("--repeats", type=int, default=9)
    p.add_argument("--out", default="profiles/r21_ffd_bench.json")
    args = p.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("ffd_bench needs a HIP device: nothing is measured without one")
    record = {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            record = json.load(fh)
    record.update(device=torch.cuda.get_device_name(0), repeats=args.repeats)
    if args.part in ("evaluation", "all"):
        evaluation(args, record)
    if args.part in ("registration", "all"):
        registration(args, record)
    if args.part in ("statement", "all"):
        statement(args, record)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
    print(json.dumps(record))


if __name__ == "__main__":
    main()
