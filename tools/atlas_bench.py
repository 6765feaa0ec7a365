"""Timing of the correlation-ratio affine registration on one MI355X -> profiles/r11_atlas_bench.json (record only, no bar).

    python tools/atlas_bench.py [--repeats 9] [--out profiles/r11_atlas_bench.json] [--skip_host] [--bins 32]

A 182 x 218 x 182 moving volume (the MNI152 1 mm grid) against a 256^3 fixed volume, at every level of the (4, 2, 1)
pyramid.  HIP events around the launches after a warm-up, median of ``--repeats``:
  * one correlation-ratio evaluation: t2fit_register_binned_sums_dev (with the table) and t2fit_register_sums_lut_dev,
    queued back to back, no copy;
  * beside it one evaluation of the unchanged squared-correlation sums, t2fit_register_sums_dev, at the same sizes, and
    the ratio of the two;
  * a whole ``register_affine`` call (12 degrees of freedom, both metrics) on a smooth phantom at half the size: wall
    time and iterations per level;
  * the numpy statement of one evaluation at the coarsest level on the host.
No device, no number: the tool fails without a GPU."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FIXED_SHAPE, MOVING_SHAPE = (256, 256, 256), (182, 218, 182)  # (Z, Y, X)


def centred(shape, spacing=1.0):
    from fetal_t2mapping_amd import _resample as R

    return R.Geometry(shape[::-1], (spacing,) * 3, tuple(-(np.array(shape[::-1]) - 1) * spacing / 2.0))


def blobs(shape, seed, n=9, width=(0.05, 0.1)):
    rng = np.random.default_rng(seed)
    axes = [np.arange(s) - (s - 1) / 2.0 for s in shape]
    zz, yy, xx = np.meshgrid(*axes, indexing="ij", sparse=True)
    vol = np.zeros(shape)
    for c, s, amp in zip(rng.uniform(-0.25, 0.25, (n, 3)) * min(shape), rng.uniform(width[0], width[1], n) * min(shape), rng.uniform(300, 900, n)):
        vol += amp * np.exp(-((xx - c[0]) ** 2 + (yy - c[1]) ** 2 + (zz - c[2]) ** 2) / (2 * s * s))
    return vol.astype(np.float32)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--repeats", type=int, default=9)
    p.add_argument("--bins", type=int, default=32)
    p.add_argument("--out", default="profiles/r11_atlas_bench.json")
    p.add_argument("--skip_host", action="store_true", help="do not time the numpy statement")
    args = p.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("atlas_bench needs a HIP device: nothing is measured without one")
    from fetal_t2mapping_amd import _register as G
    from fetal_t2mapping_amd import _resample as R
    from fetal_t2mapping_amd import t2map
    from fetal_t2mapping_amd._gpu import current_stream
    from fetal_t2mapping_amd._gpu_register import DeviceAffinePyramid

    dev = torch.device("cuda", 0)
    n_bins = args.bins
    # wider blobs: the masks (> 20) cover some 30 % of the volumes, a head in its field of view; N says how many voxels count
    fixed = torch.from_numpy(blobs(FIXED_SHAPE, 51, width=(0.06, 0.12))).to(dev)
    moving = torch.from_numpy(blobs(MOVING_SHAPE, 52, width=(0.06, 0.12))).to(dev)
    fg, mg = centred(FIXED_SHAPE), centred(MOVING_SHAPE)
    fmask, mmask = (fixed > 20).to(torch.uint8), (moving > 20).to(torch.uint8)
    p0 = np.array([0.05, -0.04, 0.06, 1.3, -0.8, 0.6, 0.03, -0.02, 0.01, 0.01, 0.0, -0.01])
    pyramid = DeviceAffinePyramid(fixed, fmask, moving, mmask, dev)
    lib = pyramid.lib

    def median_ms(fn):
        for _ in range(3):
            fn()
        out = []
        for _ in range(args.repeats):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            end.record()
            end.synchronize()
            out.append(start.elapsed_time(end))
        return sorted(out)[len(out) // 2]

    record = {"device": torch.cuda.get_device_name(0), "fixed": list(FIXED_SHAPE), "moving": list(MOVING_SHAPE), "bins": n_bins,
              "repeats": args.repeats, "levels": []}
    coarse = None
    for s in (4, 2, 1):
        level = pyramid.level(s)
        lf, lfm, lm, lmm, _, ptr, nbytes = level
        bins = pyramid.bins(level, n_bins)
        a = np.ascontiguousarray(R.index_affine(G.level_geometry(fg, s), G.level_geometry(mg, s), G.compose_affine(p0, np.zeros(3)))).reshape(12)
        a_ptr = a.ctypes.data_as(C.POINTER(C.c_double))
        out, _, bptr, bbytes = pyramid._buffers(lfm.shape, n_bins)
        binned, lut, sums = out.data_ptr(), out.data_ptr() + 16 * n_bins, out.data_ptr() + 24 * n_bins
        geo = (lfm.data_ptr(), *lfm.shape, lm.data_ptr(), lmm.data_ptr(), *lm.shape)

        def cr_binned():
            assert lib.t2fit_register_binned_sums_dev(bins.data_ptr(), *geo, a_ptr, n_bins, binned, lut, bptr, bbytes, current_stream()) == 0

        def cr_lut():
            assert lib.t2fit_register_sums_lut_dev(bins.data_ptr(), lut, n_bins, *geo, a_ptr, sums, ptr, nbytes, current_stream()) == 0

        def cr():
            cr_binned(), cr_lut()

        def ncc():
            assert lib.t2fit_register_sums_dev(lf.data_ptr(), *geo, a_ptr, pyramid.out.data_ptr(), ptr, nbytes, current_stream()) == 0

        ms = {"cr_ms": median_ms(cr), "cr_binned_and_table_ms": median_ms(cr_binned), "cr_sums_lut_ms": median_ms(cr_lut),
              "ncc_ms": median_ms(ncc)}
        host = out.cpu().numpy()
        ms.update(shrink=s, fixed_mask_voxels=int(lfm.sum().item()), fixed=list(lf.shape), moving=list(lm.shape), cr_over_ncc=ms["cr_ms"] / ms["ncc_ms"],
                  N=float(host[3 * n_bins]), bins_populated=int(np.count_nonzero(host[:n_bins])),
                  CR=G.cr_metric(host[:2 * n_bins], host[3 * n_bins:])[0])
        record["levels"].append(ms)
        if s == 4:
            coarse = (bins.cpu().numpy(), lm.cpu().numpy(), a.reshape(3, 4), lfm.cpu().numpy(), lmm.cpu().numpy(), host)

    # a whole registration: a smooth phantom, remapped, moved by a known affine, at 128 x 128 x 128
    shape = (128, 128, 128)
    g = centred(shape)
    subject = blobs(shape, 53)
    remapped = ((900.0 - 700.0 * np.abs(subject / subject.max() - 0.45) / 0.55) * (subject > 20)).astype(np.float32)
    true = G.compose_affine([0.07, 0.05, -0.09, 2.5, -1.5, 2.0, 0.05, -0.05, 0.04, 0.03, -0.02, 0.025], np.zeros(3))
    template, _ = t2map.resample_volume(torch.from_numpy(remapped).to(dev), g, like=g, transform=np.linalg.inv(true))
    subject_dev = torch.from_numpy(subject).to(dev)
    masks = dict(fixed_mask=(subject_dev > 20).to(torch.uint8), moving_mask=(template > 0).to(torch.uint8))
    record["registration"] = {"shape": list(shape), "levels": [4, 2, 1], "dof": 12}
    for metric in ("cr", "ncc"):
        t2map.register.register_affine(subject_dev, template, g, g, metric=metric, bins=n_bins, levels=(4,), max_iter=2, **masks)  # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        found = t2map.register.register_affine(subject_dev, template, g, g, metric=metric, bins=n_bins, **masks)
        torch.cuda.synchronize()
        record["registration"][metric] = {
            "wall_ms": (time.perf_counter() - t0) * 1e3, "iterations": list(found.iterations), "stops": list(found.stops),
            "metric": found.metric, "tre_mm": G.target_registration_error(found.transform, true, masks["fixed_mask"].cpu().numpy(), g),
            "start_tre_mm": G.target_registration_error(np.eye(4), true, masks["fixed_mask"].cpu().numpy(), g)}

    if not args.skip_host:
        bins_h, moving_h, a_h, fm_h, mm_h, host = coarse
        t0 = time.perf_counter()
        binned_h = G.binned_sums(bins_h, moving_h, a_h, n_bins, fm_h, mm_h)
        sums_h = G.registration_sums_lut(bins_h, G.lut_from_binned(binned_h), moving_h, a_h, fm_h, mm_h)
        record["numpy_statement"] = {"level": 4, "s": time.perf_counter() - t0, "threads": os.environ.get("OMP_NUM_THREADS"),
                                     "bit_equal_to_device": bool(np.array_equal(np.r_[binned_h, sums_h].view(np.uint64),
                                                                                np.r_[host[:2 * n_bins], host[3 * n_bins:]].view(np.uint64)))}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
    print(json.dumps(record))


if __name__ == "__main__":
    main()
