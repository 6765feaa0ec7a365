"""Timing of the N4 bias-field correction on one MI355X -> profiles/r12_n4_bench.json (record only, no bar).

    python tools/n4_bench.py [--repeats 9] [--out profiles/r12_n4_bench.json] [--skip_host] [--shapes 57x256x256 256x256x256]

A three-class ball under a smooth field, at 256 x 256 x 57 (a raw stack) and at 256^3.  HIP events around the launches
after a warm-up, median of ``--repeats``:
  * one iteration per level (lattice sides 4, 5, 7, 11): t2fit_n4_histogram_dev, t2fit_n4_fit_dev and t2fit_n4_field_dev
    queued back to back with a fixed table, no copy -- the kernels of an iteration without its host half -- and each of
    the three alone; beside them the level's t2fit_n4_weights_dev;
  * a whole default ``n4_correct`` call: wall time, iterations per level, and the share of the wall time that is not
    kernels (the table on the host, the copies that wait for the stream), from the per-level kernel times above;
  * the numpy statement of one iteration on the host at sides 4 and 11, at the first shape only (a whole call of the
    statement takes minutes there).
No device, no number: the tool fails without a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def phantom(shape, seed=12):
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.linspace(-1, 1, nz), np.linspace(-1, 1, ny), np.linspace(-1, 1, nx), indexing="ij", sparse=True)
    r = np.sqrt(z * z + y * y + x * x)
    cls = (r < 0.9).astype(np.int8) + (r < 0.65) + (r < 0.4)
    vol = np.array([0.0, 300.0, 600.0, 1000.0])[cls] * np.exp(0.25 * x - 0.2 * y * y + 0.15 * z * x + 0.1 * z)
    vol = vol + np.random.default_rng(seed).normal(0.0, 5.0, shape)
    return np.where(cls > 0, np.maximum(vol, 1.0), 0.0).astype(np.float32), (cls > 0).astype(np.uint8)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--repeats", type=int, default=9)
    p.add_argument("--out", default="profiles/r12_n4_bench.json")
    p.add_argument("--shapes", nargs="+", default=["57x256x256", "256x256x256"], help="Z x Y x X")
    p.add_argument("--skip_host", action="store_true", help="do not time the numpy statement")
    args = p.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("n4_bench needs a HIP device: nothing is measured without one")
    from fetal_t2mapping_amd import _bias
    from fetal_t2mapping_amd import t2map
    from fetal_t2mapping_amd._gpu import current_stream
    from fetal_t2mapping_amd._gpu_bias import DeviceSteps

    dev = torch.device("cuda", 0)

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

    record = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "shapes": []}
    for at, text in enumerate(args.shapes):
        shape = tuple(int(v) for v in text.split("x"))
        vol, mask = phantom(shape)
        steps = DeviceSteps(vol, mask, dev)
        lib = steps.lib
        lo, hi = steps.range()
        slope = _bias.slope_of(lo, hi)
        table = _bias.sharpen_table(steps.histogram(float(lo), slope, _bias.BINS), lo, slope, 0.15)
        entry = {"shape": list(shape), "mask_voxels": int(mask.sum()), "levels": []}
        lattice = np.zeros((4, 4, 4))
        for level in range(4):
            if level:
                lattice = _bias.refine(lattice)
            steps.set_level(lattice)
            steps.table[:_bias.BINS].copy_(torch.from_numpy(table))
            vox, geo = steps.u.numel(), tuple(steps.u.shape)

            def hist():
                assert lib.t2fit_n4_histogram_dev(steps.u.data_ptr(), steps.m.data_ptr(), vox, float(lo), slope, _bias.BINS,
                                                  steps.hist.data_ptr(), current_stream()) == 0

            def fit():
                assert lib.t2fit_n4_fit_dev(steps.u.data_ptr(), steps.m.data_ptr(), *geo, steps.table.data_ptr(), float(lo), slope,
                                            _bias.BINS, steps.side, steps.omega.data_ptr(), steps.lat.data_ptr(), steps.delta.data_ptr(),
                                            steps.ptr, steps.nbytes, current_stream()) == 0

            def field():
                assert lib.t2fit_n4_field_dev(steps.lat.data_ptr(), steps.side, steps.u0.data_ptr(), steps.m.data_ptr(), *geo,
                                              steps.field.data_ptr(), steps.u.data_ptr(), steps.sums.data_ptr(), steps.rng.data_ptr(),
                                              steps.ptr, steps.nbytes, current_stream()) == 0

            def weights():
                assert lib.t2fit_n4_weights_dev(steps.m.data_ptr(), *geo, steps.side, steps.omega.data_ptr(), steps.ptr, steps.nbytes,
                                                current_stream()) == 0

            def iteration():
                hist(), fit(), field()

            entry["levels"].append({"side": steps.side, "iteration_ms": median_ms(iteration), "histogram_ms": median_ms(hist),
                                    "fit_ms": median_ms(fit), "field_ms": median_ms(field), "weights_ms": median_ms(weights)})
            lattice = np.zeros_like(lattice)  # (the timed fits moved the lattice: every level starts from zeros again)
        del steps
        t2map.bias.n4_correct(vol, mask, max_iter=(2, 2))  # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        found = t2map.bias.n4_correct(vol, mask)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        kernels = sum(n * lv["iteration_ms"] + lv["weights_ms"] for n, lv in zip(found.iterations, entry["levels"]))
        entry["whole_call"] = {"wall_ms": wall, "iterations": list(found.iterations), "kernel_ms_estimate": kernels,
                               "share_outside_kernels": 1.0 - kernels / wall}
        if at == 0 and not args.skip_host:
            host = _bias.HostSteps(vol, mask)
            entry["numpy_statement"] = {"threads": os.environ.get("OMP_NUM_THREADS"), "iteration_s": {}}
            for side in (4, 11):
                host.set_level(np.zeros((side,) * 3))
                t0 = time.perf_counter()
                h_lo, h_hi = host.range()
                h_slope = _bias.slope_of(h_lo, h_hi)
                host.fit(_bias.sharpen_table(host.histogram(float(h_lo), h_slope, _bias.BINS), h_lo, h_slope, 0.15), float(h_lo), h_slope)
                host.eval_field()
                entry["numpy_statement"]["iteration_s"][str(side)] = time.perf_counter() - t0
        record["shapes"].append(entry)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
    print(json.dumps(record))


if __name__ == "__main__":
    main()
