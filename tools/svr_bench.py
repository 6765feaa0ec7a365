"""Measure slice-to-volume registration (t2fit_svr_sums_dev, t2map.register.register_slices, t2map.sr.reconstruct_svr) at the
headline size -- three 256 x 256 x 57 stacks of 1 x 1 x 4.5 mm against 256^3:

    (a) one batched evaluation: the 43 sums of all 171 slices, each under its own affine, in one call;
    (b) the same 171 slices as 171 calls of t2fit_register_sums_dev on one-slice volumes, the only way without (a);
        the two differ in their summation tree (and (b) has u_z = 0), so the counts must be equal and the largest
        relative difference of the other sums is reported;
    (c) one whole register_slices call from poses +-3 degrees / +-2 mm off: wall time, the device time of its
        evaluations (HIP events around every t2fit_svr_sums_dev call), the iteration counts;
    (d) reconstruct_svr with two rounds beside the plain reconstruct_sr of the same run (``--echoes`` echoes).

    python tools/svr_bench.py [--out profiles/r16_svr_bench.json] [--repeats 7]

Times are HIP events around a call on an otherwise idle stream after a warm-up, the median of the repeats; wall times are
time.perf_counter around a synchronised call.  All in one process."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from recon_bench import geometries  # noqa: E402  (same stacks as the merge's benchmark)
from sr_slice_bench import median_ms, motion  # noqa: E402


def smooth_volume(side, seed):
    """A float32 CUDA volume side^3: coarse noise interpolated up, smooth at the scale of a slice, positive."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    coarse = torch.rand((1, 1, side // 8, side // 8, side // 8), generator=g, device="cuda")
    fine = torch.nn.functional.interpolate(coarse, size=(side, side, side), mode="trilinear", align_corners=True)[0, 0]
    zz, yy, xx = torch.meshgrid(*[torch.linspace(-1, 1, side, device="cuda")] * 3, indexing="ij")
    return (fine * 1000.0 * ((xx * xx + yy * yy + zz * zz) < 0.7)).contiguous()


class Timing:
    """The library with HIP events around every t2fit_svr_sums_dev call."""

    def __init__(self, lib):
        self.lib, self.events = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name != "t2fit_svr_sums_dev":
            return fn

        def call(*args):
            import torch

            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rc = fn(*args)
            b.record()
            self.events.append((a, b))
            return rc

        return call

    def device_ms(self):
        import torch

        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in self.events]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--slices", type=int, default=57)
    ap.add_argument("--echoes", type=int, default=1, help="echoes of the reconstructions of (d)")
    args = ap.parse_args()
    side, n_sl, thick = args.side, args.slices, 4.5

    import torch

    import fetal_t2mapping_amd as t2
    from fetal_t2mapping_amd import _abi, _gpu_register as GR, _sr as S, _svr as V
    from fetal_t2mapping_amd._gpu import require, workspace

    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: this tool measures on the GPU")
    lib = require(*(_abi.SVR_SYMBOLS + _abi.REGISTER_SYMBOLS))
    dev = torch.device("cuda", 0)
    geoms = geometries(side, n_sl, thick)
    order, hi, _, _ = S.sr_plan(geoms)
    volume = smooth_volume(side, 0)
    stacks = {o: t2.resample_volume(volume, hi, like=geoms[o])[0].reshape(geoms[o].shape).contiguous() for o in order}
    masks = {o: (stacks[o] > 50.0).to(torch.uint8) for o in order}
    n = 3 * n_sl
    off = {o: motion(n_sl, 3.0, 2.0, 20 + i) for i, o in enumerate(order)}
    models = [V.SliceModel(geoms[o], masks[o].cpu().numpy(), hi) for o in order]
    a_all = np.stack([models[s].affine(k, off[o][k]) for s, o in enumerate(order) for k in range(n_sl)])
    s_of = np.repeat(np.arange(3, dtype=np.int32), n_sl)
    k_of = np.tile(np.arange(n_sl, dtype=np.int32), 3)
    rec = {"size": {"stacks": [3, n_sl, side, side], "spacing": [1.0, 1.0, thick], "volume": list(hi.shape), "slices": n},
           "poses": "components uniform in +-3 degrees / +-2 mm about each slice's mask centroid", "repeats": args.repeats}
    rows = []

    def row(what, **kw):
        rows.append({"what": what, **kw})
        print(json.dumps(rows[-1]), flush=True)

    # (a) one batched evaluation, below the Python wrapper: the table is on the device
    slices = GR.DeviceSlices([stacks[o] for o in order], [masks[o] for o in order], volume, None, n, dev)
    got_a = slices.sums(a_all, s_of, k_of).copy()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def batched():
        rc = lib.t2fit_svr_sums_dev(3, slices.fixed_ptrs, slices.mask_ptrs, slices.lo_size, slices.moving.data_ptr(), None, *slices.moving.shape,
                                    slices.table.data_ptr(), n, slices.out.data_ptr(), slices.ws_ptr, slices.ws_bytes, stream)
        assert rc == 0

    ms_a = median_ms(batched, args.repeats)
    row("(a) one batched evaluation of all slices: t2fit_svr_sums_dev", ms_median=ms_a, launches=2)
    # (b) one t2fit_register_sums_dev call per slice, on one-slice volumes
    need = C.c_size_t(0)
    assert lib.t2fit_register_workspace_bytes(1, side, side, C.byref(need)) == 0
    ws, ws_ptr = workspace(need.value, dev)
    ones = torch.ones(tuple(volume.shape), dtype=torch.uint8, device=dev)
    out_b = torch.zeros((n, 43), dtype=torch.float64, device=dev)
    shifted = a_all.copy()
    shifted[:, :, 3] = shifted[:, :, 3] + shifted[:, :, 2] * k_of[:, None]  # (ix, iy, 0) lands where (ix, iy, k) does
    per_slice = []
    for r in range(n):
        o = order[s_of[r]]
        at = int(k_of[r]) * side * side
        per_slice.append((stacks[o].data_ptr() + 4 * at, masks[o].data_ptr() + at,
                          np.ascontiguousarray(shifted[r]).ctypes.data_as(C.POINTER(C.c_double)), out_b.data_ptr() + 8 * 43 * r))

    def one_by_one():
        for fixed, fmask, a, out in per_slice:
            rc = lib.t2fit_register_sums_dev(fixed, fmask, 1, side, side, volume.data_ptr(), ones.data_ptr(), *volume.shape, a, out, ws_ptr,
                                             need.value, stream)
            assert rc == 0

    ms_b = median_ms(one_by_one, args.repeats)
    row("(b) the same slices, one t2fit_register_sums_dev call each on a one-slice volume", ms_median=ms_b, launches=2 * n,
        ratio_b_over_a=ms_b / ms_a)
    got_b = out_b.cpu().numpy()
    scale = np.maximum(np.abs(got_a), 1.0)
    # u_z = 0 in (b): only the sums without u_z compare; N must be equal
    cols = [q for q in range(42) if q < 6 or (q - 6) % 4 != 2]
    rec["a_against_b"] = {"N_equal": bool(np.array_equal(got_a[:, 0], got_b[:, 0])), "counted_voxels": float(got_a[:, 0].sum()),
                          "largest_relative_difference": float(np.max(np.abs(got_a[:, cols] - got_b[:, cols]) / scale[:, cols]))}
    print(json.dumps(rec["a_against_b"]), flush=True)
    # (c) one whole register_slices call
    timing = Timing(lib)
    real_require = GR.require
    GR.require = lambda *symbols: timing
    try:
        kw = dict(stack_masks=masks, init=off)
        t2.register.register_slices(stacks, geoms, volume, hi, max_iter=2, **kw)  # warm-up
        timing.events.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        found = t2.register.register_slices(stacks, geoms, volume, hi, **kw)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1000.0
        device = timing.device_ms()
    finally:
        GR.require = real_require
    its = np.concatenate([found.iterations[o] for o in order])
    status = [s for o in order for s in found.status[o]]
    err = {o: float(np.mean(np.abs(found.parameters[o][:, 3:]))) for o in order}
    row("(c) one register_slices call", wall_ms=wall, evaluations=len(device), device_ms_of_the_evaluations=float(np.sum(device)),
        share_outside_the_kernels=1.0 - float(np.sum(device)) / wall, iterations_min_median_max=[int(its.min()), float(np.median(its)), int(its.max())],
        status={s: status.count(s) for s in sorted(set(status))}, mean_abs_translation_left_mm=err)
    # (d) two rounds of reconstruct_svr beside reconstruct_sr
    multi = {o: stacks[o][None].repeat(args.echoes, 1, 1, 1).contiguous() for o in order}

    def wall_ms(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1000.0

    ms_sr = wall_ms(lambda: t2.sr.reconstruct_sr(multi, geoms))
    ms_svr = wall_ms(lambda: t2.sr.reconstruct_svr(multi, geoms, rounds=2, slice_masks=masks))
    row(f"(d) reconstruct_sr, default call, {args.echoes} echo(es)", wall_ms=ms_sr)
    row(f"(d) reconstruct_svr, two rounds, {args.echoes} echo(es)", wall_ms=ms_svr, ratio_to_reconstruct_sr=ms_svr / ms_sr)
    rec["rows"] = rows
    rec["a_faster_than_b"] = bool(ms_a < ms_b)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    if not rec["a_faster_than_b"] or not rec["a_against_b"]["N_equal"]:
        raise SystemExit("(a) is not faster than (b), or they count other voxels")


if __name__ == "__main__":
    main()
