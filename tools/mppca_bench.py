"""Measure the MP-PCA denoiser (t2map.denoise_mppca, t2fit_mppca_dev) in one process:

    python tools/mppca_bench.py [--out profiles/r19_mppca_bench.json] [--quick]

256^3 x 8 TE (--quick: 32 x 256 x 256 x 8), with the brain mask of the synthetic volume and with none; dims 2 / radius 2,
dims 3 / radius 1 and dims 3 / radius 2.  Raw calls on preallocated buffers, HIP events around each, the median of 7 after a
warm-up:
  eigen_ms      the estimate-only call (out_dev NULL): the eigen kernel alone, without its projector stores
  call_ms       the denoising call: the eigen kernel with its projector stores, then the aggregate kernel
  aggregate_ms  call_ms - eigen_ms: the aggregate kernel plus the projector stores of the eigen kernel
Logical bytes of that last part, with P = 8 * nTE (nTE + 1) / 2 * centres: P written once and read once, the processed flags,
the stack read once and written once.  Then a whole denoise_tv(joint=True) call at sqrt(8) sigma (the defaults otherwise) as
the yardstick a user would compare with, and the numpy statement on a 64^3 crop with its sweep histogram."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPEATS = 7
CONFIGS = ((2, 2), (3, 1), (3, 2))  # (dims, radius)


def timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def median_ms(fn):
    fn()  # warm-up
    return float(np.median([timed(fn)[0] for _ in range(REPEATS)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--crop", type=int, default=64, help="side of the crop the numpy statement runs on (0: skip)")
    args = ap.parse_args()

    import torch

    import fetal_t2mapping_amd as t2
    from fetal_t2mapping_amd import _abi, _mppca, synth
    from fetal_t2mapping_amd._gpu import current_stream, workspace
    from fetal_t2mapping_amd._gpu_mppca import mppca_params
    from fetal_t2mapping_amd._lib import check, load

    lib = load()
    dev = torch.device("cuda", 0)
    shape, n_te = ((32, 256, 256) if args.quick else (256, 256, 256)), 8
    echoes, mask, _ = synth.brain_volume_torch(shape, n_te, seed=synth.SEED_BASE, device=dev)
    echoes, mask = echoes.reshape((n_te,) + shape).contiguous(), (mask.reshape(shape) != 0).to(torch.uint8).contiguous()
    sigma_bg, _ = t2.estimate_background_sigma(echoes, mask)
    out = torch.empty_like(echoes)
    sig = torch.empty(shape, dtype=torch.float32, device=dev)
    rank = torch.empty(shape, dtype=torch.uint8, device=dev)
    vol = int(np.prod(shape))
    rec = {"stack": "x".join(map(str, shape)) + f"x{n_te}", "mask_fraction": float(mask.float().mean()), "repeats": REPEATS,
           "statistic": "median", "device": torch.cuda.get_device_name(dev), "background_sigma": sigma_bg,
           "occupancy_choice": "V in registers (234 VGPRs at 8 echoes, 2 waves per SIMD, no LDS, no scratch)", "gpu": [], "statement": []}
    for dims, r in CONFIGS:
        par = mppca_params(r, dims)
        need = C.c_size_t()
        check(lib.t2fit_mppca_workspace_bytes(C.byref(par), n_te, *shape, C.byref(need)))
        ws, ws_ptr = workspace(need.value, dev)
        centres = (shape[0] - 2 * r if dims == 3 else shape[0]) * (shape[1] - 2 * r) * (shape[2] - 2 * r)
        p_bytes = 8 * (n_te * (n_te + 1) // 2) * centres
        for label, m in (("brain mask", mask), ("no mask", None)):
            mp = None if m is None else m.data_ptr()
            st = current_stream()
            eigen = median_ms(lambda: check(lib.t2fit_mppca_dev(C.byref(par), echoes.data_ptr(), mp, None, sig.data_ptr(),
                                                                 rank.data_ptr(), n_te, *shape, None, 0, st)))
            call = median_ms(lambda: check(lib.t2fit_mppca_dev(C.byref(par), echoes.data_ptr(), mp, out.data_ptr(), sig.data_ptr(),
                                                                rank.data_ptr(), n_te, *shape, ws_ptr, need.value, st)))
            nbytes = 2 * p_bytes + centres + 2 * 4 * n_te * vol
            seen = sig[sig > 0]
            row = {"dims": dims, "radius": r, "window": (2 * r + 1) ** dims, "mask": label, "centres": centres,
                   "workspace_bytes": need.value, "eigen_ms": eigen, "call_ms": call, "aggregate_ms": call - eigen,
                   "aggregate_logical_bytes": nbytes, "aggregate_TB_per_s": nbytes / max(call - eigen, 1e-9) / 1e9,
                   "median_sigma": float(seen.median()) if seen.numel() else 0.0,
                   "mean_rank": float(rank[sig > 0].float().mean()) if seen.numel() else 0.0}
            rec["gpu"].append(row)
            print(json.dumps(row), flush=True)
        del ws
    w = float(np.sqrt(8.0)) * sigma_bg
    ms = median_ms(lambda: t2.denoise_tv(echoes, w, out=out, joint=True))
    n_iter = t2.denoise_tv(echoes, w, out=out, joint=True, return_info=True)[1]["n_iter"].cpu().numpy()
    rec["tv_joint_call"] = {"weight": "sqrt8sigma", "weight_value": w, "call_ms": ms, "n_iter_mean": float(n_iter.mean()),
                            "n_iter_max": int(n_iter.max())}
    print(json.dumps(rec["tv_joint_call"]), flush=True)
    if args.crop:
        c = args.crop
        lo = [(s - min(c, s)) // 2 for s in shape]
        crop = echoes[:, lo[0]:lo[0] + c, lo[1]:lo[1] + c, lo[2]:lo[2] + c].cpu().numpy()
        for dims, r in CONFIGS:
            t0 = time.time()
            parts = _mppca.mppca_parts(crop, r, dims)
            dt = time.time() - t0
            got = t2.denoise_mppca(crop, radius=r, dims=dims)
            row = {"dims": dims, "radius": r, "crop": list(crop.shape), "numpy_s": dt,
                   "sweep_histogram": np.bincount(parts["sweeps"].ravel(), minlength=_mppca.MAX_SWEEPS + 1).tolist(),
                   "device_equals_statement": bool(got.tobytes() == parts["out"].tobytes())}
            rec["statement"].append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
