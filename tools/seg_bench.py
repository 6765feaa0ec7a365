"""Measure the tissue segmentation (t2map.seg, t2fit_seg_*) in one process:

    python tools/seg_bench.py [--out profiles/r20_seg_bench.json] [--quick]

256^3 (--quick: 32 x 256 x 256), K = 8 classes, C = 2 channels, inside the brain mask of the synthetic volume.  Raw calls on
preallocated buffers, HIP events around each, the median of 7 after a warm-up:
  priors_ms   t2fit_seg_priors_dev at sigma = 2 voxels (17 taps per axis): three passes over K planes
  estep_ms    one t2fit_seg_estep_dev
  sums_ms     one t2fit_seg_sums_dev (the moments kernel and the reduce passes)
  call_ms     a default seg.segment_em call on device tensors (15 iterations, one host synchronisation each for the model)
Logical bytes, per voxel: priors 4 (labels) + 3 passes x (4 K read + 4 K written) less the x pass's read; E-step 4 K (p_old,
each plane counted once) + 4 K (pi) + 4 C (y) + 1 (mask) + 4 K (p_new); sums 4 K + 4 C + 1.  Beside them one 3-D TV iteration
of the first channel in the same process (two calls with eps = 0 and max_iter = 11 / 41, the difference over 30), the
yardstick of a stencil pass here, and the numpy statement of one E-step and one sums call on a 64^3 crop."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPEATS = 7


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
    from fetal_t2mapping_amd import _seg, synth
    from fetal_t2mapping_amd._gpu import current_stream, workspace
    from fetal_t2mapping_amd._lib import check, load

    lib = load()
    seg = t2.seg
    dev = torch.device("cuda", 0)
    shape, K, Cn = ((32, 256, 256) if args.quick else (256, 256, 256)), 8, 2
    n = int(np.prod(shape))
    echoes, mask, _ = synth.brain_volume_torch(shape, 6, seed=synth.SEED_BASE, device=dev)
    echoes = echoes.reshape((6,) + shape)
    y = echoes[[0, 5]].contiguous()
    mask = (mask.reshape(shape) != 0).to(torch.uint8).contiguous()
    # a label atlas of K classes: the first channel's intensity quantiles inside the mask, so every class has voxels
    inside = y[0][mask != 0]
    edges = torch.quantile(inside[:: max(1, inside.numel() // 1000000)], torch.linspace(0, 1, K + 1, device=dev)[1:-1])
    labels = torch.where(mask != 0, torch.bucketize(y[0], edges).to(torch.int32) + 1, torch.zeros((), dtype=torch.int32, device=dev))
    classes = np.arange(1, K + 1, dtype=np.int32)
    cls = (C.c_int32 * K)(*classes.tolist())
    taps = _seg.gauss_taps(2.0)
    tp, r = taps.ctypes.data_as(C.POINTER(C.c_double)), (len(taps) - 1) // 2
    need = C.c_size_t(0)
    check(lib.t2fit_seg_workspace_bytes(K, Cn, *shape, C.byref(need)))
    ws, ws_ptr = workspace(need.value, dev)
    prior = torch.empty((K,) + shape, dtype=torch.float32, device=dev)
    st = current_stream()
    rec = {"volume": "x".join(map(str, shape)), "classes": K, "channels": Cn, "mask_fraction": float(mask.float().mean()),
           "repeats": REPEATS, "statistic": "median", "device": torch.cuda.get_device_name(dev), "workspace_bytes": need.value}

    def row(name, ms, bytes_per_voxel):
        rec[name] = {"ms": ms, "logical_bytes": bytes_per_voxel * n, "bytes_per_voxel": bytes_per_voxel,
                     "GB_per_s": bytes_per_voxel * n / ms / 1e6}
        print(name, json.dumps(rec[name]), flush=True)

    row("priors", median_ms(lambda: check(lib.t2fit_seg_priors_dev(labels.data_ptr(), cls, K, *shape, tp, r, tp, r, tp, r,
                                                                    prior.data_ptr(), ws_ptr, st))), 4 + 3 * 8 * K - 4 * K)
    M = seg.effective_mask(y, mask)
    pi = seg.normalise_priors(prior, M, 1e-3)
    sums = torch.empty(K * _seg.n_moments(Cn), dtype=torch.float64, device=dev)
    sums_call = lambda p: check(lib.t2fit_seg_sums_dev(p.data_ptr(), y.data_ptr(), M.data_ptr(), K, Cn, *shape, sums.data_ptr(), ws_ptr, st))
    sums_call(pi)
    model = _seg.class_model(sums.cpu().numpy().reshape(K, -1), Cn, 1e-6)
    rows, live = _seg.pack_model(model)
    p_new = torch.empty_like(pi)
    estep_call = lambda: check(lib.t2fit_seg_estep_dev(pi.data_ptr(), pi.data_ptr(), y.data_ptr(), M.data_ptr(),
                                                       rows.ctypes.data_as(C.POINTER(C.c_double)), live.ctypes.data_as(C.POINTER(C.c_int32)),
                                                       0.5, K, Cn, *shape, p_new.data_ptr(), st))
    row("estep", median_ms(estep_call), 12 * K + 4 * Cn + 1)
    row("sums", median_ms(lambda: sums_call(p_new)), 4 * K + 4 * Cn + 1)
    rec["sums_share_of_an_iteration"] = rec["sums"]["ms"] / (rec["sums"]["ms"] + rec["estep"]["ms"])
    rec["live_classes"] = int(live.sum())
    call = median_ms(lambda: seg.segment_em(y, mask, prior, classes))
    res = seg.segment_em(y, mask, prior, classes)
    rec["segment_em_call"] = {"ms": call, "n_iter": int(res.n_iter), "ms_per_iteration": call / max(1, int(res.n_iter)),
                              "dead": [bool(d) for d in res.model.dead]}
    print("segment_em_call", json.dumps(rec["segment_em_call"]), flush=True)
    # the yardstick: one iteration of the 3-D TV pass on one volume of the same size
    one = y[:1].contiguous()
    out = torch.empty_like(one)
    t2.denoise_tv(one, 10.0, eps=0.0, max_iter=3, dims=3, out=out)
    ms = {m: min(timed(lambda: t2.denoise_tv(one, 10.0, eps=0.0, max_iter=m, dims=3, out=out))[0] for _ in range(3)) for m in (11, 41)}
    per_iter = (ms[41] - ms[11]) / 30.0
    rec["tv3d_iteration"] = {"ms": per_iter, "bytes_per_voxel": 4 + 2 * 3 * 4, "GB_per_s": (4 + 24) * n / per_iter / 1e6}
    print("tv3d_iteration", json.dumps(rec["tv3d_iteration"]), flush=True)
    if args.crop:
        c = args.crop
        lo = [(s - min(c, s)) // 2 for s in shape]
        sl = (slice(None),) + tuple(slice(a, a + c) for a in lo)
        yc, pc, pic, Mc = (t[sl].cpu().numpy() for t in (y, p_new, pi, M[None]))
        t0 = time.time()
        want = _seg.e_step(pic, pic, yc, Mc[0], model, 0.5)
        t_e = time.time() - t0
        t0 = time.time()
        s_np = _seg.moment_sums(want, yc, Mc[0])
        t_s = time.time() - t0
        got = seg.e_step(pic, pic, yc, Mc[0], model, 0.5)
        rec["statement"] = {"crop": list(yc.shape[1:]), "estep_numpy_s": t_e, "sums_numpy_s": t_s,
                            "estep_max_ulp": int(np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max()),
                            "sums_equal": bool(seg.moment_sums(want, yc, Mc[0]).tobytes() == s_np.tobytes())}
        print("statement", json.dumps(rec["statement"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
