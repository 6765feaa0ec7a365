"""Measure the vector-valued (joint) TV denoiser (t2map.denoise_tv(joint=True)) beside the scalar one, in one process:

    python tools/tvj_bench.py [--out profiles/r18_tvj_bench.json] [--quick]

256^3 x 8 TE (--quick: 64 x 256 x 256 x 8).  One iteration, joint and scalar, 2-D / 3-D x f32 / f64: two calls with eps = 0 and
max_iter = 11 / 41, HIP events around each, the median of 7 after a warm-up; the difference over 30 is one pass + one reduce
launch.  Traffic per iteration is arithmetic, with e = sizeof(T) and C channels:
  scalar: voxels * (4 + 2 * dims * e)
  joint:  voxels * ((2 - 1 / C) * (4 + dims * e) + dims * e)   (f and p read twice, the last channel once; p written once)
Then a whole call (dims = 2, f32, the defaults) at 1 sigma and at sqrt(8) sigma, joint and scalar."""
import argparse
import json
import os
import sys

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
    args = ap.parse_args()

    import torch

    import fetal_t2mapping_amd as t2
    from fetal_t2mapping_amd import synth

    dev = torch.device("cuda", 0)
    shape, n_te = ((64, 256, 256) if args.quick else (256, 256, 256)), 8
    echoes, mask, _ = synth.brain_volume_torch(shape, n_te, seed=synth.SEED_BASE, device=dev)
    echoes, mask = echoes.reshape((n_te,) + shape), mask.reshape(shape)
    sigma, _ = t2.estimate_background_sigma(echoes, mask)
    out = torch.empty_like(echoes)
    vox = echoes.numel()
    rec = {"stack": "x".join(map(str, shape)) + f"x{n_te}", "sigma": sigma, "repeats": REPEATS, "statistic": "median",
           "device": torch.cuda.get_device_name(dev), "pass": [], "call": []}
    for dims in (2, 3):
        for prec, elem in (("f32", 4), ("f64", 8)):
            row = {"dims": dims, "precision": prec}
            for name, joint in (("scalar", False), ("joint", True)):
                ms = {m: median_ms(lambda: t2.denoise_tv(echoes, sigma, eps=0.0, max_iter=m, dims=dims, precision=prec, out=out,
                                                         joint=joint)) for m in (11, 41)}
                per_iter = (ms[41] - ms[11]) / 30.0
                nbytes = vox * ((2.0 - 1.0 / n_te) * (4 + dims * elem) + dims * elem) if joint else vox * (4 + 2 * dims * elem)
                row[name] = {"ms_per_iteration": per_iter, "bytes_per_iteration": nbytes, "TB_per_s": nbytes / per_iter / 1e9,
                             "ms_11": ms[11], "ms_41": ms[41]}
            row["time_ratio_joint_over_scalar"] = row["joint"]["ms_per_iteration"] / row["scalar"]["ms_per_iteration"]
            row["traffic_ratio_joint_over_scalar"] = row["joint"]["bytes_per_iteration"] / row["scalar"]["bytes_per_iteration"]
            rec["pass"].append(row)
            print(json.dumps(row), flush=True)
    for label, w in (("1sigma", sigma), ("sqrt8sigma", float(np.sqrt(8.0)) * sigma)):
        for name, joint in (("scalar", False), ("joint", True)):
            ms = median_ms(lambda: t2.denoise_tv(echoes, w, out=out, joint=joint))
            n_iter = t2.denoise_tv(echoes, w, out=out, joint=joint, return_info=True)[1]["n_iter"].cpu().numpy()
            row = {"weight": label, "weight_value": w, "kind": name, "call_ms": ms, "problems": int(n_iter.size),
                   "n_iter_min": int(n_iter.min()), "n_iter_mean": float(n_iter.mean()), "n_iter_max": int(n_iter.max())}
            rec["call"].append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
