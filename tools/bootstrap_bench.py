#!/usr/bin/env python3
"""Times the parametric bootstrap (t2map.bootstrap_volume / t2fit_bootstrap_dev) on the GPU.  One JSON line per
configuration and repetition:

    python tools/bootstrap_bench.py [--sizes 180x256x256x6 256x256x256x8] [--replicas 32] [--warm 5] [--repeat 2]
                                    [--calls 5] [--out profiles/r06_bootstrap_bench.jsonl]

Per replica, from HIP events around the public pieces after --warm discarded replicas: synth_ms (t2fit_boot_synth_dev),
fit_ms (t2fit_volume_dev on the replica, the call as the loop makes it: fit kernel + epilogue) and fit_kernel_ms (the
library's own timing of the fit kernel).  The loop itself is timed by the host clock around t2fit_bootstrap_dev, which
returns when the maps are complete.  Three modes -- interval with two streams (the default a user gets), interval with
one stream (T2FIT_BOOT_STREAMS=1) and moments only -- are called --calls times each, in alternation, after one warm
call per mode; loop_*_ms lists every call's wall time of R replicas, *_min_ms / *_median_ms summarise them and
*_per_replica_ms is the median over R.  Differences of wall times are not reported: the accumulation and finalisation
kernels are too small beside the spread of a call (their times are in the kernel trace,
profiles/r06_bootstrap_kernel_stats.csv).  synth_gbps: the 4 nTE bytes per voxel the synthesis writes over synth_ms.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = (("gaussian_rician", "lbfgsb", "f64"), ("gaussian", "lm", "f32"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["180x256x256x6", "256x256x256x8"], help="Z x Y x X x nTE")
    ap.add_argument("--replicas", type=int, default=32)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5, help="timed calls of each loop mode per repetition, alternating")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bootstrap_bench: no HIP device (timings are taken on the GPU only)")
    import fetal_t2mapping_amd as t2
    from fetal_t2mapping_amd import _abi, synth
    from fetal_t2mapping_amd._lib import check, require_gpu

    lib = require_gpu()
    dev = torch.device("cuda", 0)
    R = args.replicas

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    for size in args.sizes:
        z, y, x, n_te = (int(v) for v in size.split("x"))
        n_vox = z * y * x
        echoes, mask, te = synth.brain_volume_torch((z, y, x), n_te, synth.SEED_BASE, dev)
        for fit, solver, precision in CONFIGS:
            table = t2.fit_table(fit, True)
            cfg = t2.make_config(fit, table, te, True, False, solver, precision)
            base = t2.fit_volume(echoes.reshape(n_te, z, y, x), mask, te, fit, table, solver=solver, precision=precision, extras=True)
            sigma, _ = t2.estimate_background_sigma(echoes.reshape(n_te, z, y, x), mask.reshape(z, y, x))
            block = torch.empty((n_te, n_vox), dtype=torch.float32, device=dev)
            rep = [torch.empty(n_vox, dtype=torch.float32, device=dev) for _ in range(4)]
            status = torch.empty(n_vox, dtype=torch.uint8, device=dev)
            rm = _abi.T2FitMaps()
            rm.t2, rm.k, rm.sigma, rm.res, rm.status = (*(r.data_ptr() for r in rep), status.data_ptr())
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            t2_d, k_d = base.t2.reshape(-1), base.k.reshape(-1)

            def do_synth(r):
                check(lib.t2fit_boot_synth_dev(C.byref(cfg), t2_d.data_ptr(), k_d.data_ptr(), sigma, None, mask.data_ptr(), n_vox,
                                               0, 0, r, 0, block.data_ptr(), st))

            def do_fit():
                check(lib.t2fit_volume_dev(C.byref(cfg), block.data_ptr(), 0, mask.data_ptr(), n_vox, C.byref(rm), st))

            out = _abi.T2FitBootMaps()
            maps = [torch.empty(n_vox, dtype=torch.float32, device=dev) for _ in range(5)]
            n_ok = torch.empty(n_vox, dtype=torch.int32, device=dev)

            def loop(interval, one_stream=False):
                out.mean[0], out.bias[0], out.std[0] = (m.data_ptr() for m in maps[:3])
                out.ci_lo[0], out.ci_hi[0] = (maps[3].data_ptr(), maps[4].data_ptr()) if interval else (None, None)
                out.n_ok = n_ok.data_ptr()
                os.environ["T2FIT_BOOT_STREAMS"] = "1" if one_stream else "2"
                torch.cuda.synchronize()
                t = time.perf_counter()
                check(lib.t2fit_bootstrap_dev(None, C.byref(cfg), t2_d.data_ptr(), k_d.data_ptr(), None, sigma, None, 0,
                                              mask.data_ptr(), n_vox, R, 0, 0.05, 1, C.byref(out), 0, st))
                return (time.perf_counter() - t) * 1e3

            modes = {"two_stream": (True, False), "one_stream": (True, True), "moments_only": (False, False)}
            for repeat in range(args.repeat):
                lib.t2fit_set_timing(1)
                ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.warm + R)]
                kernel_ms = []
                for r in range(args.warm + R):
                    ev[r][0].record()
                    do_synth(r)
                    ev[r][1].record()
                    do_fit()
                    ev[r][2].record()
                    torch.cuda.synchronize()
                    kernel_ms.append(lib.t2fit_kernel_ms(0))
                lib.t2fit_set_timing(0)
                synth_ms = float(np.mean([e[0].elapsed_time(e[1]) for e in ev[args.warm:]]))
                fit_ms = float(np.mean([e[1].elapsed_time(e[2]) for e in ev[args.warm:]]))
                fit_kernel_ms = float(np.mean(kernel_ms[args.warm:]))
                for mode in modes.values():  # warm: code objects, allocator
                    loop(*mode)
                walls = {name: [] for name in modes}
                for _ in range(args.calls):
                    for name, mode in modes.items():
                        walls[name].append(loop(*mode))
                counted = float(n_ok[mask != 0].float().mean())
                rec = {
                    "tool": "bootstrap_bench", "shape": [z, y, x], "n_te": n_te, "n_vox": n_vox, "n_masked": int(mask.sum()),
                    "fit": fit, "solver": solver, "precision": precision, "replicas": R, "warm": args.warm, "repeat": repeat,
                    "calls": args.calls, "noise_sigma": round(sigma, 4), "mean_n_ok": round(counted, 3),
                    "synth_ms": round(synth_ms, 4), "synth_gbps": round(4.0 * n_te * n_vox / (synth_ms * 1e-3) / 1e9, 1),
                    "fit_ms": round(fit_ms, 4), "fit_kernel_ms": round(fit_kernel_ms, 4),
                }
                for name, w in walls.items():
                    rec[f"loop_{name}_ms"] = [round(v, 3) for v in w]
                    rec[f"{name}_min_ms"] = round(min(w), 3)
                    rec[f"{name}_median_ms"] = round(float(np.median(w)), 3)
                    rec[f"{name}_per_replica_ms"] = round(float(np.median(w)) / R, 4)
                rec["replicas_per_s"] = round(R / (float(np.median(walls["two_stream"])) * 1e-3), 2)
                rec["two_stream_per_replica_over_fit_ms"] = round(float(np.median(walls["two_stream"])) / R / fit_ms, 4)
                emit(rec)
            del block, rep, status, maps, n_ok, base
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
