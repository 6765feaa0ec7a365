"""Measure the chi^2 rule of the T2-spectrum fit (t2fit_nnls_chi2_dev) beside the fixed-weight fit (t2fit_nnls_dev) in one run:

    python tools/nnls_chi2_bench.py [--out profiles/r27_nnls_chi2_bench.json] [--quick]
                                    [--fixed_parent FILE --fixed_this FILE]

256^3 x 8 TE (--quick: 32 x 256 x 256 x 8) inside the mask of the synthetic brain volume, 40 log-spaced T2 from 10 to 2000 ms.
Raw calls on preallocated buffers, HIP events around each, the median of 5 after a warm-up.  Every step below is a fresh child
process under its own time limit; the first that fails ends the run.
  step `volume_order`: t2fit_nnls_dev at mu = 0.03 and at mu = 0 and t2fit_nnls_chi2_dev at factor 1.02, each without the
      spectrum output; per call ms, the outer steps summed over the fitted voxels and ns per outer step (ms / steps: the whole
      device's time per step, not a wave's); for the rule the distributions of solves, nit, rule and the chosen mu, and the
      ratio of its time per outer step to the fixed-weight kernel's at 0.03 and at 0
  step `random_order`: the same three calls on the same voxels in a random order (one permutation of all voxels, mask
      included): every chunk then holds the volume's mix of masked and cheap and dear voxels, so the difference to
      `volume_order` is what the tail and the spread of the cost per voxel cost
--fixed_parent / --fixed_this: two outputs of tools/nnls_bench.py, of the parent commit and of this one in the same session; their
rows for t2fit_nnls_dev are copied in side by side (`unchanged_path`)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

REPEATS = 5
N_BASIS = 40
FACTOR = 1.02
STEPS = (("volume_order", 420), ("random_order", 420))  # (name, seconds it may take)
NOT_MEASURED = ["hardware counters (LDS bank conflicts, VALU busy, scalar-register spill traffic)", "warm starts between a voxel's solves",
                "other chunk sizes (T2FIT_NNLS_CHUNK is unchanged)", "32 echoes x 64 T2 under the rule",
                "a volume whose signal-to-noise ratio varies by an order of magnitude"]


def timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def median_ms(fn, repeats=REPEATS):
    fn()  # warm-up
    times = [timed(fn) for _ in range(repeats)]
    return float(np.median(times)), [float(t) for t in times]


def volume(shape, n_te, shuffle):
    import torch

    from fetal_t2mapping_amd import synth

    dev = torch.device("cuda", 0)
    echoes, mask, te = synth.brain_volume_torch(shape, n_te, seed=synth.SEED_BASE, device=dev)
    n_vox = int(np.prod(shape))
    y, m = echoes.reshape(n_te, n_vox), (mask.reshape(n_vox) != 0).to(torch.uint8)
    if shuffle:
        perm = torch.randperm(n_vox, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
        y, m = y[:, perm], m[perm]
    return y.contiguous(), m.contiguous(), np.asarray(te, np.float64)


def quantiles(t):
    q = np.quantile(t.double().cpu().numpy(), [0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0])
    return dict(zip(("min", "p05", "p25", "median", "p75", "p95", "max"), (float(v) for v in q)))


def step(shape, shuffle):
    import torch

    from fetal_t2mapping_amd import _abi, _gpu_nnls
    from fetal_t2mapping_amd._gpu import current_stream
    from fetal_t2mapping_amd._lib import check, load

    lib = load()
    y, mask, te = volume(shape, 8, shuffle)
    n_te, n_vox = y.shape
    dev = y.device
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    p, c = _gpu_nnls.params(), _gpu_nnls.chi2_params(factor=FACTOR)
    st = current_stream()
    rec = {"voxels": n_vox, "masked_voxels": int(mask.sum()), "n_te": n_te, "n_basis": N_BASIS, "order": "random" if shuffle else "volume"}
    for name, mu in (("fixed_0.03", _gpu_nnls.DEFAULT_MU), ("fixed_0", 0.0), ("chi2", None)):
        b = _gpu_nnls.spectrum_basis(te, _gpu_nnls.log_grid(10.0, 2000.0, N_BASIS), 0.0 if mu is None else mu, {"csf": (600.0, 2000.0)})
        packed = torch.from_numpy(_gpu_nnls.pack(b)).to(dev)
        func, amp, rmse, nit, status = f32(b.n_func, n_vox), f32(n_vox), f32(n_vox), i32(n_vox), i32(n_vox)
        common = (y.data_ptr(), n_te, n_vox, mask.data_ptr(), packed.data_ptr(), None, func.data_ptr(), amp.data_ptr(), rmse.data_ptr(),
                  nit.data_ptr(), status.data_ptr())
        if mu is None:
            wmu, ratio, solves, rule = f32(n_vox), f32(n_vox), i32(n_vox), i32(n_vox)
            call = lambda: check(lib.t2fit_nnls_chi2_dev(C.byref(p), C.byref(c), *common, wmu.data_ptr(), ratio.data_ptr(), solves.data_ptr(),
                                                         rule.data_ptr(), st))
        else:
            call = lambda: check(lib.t2fit_nnls_dev(C.byref(p), *common, st))
        ms, times = median_ms(call)
        fitted = (mask != 0) & (status != _abi.NNLS_NONFINITE)
        steps = int(nit[fitted].sum(dtype=torch.int64))
        row = {"ms": ms, "ms_of_the_repeats": times, "fitted_voxels": int(fitted.sum()), "not_ok": int((status[fitted] != _abi.NNLS_OK).sum()),
               "outer_steps": steps, "outer_steps_per_voxel": steps / max(int(fitted.sum()), 1), "ns_per_outer_step": ms * 1e6 / max(steps, 1)}
        if mu is None:
            found = fitted & (rule == _abi.NNLS_RULE_FOUND)
            row.update(factor=FACTOR, solves=quantiles(solves[fitted]), nit=quantiles(nit[fitted]), mu=quantiles(wmu[fitted]),
                       rule_counts={k: int((rule[fitted] == getattr(_abi, "NNLS_RULE_" + k)).sum()) for k in ("FOUND", "EXACT", "LOW", "HIGH")},
                       mean_solves=float(solves[fitted].double().mean()), ratio_of_the_found=quantiles(ratio[found]) if bool(found.any()) else None)
        rec[name] = row
        print(json.dumps({name: row}), flush=True)
    for name in ("fixed_0.03", "fixed_0"):
        rec["chi2"]["ns_per_outer_step_over_" + name] = rec["chi2"]["ns_per_outer_step"] / rec[name]["ns_per_outer_step"]
    rec["chi2"]["ms_over_fixed_0.03"] = rec["chi2"]["ms"] / rec["fixed_0.03"]["ms"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--step", choices=[s for s, _ in STEPS], help="run this step in this process and print its record (what the tool starts itself)")
    ap.add_argument("--fixed_parent", help="tools/nnls_bench.py's output on the parent commit")
    ap.add_argument("--fixed_this", help="tools/nnls_bench.py's output on this commit, same session")
    args = ap.parse_args()
    shape = (32, 256, 256) if args.quick else (256, 256, 256)
    if args.step:
        print("RECORD " + json.dumps(step(shape, args.step == "random_order")), flush=True)
        return

    rec = {"stack": "x".join(map(str, shape)) + "x8", "repeats": REPEATS, "statistic": "median", "not_measured": NOT_MEASURED}
    for name, limit in STEPS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name] + (["--quick"] if args.quick else [])
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(done.stdout)
        if done.returncode != 0:
            sys.exit(f"step {name} ended with status {done.returncode}: nothing more is started")
        rec[name] = json.loads([line for line in done.stdout.splitlines() if line.startswith("RECORD ")][-1][len("RECORD "):])
    a, b = rec["volume_order"], rec["random_order"]
    rec["volume_order_over_random_order_ms"] = {k: a[k]["ms"] / b[k]["ms"] for k in ("fixed_0.03", "fixed_0", "chi2")}
    if args.fixed_parent and args.fixed_this:
        keep = ("n_te", "n_basis", "mu", "stack", "nnls_ms", "nnls_x_ms", "mean_nit", "ns_per_serial_step")
        rows = lambda path: [{k: r[k] for k in keep if k in r} for r in json.load(open(path))["runs"]]
        rec["unchanged_path"] = {"what": "tools/nnls_bench.py's rows for t2fit_nnls_dev, parent commit and this one, same session",
                                 "parent": rows(args.fixed_parent), "this": rows(args.fixed_this)}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
