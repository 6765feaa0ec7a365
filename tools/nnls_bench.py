"""Measure the T2-spectrum fit (t2map.spectrum.solve, t2fit_nnls_dev) in one run:

    python tools/nnls_bench.py [--out profiles/r26_nnls_bench.json] [--quick]

256^3 x 8 TE (--quick: 32 x 256 x 256 x 8) inside the mask of the synthetic brain volume, 40 log-spaced T2 from 10 to 2000 ms, at
mu = 0, 0.03 (the default) and 0.1; and 32 x 256 x 256 x 32 TE with 64 basis functions at the default mu.  Raw calls on
preallocated buffers, HIP events around each, the median of 5 after a warm-up:
  nnls_ms          t2fit_nnls_dev without the spectrum output (the 64-byte header read-back and its wait included)
  nnls_x_ms        the same call with the spectrum written (n_basis planes)
  mean_nit, mean_passive, max_passive, not_ok   from one further call: outer steps, the coefficients above 0 at the end, voxels
                   whose status is not 0
  wave_us_per_voxel   nnls_ms x the waves the grid keeps resident / fitted voxels: what one wave spends on one voxel
  serial_steps_per_voxel, ns_per_serial_step   every outer step runs one row of the factor and two substitutions, each a chain of
                   about `passive` dependent steps (a lane read, an IEEE float64 division, a multiply, a subtraction); with the
                   mean final passive size standing in for the size along the way this is 3 x mean_nit x mean_passive steps
beside, on the same 8-echo volume: t2fit_dict_match_dev at 512 atoms, t2.fit_volume(solver='lm', precision='f32'), and
scipy.optimize.nnls on the augmented system for 200 masked voxels on the host (one thread)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

REPEATS = 5


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
    return float(np.median([timed(fn) for _ in range(repeats)]))


def volume(shape, n_te):
    import torch

    from fetal_t2mapping_amd import synth

    dev = torch.device("cuda", 0)
    echoes, mask, te = synth.brain_volume_torch(shape, n_te, seed=synth.SEED_BASE, device=dev)
    n_vox = int(np.prod(shape))
    return echoes.reshape(n_te, n_vox).contiguous(), (mask.reshape(n_vox) != 0).to(torch.uint8).contiguous(), np.asarray(te, np.float64)


def run(y, mask, te, n_basis, mu, cus):
    import torch

    from fetal_t2mapping_amd import _abi, _gpu_nnls
    from fetal_t2mapping_amd._gpu import current_stream
    from fetal_t2mapping_amd._lib import check, load

    lib = load()
    n_te, n_vox = y.shape
    dev = y.device
    b = _gpu_nnls.spectrum_basis(te, _gpu_nnls.log_grid(10.0, 2000.0, n_basis), mu, {"csf": (600.0, 2000.0)})
    packed = torch.from_numpy(_gpu_nnls.pack(b)).to(dev)
    x = torch.empty((n_basis, n_vox), dtype=torch.float32, device=dev)
    func = torch.empty((b.n_func, n_vox), dtype=torch.float32, device=dev)
    amp, rmse = (torch.empty(n_vox, dtype=torch.float32, device=dev) for _ in range(2))
    nit, status = (torch.empty(n_vox, dtype=torch.int32, device=dev) for _ in range(2))
    p = _gpu_nnls.params()
    st = current_stream()
    call = lambda xp: check(lib.t2fit_nnls_dev(C.byref(p), y.data_ptr(), n_te, n_vox, mask.data_ptr(), packed.data_ptr(), xp, func.data_ptr(),
                                               amp.data_ptr(), rmse.data_ptr(), nit.data_ptr(), status.data_ptr(), st))
    ms = median_ms(lambda: call(None))
    ms_x = median_ms(lambda: call(x.data_ptr()))
    fitted = status == _abi.NNLS_OK
    n_fit = int(fitted.sum())
    passive = (x > 0).sum(dim=0)[fitted].double()
    mean_nit, mean_p = float(nit[fitted].double().mean()), float(passive.mean())
    waves, lds, per_cu = _gpu_nnls.workgroup(n_basis)  # what the library launches
    resident = cus * waves * per_cu
    steps = 3.0 * mean_nit * mean_p
    return {"n_te": n_te, "n_basis": n_basis, "mu": mu, "voxels": n_vox, "masked_voxels": int(mask.sum()), "fitted_voxels": n_fit,
            "not_ok": int(((status != _abi.NNLS_OK) & (mask != 0)).sum()), "nnls_ms": ms, "nnls_x_ms": ms_x, "mean_nit": mean_nit,
            "max_nit": int(nit.max()), "mean_passive": mean_p, "max_passive": int(passive.max()), "waves_per_workgroup": waves,
            "lds_bytes_per_workgroup": lds, "resident_waves": resident, "wave_us_per_voxel": ms * 1e3 * resident / n_fit,
            "serial_steps_per_voxel": steps, "ns_per_serial_step": ms * 1e6 * resident / n_fit / steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()

    import torch
    from scipy.optimize import nnls

    import fetal_t2mapping_amd as t2
    from fetal_t2mapping_amd import _dict, _gpu_nnls
    from fetal_t2mapping_amd._gpu import current_stream
    from fetal_t2mapping_amd._lib import check, load

    shape = (32, 256, 256) if args.quick else (256, 256, 256)
    y, mask, te = volume(shape, 8)
    dev = y.device
    props = torch.cuda.get_device_properties(dev)
    cus = props.multi_processor_count
    rec = {"stack": "x".join(map(str, shape)) + "x8", "repeats": REPEATS, "statistic": "median", "device": props.name, "compute_units": cus,
           "not_measured": ["hardware counters (LDS bank conflicts, VALU busy)", "lane-per-voxel variant", "other workgroup sizes",
                            "a 256^3 volume with 32 echoes"], "runs": []}
    for mu in (0.0, _gpu_nnls.DEFAULT_MU, 0.1):
        rec["runs"].append(run(y, mask, te, 40, mu, cus))
        print(json.dumps(rec["runs"][-1]), flush=True)

    # beside: the dictionary fit at 512 atoms and the float32 LM fit of the same volume
    lib = load()
    n_vox = y.shape[1]
    d = _dict.monoexp(te, _dict.log_grid(20.0, 2000.0, 512))
    packed = torch.from_numpy(_dict.pack(d.atoms)).to(dev)
    index = torch.empty(n_vox, dtype=torch.int32, device=dev)
    scale, rmse = (torch.empty(n_vox, dtype=torch.float32, device=dev) for _ in range(2))
    st = current_stream()
    rec["dict_512_ms"] = median_ms(lambda: check(lib.t2fit_dict_match_dev(y.data_ptr(), 8, n_vox, mask.data_ptr(), packed.data_ptr(),
                                                                          index.data_ptr(), scale.data_ptr(), rmse.data_ptr(), st)))
    table = t2.fit_table("gaussian", True)
    echoes4, mask3 = y.reshape((8,) + shape), mask.reshape(shape)
    rec["lm_f32_ms"] = median_ms(lambda: t2.fit_volume(echoes4, mask3, te, "gaussian", table, solver="lm", precision="f32"), repeats=3)
    print(json.dumps({"dict_512_ms": rec["dict_512_ms"], "lm_f32_ms": rec["lm_f32_ms"]}), flush=True)

    # beside: scipy on the host, 200 masked voxels
    idx = torch.nonzero(mask).reshape(-1)
    pick = idx[torch.from_numpy(np.random.default_rng(0).choice(idx.numel(), size=200, replace=False)).to(dev)]
    sample = y[:, pick].cpu().numpy().astype(np.float64)
    rec["scipy"] = []
    for mu in (0.0, _gpu_nnls.DEFAULT_MU, 0.1):
        A = _gpu_nnls.monoexp_basis(te, _gpu_nnls.log_grid(10.0, 2000.0, 40))
        aug = np.vstack([A, mu * np.eye(40)])
        t0 = time.perf_counter()
        for v in range(sample.shape[1]):
            nnls(aug, np.concatenate([sample[:, v], np.zeros(40)]))
        per = (time.perf_counter() - t0) / sample.shape[1]
        rec["scipy"].append({"mu": mu, "ms_per_voxel_one_thread": per * 1e3, "ms_for_the_masked_voxels_one_thread": per * 1e3 * int(mask.sum())})
        print(json.dumps(rec["scipy"][-1]), flush=True)
    del y, mask, echoes4, mask3

    # the largest problem on a smaller volume
    y, mask, te = volume((32, 256, 256), 32)
    rec["runs"].append(dict(run(y, mask, te, 64, _gpu_nnls.DEFAULT_MU, cus), stack="32x256x256x32"))
    print(json.dumps(rec["runs"][-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
