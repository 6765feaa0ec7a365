"""Measure the dictionary fit (t2map.dictionary.match, t2fit_dict_match_dev) in one run:

    python tools/dict_bench.py --build-t0        # no GPU: the tool-only build with T = 0 (see below)
    python tools/dict_bench.py [--out profiles/r22_dict_bench.json] [--quick]

256^3 x 8 TE (--quick: 32 x 256 x 256 x 8) inside the mask of the synthetic brain volume; 512 and 4096 mono-exponential atoms
(20 .. 2000 ms, log-spaced) and a 64 x 32 two-compartment table.  Raw calls on preallocated buffers, HIP events around each,
the median of 5 after a warm-up:
  match_ms      t2fit_dict_match_dev (the 64-byte header read-back and its wait included)
  match_t0_ms   the same call of a library built with -DT2FIT_DICT_NO_RESCORE_BAND (T = 0: only atoms that tie with the running
                float32 best are re-scored; its results are wrong), in a child process; match_ms - match_t0_ms estimates the
                time the float64 re-scores of the band cost.  Skipped when that library has not been built.
  mfma_bound_ms 2 A nTE voxels / (64 FLOP/clk/SIMD x 4 SIMDs x CUs x clock) for the voxels of the 32-voxel groups that hold a
                masked voxel (what the kernel multiplies), and for the whole volume
  matmul_ms     torch.matmul of the same float32 operands (normalised atoms x the masked voxels, compacted beforehand, in
                chunks whose score matrix is 1 GiB) followed by max over the atoms: float32 scores only, no float64 stage
  lm_f32_ms     t2.fit_volume(solver='lm', precision='f32') of the same volume, the whole call
and, on the CPU, the number of float64 re-scores per voxel that the kernel's rule makes on 1000 masked voxels (the exact
float32 chain of tests/dict_cases.py), against the number a second pass over the final best would make."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

REPEATS = 5
T0_LIB = os.path.join(REPO, "tools", "diag", "lib", "libt2fit_hip_dict_t0.so")
FLOP_PER_CLK_SIMD, SIMDS_PER_CU = 64, 4


def build_t0():
    from fetal_t2mapping_amd import build

    os.makedirs(os.path.dirname(T0_LIB), exist_ok=True)
    cmd = [build.hipcc(), "-O3", "-std=c++17", f"--offload-arch={build.ARCH}", "-shared", "-fPIC", "-fno-gpu-rdc", "-ffp-contract=off",
           "-DT2FIT_DICT_NO_RESCORE_BAND", "-o", T0_LIB, *build.SOURCES]
    print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)


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


def dictionaries(te):
    from fetal_t2mapping_amd import _dict

    return (("mono512", _dict.monoexp(te, _dict.log_grid(20.0, 2000.0, 512))),
            ("mono4096", _dict.monoexp(te, _dict.log_grid(20.0, 2000.0, 4096))),
            ("biexp64x32", _dict.biexp(te, _dict.log_grid(20.0, 2000.0, 64), 2000.0, np.arange(32) / 32)))


def volume(quick):
    import torch

    from fetal_t2mapping_amd import synth

    dev = torch.device("cuda", 0)
    shape, n_te = ((32, 256, 256) if quick else (256, 256, 256)), 8
    echoes, mask, te = synth.brain_volume_torch(shape, n_te, seed=synth.SEED_BASE, device=dev)
    n_vox = int(np.prod(shape))
    return shape, echoes.reshape(n_te, n_vox).contiguous(), (mask.reshape(n_vox) != 0).to(torch.uint8).contiguous(), np.asarray(te, np.float64)


def match_times(quick):
    """{name: ms} of the raw call with the library this process loaded."""
    import torch

    from fetal_t2mapping_amd import _dict
    from fetal_t2mapping_amd._gpu import current_stream
    from fetal_t2mapping_amd._lib import check, load

    lib = load()
    shape, y, mask, te = volume(quick)
    n_vox = y.shape[1]
    index = torch.empty(n_vox, dtype=torch.int32, device=y.device)
    scale = torch.empty(n_vox, dtype=torch.float32, device=y.device)
    rmse = torch.empty(n_vox, dtype=torch.float32, device=y.device)
    out = {}
    for name, d in dictionaries(te):
        packed = torch.from_numpy(_dict.pack(d.atoms)).to(y.device)
        st = current_stream()
        out[name] = median_ms(lambda: check(lib.t2fit_dict_match_dev(y.data_ptr(), 8, n_vox, mask.data_ptr(), packed.data_ptr(),
                                                                      index.data_ptr(), scale.data_ptr(), rmse.data_ptr(), st)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--build-t0", action="store_true", help="build the T = 0 library (no GPU needed) and leave")
    ap.add_argument("--t0-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--clock_ghz", type=float, default=2.4, help="clock of the bound (MI355X peak engine clock)")
    args = ap.parse_args()
    if args.build_t0:
        build_t0()
        return
    if args.t0_child:  # started with T2FIT_LIB pointing at the T = 0 library
        print("T0 " + json.dumps(match_times(args.quick)), flush=True)
        return
    t0 = None
    if os.path.exists(T0_LIB):  # before this process touches the GPU
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--t0-child"] + (["--quick"] if args.quick else []),
                               env=dict(os.environ, T2FIT_LIB=T0_LIB), capture_output=True, text=True, timeout=900)
        lines = [ln for ln in child.stdout.splitlines() if ln.startswith("T0 ")]
        if child.returncode != 0 or not lines:
            raise SystemExit(f"the T = 0 child failed ({child.returncode}):\n{child.stdout}\n{child.stderr}")
        t0 = json.loads(lines[-1][3:])

    import torch

    import dict_cases as K
    import fetal_t2mapping_amd as t2
    from fetal_t2mapping_amd import _dict

    shape, y, mask, te = volume(args.quick)
    n_vox = y.shape[1]
    dev = y.device
    props = torch.cuda.get_device_properties(dev)
    cus = props.multi_processor_count
    ours = match_times(args.quick)
    masked = int(mask.sum())
    groups = int((mask.reshape(-1, 32).max(dim=1).values != 0).sum()) if n_vox % 32 == 0 else None
    idx = torch.nonzero(mask).reshape(-1)
    y_in = y[:, idx].contiguous()
    rec = {"stack": "x".join(map(str, shape)) + "x8", "voxels": n_vox, "masked_voxels": masked, "voxels_in_active_groups": groups * 32,
           "repeats": REPEATS, "statistic": "median", "device": props.name, "compute_units": cus, "clock_ghz_of_the_bound": args.clock_ghz,
           "not_measured": ["hardware counters", "65536 atoms"], "dictionaries": []}
    rng = np.random.default_rng(0)
    sample = y_in[:, torch.from_numpy(rng.choice(masked, size=min(1000, masked), replace=False)).to(dev)].cpu().numpy()
    for name, d in dictionaries(te):
        a_count = d.n_atoms
        flops_per_voxel = 2.0 * a_count * 8
        rate = FLOP_PER_CLK_SIMD * SIMDS_PER_CU * cus * args.clock_ghz * 1e9
        dh, _, dmax = _dict.normalise(d.atoms)
        dh_t = torch.from_numpy(dh).to(dev)
        chunk = max(1, (1 << 30) // (4 * a_count))

        def matmul_max():
            best = torch.empty(masked, dtype=torch.int64, device=dev)
            for lo in range(0, masked, chunk):
                best[lo:lo + chunk] = torch.matmul(dh_t, y_in[:, lo:lo + chunk]).max(dim=0).indices
            return best

        mm = median_ms(matmul_max)
        # agreement of the float32 baseline with the float64 definition, and the re-score counts of the rule, on the sample
        want = _dict.match(sample, d.atoms)[0]
        s32 = K.chain32(dh, sample, 8)
        s64 = _dict.scores(dh, sample)
        band = _dict.band(sample, dmax, 8)
        band32 = band.astype(np.float32)
        band32 = np.where(band32.astype(np.float64) < band, np.nextafter(band32, np.float32(np.inf)), band32)
        got, count = K.candidate_rule(s32, s64, band32, 8)
        second = (s32 >= (s32.max(axis=1) - band32)[:, None]).sum(axis=1)
        row = {"dictionary": name, "atoms": a_count, "match_ms": ours[name], "match_t0_ms": None if t0 is None else t0[name],
               "rescore_band_ms_estimate": None if t0 is None else ours[name] - t0[name],
               "mfma_bound_ms_active_groups": flops_per_voxel * groups * 32 / rate * 1e3,
               "mfma_bound_ms_whole_volume": flops_per_voxel * n_vox / rate * 1e3,
               "fraction_of_bound": flops_per_voxel * groups * 32 / rate * 1e3 / ours[name],
               "matmul_ms": mm, "matmul_chunk_voxels": chunk, "speedup_over_matmul": mm / ours[name],
               "sample_voxels": int(sample.shape[1]), "rule_equals_statement_on_sample": bool(np.array_equal(got, want)),
               "float32_argmax_differs_on_sample": int(np.sum(np.argmax(s32, axis=1) != want)),
               "rescores_per_voxel_mean": float(count.mean()), "rescores_per_voxel_max": int(count.max()),
               "second_pass_rescores_mean": float(second.mean())}
        rec["dictionaries"].append(row)
        print(json.dumps(row), flush=True)
    echoes4 = y.reshape((8,) + shape)
    mask3 = mask.reshape(shape)
    table = t2.fit_table("gaussian", True)
    rec["lm_f32_ms"] = median_ms(lambda: t2.fit_volume(echoes4, mask3, te, "gaussian", table, solver="lm", precision="f32"), repeats=3)
    print(json.dumps({"lm_f32_ms": rec["lm_f32_ms"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
