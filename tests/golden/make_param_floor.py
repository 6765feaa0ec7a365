"""How well does the reference agree with ITSELF in k, sigma, the objective and its iterates?  (fixture: tests/golden/param_floor.npz)

tests/golden/noise_floor.npz measures the reference's self-agreement in T2 and the iteration count and defines the
STABLE set of every fixture.  This script measures the other outputs on those rows, with the same 24 seeds
(12345 + 1000 j) and the same one-ulp perturbation of exp / log / i0e (oracle/noise_model.py; the rician objective's float32
``np.log(signal)`` moved by one FLOAT32 ulp, perturbed_objectives(f32_log_ulp=True)): per fixture, per stable
row and per seed the deviation from the golden row of

    k        relative                                   <name>/k_rel      (24, n_stable) float32, 8 mantissa bits kept
    sigma    relative, 3-parameter models               <name>/sigma_rel  (24, n_stable) float32, 8 mantissa bits kept
    fun      oracle.noise_model.fun_deviation           <name>/fun_dev    (24, n_stable) float32, 8 mantissa bits kept
    T2       absolute, ms (maximum over the seeds)      <name>/t2_abs_max (n_stable,)

and the maxima over the seeds (<key>_max), the rows (<name>/rows) and which of them some seed takes out of the stable
rule today (<name>/left_stable: T2 beyond 1e-3 ms, another nit or another success flag).  noise_floor.npz is read, never
written: its stable sets are fixed data.

The same for the frozen stack (frozen/<name>/...): the rows tests hold the numpy_legacy lane solver to
(frozen_voxels_<name>.npz `stable`, for the least-squares models intersected with the default stable set), deviations
from the FROZEN fixture's row.  The rician objective is perturbed in its float32-promotion form
(perturbed_objectives(numpy_legacy=True)) and stored per seed.  For the two least-squares models numpy_legacy changes
nothing in the objective, so their perturbed fits ARE the default stack's (same seed, same rows): only the rows and
the per-row maxima against the frozen row are stored, and tests take the default stack's per-seed arrays at those rows
as the yardstick (storing them twice would take the file past the size limit of a committed file).

Traces: the traced rows of a fixture (trace_first_row ..) that are stable are fitted again under every seed with the
reference's callback (oracle.noise_model.perturbed_traced_fit); per row and iteration the maximum over the seeds of the
deviation of f_val (fun_deviation) and of the step length (relative) from the golden trace over the common length
(<name>/trace_rows, <name>/trace_f_dev, <name>/trace_step_dev: (n_rows, 64), NaN beyond the trace), and the share of
(row, seed) pairs whose trace length differs (trace_len_differs_share).

    OPENBLAS_NUM_THREADS=1 python -B tests/golden/make_param_floor.py
"""
import glob
import os
import sys
import time

os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402
import scipy  # noqa: E402
from scipy.optimize import minimize  # noqa: E402

from oracle import t2fit_oracle as O  # noqa: E402
from oracle.noise_model import (deviation_stats, fun_deviation, perturbed_objectives, perturbed_traced_fit,  # noqa: E402
                                rel_deviation, trace_deviation)

K_SEEDS = 24
SEEDS = [12345 + 1000 * j for j in range(K_SEEDS)]  # make_noise_floor.py's
TRACE_LEN = 64


def _stable_rows(name):
    return np.flatnonzero(np.load(os.path.join(HERE, "noise_floor.npz"))[name + "/stable"])


def _frozen_rows(name, mode):
    fz = np.load(os.path.join(HERE, f"frozen_voxels_{name}.npz"))
    nf = np.load(os.path.join(HERE, "noise_floor.npz"))
    return np.flatnonzero(fz["stable"] & (nf[name + "/stable"] if mode != "rician" else True))


def one_run(args):
    """(path, seed, legacy): the reference's fit of the stable rows of one fixture with every exp / log / i0e moved by at most
    one ulp -> (x, nit, success, fun) per row.  ``legacy``: the frozen stack's rows and its rician objective."""
    path, seed, legacy = args
    d = np.load(path)
    name = os.path.basename(path)[7:-4]
    mode, lf, prior = str(d["mode"]), bool(d["low_field"]), bool(d["prior"])
    rows = _frozen_rows(name, mode) if legacy else _stable_rows(name)
    rng = np.random.default_rng(seed)
    fun = None if legacy else perturbed_objectives(rng)[mode]
    x = np.zeros((len(rows), d["x"].shape[1]))
    nit, ok, f = np.zeros(len(rows), np.int32), np.zeros(len(rows), bool), np.zeros(len(rows))
    for i, v in enumerate(rows):
        fp = O.fit_table(mode, lf)
        lb, ub = O.voxel_bounds(fp, d["y"][v, 0], prior)
        if legacy:
            fun = perturbed_objectives(rng, True, d["y"][v])[mode]
        elif mode == "rician":  # np.log of the float32 samples is a float32 function: one FLOAT32 ulp, once per voxel
            fun = perturbed_objectives(rng, False, d["y"][v], f32_log_ulp=True)[mode]
        with np.errstate(all="ignore"):
            r = minimize(fun, fp["initial_guess"], args=(d["te"], np.array(d["y"][v])), method="L-BFGS-B",
                         bounds=list(zip(lb, ub)), options=fp["options"], jac=False)
        x[i], nit[i], ok[i], f[i] = r.x, r.nit, r.success, r.fun
    return x, nit, ok, f


def trace_run(args):
    """(path, seed): the stable traced rows of one fixture with the reference's callback under one perturbation seed
    -> list of (trace_f, trace_step) per row."""
    path, seed = args
    d = np.load(path)
    name = os.path.basename(path)[7:-4]
    mode, lf, prior = str(d["mode"]), bool(d["low_field"]), bool(d["prior"])
    rng = np.random.default_rng(seed)
    fun = perturbed_objectives(rng)[mode]
    first = int(d["trace_first_row"])
    stable = np.load(os.path.join(HERE, "noise_floor.npz"))[name + "/stable"]
    out = []
    for v in range(first, first + d["trace_f"].shape[0]):
        if stable[v]:
            if mode == "rician":
                fun = perturbed_objectives(rng, False, d["y"][v], f32_log_ulp=True)[mode]
            out.append(perturbed_traced_fit(fun, mode, lf, prior, d["te"], d["y"][v])[4:])
    return out


def _f32(a):
    """float32 with 8 explicit mantissa bits (rounded to nearest: 0.2 % relative, against a margin of 20 %): the low 15 bits
    of every number are zero, which is what lets the 24 x n arrays compress to within the size limit of a committed file."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return ((u + np.uint32(0x4000)) & np.uint32(0xFFFF8000)).view(np.float32)


def _deviations(out, key, runs, rows, gx, gf, gnit, gok, y, per_seed=True):
    n_par = gx.shape[1]
    k_rel = np.array([rel_deviation(x[:, 0], gx[:, 0]) for x, _, _, _ in runs])
    t2_abs = np.array([np.abs(x[:, 1] - gx[:, 1]) for x, _, _, _ in runs])
    f_dev = np.array([fun_deviation(f, gf, y) for _, _, _, f in runs])
    left = np.zeros(len(rows), bool)
    for x, nit, ok, _ in runs:
        left |= ~((np.abs(x[:, 1] - gx[:, 1]) <= 1e-3) & (nit == gnit) & (ok == gok))
    out[key + "/rows"] = rows.astype(np.int32)
    if per_seed:
        out[key + "/k_rel"] = _f32(k_rel)
        out[key + "/fun_dev"] = _f32(f_dev)
    out[key + "/k_rel_max"] = k_rel.max(axis=0).astype(np.float32)
    out[key + "/fun_dev_max"] = f_dev.max(axis=0).astype(np.float32)
    out[key + "/t2_abs_max"] = t2_abs.max(axis=0).astype(np.float32)
    out[key + "/left_stable"] = left
    if n_par == 3:
        s_rel = np.array([rel_deviation(x[:, 2], gx[:, 2]) for x, _, _, _ in runs])
        if per_seed:
            out[key + "/sigma_rel"] = _f32(s_rel)
        out[key + "/sigma_rel_max"] = s_rel.max(axis=0).astype(np.float32)


def main():
    import multiprocessing as mp

    t0 = time.time()
    paths = sorted(glob.glob(os.path.join(HERE, "voxels_*.npz")))
    meta = [(os.path.basename(p)[7:-4], str(np.load(p)["mode"])) for p in paths]
    tasks = [(p, sd, False) for p in paths for sd in SEEDS]
    legacy_paths = [p for p, (_, mode) in zip(paths, meta) if mode == "rician"]
    tasks += [(p, sd, True) for p in legacy_paths for sd in SEEDS]
    with mp.get_context("fork").Pool(min(8, os.cpu_count() or 1)) as pool:
        runs = pool.map(one_run, tasks, chunksize=1)
        traces = pool.map(trace_run, [(p, sd) for p in paths for sd in SEEDS], chunksize=1)
    by_task = {(t[0], t[1], t[2]): r for t, r in zip(tasks, runs)}
    out = {}
    pooled = {}
    n_len = n_pairs = 0
    for pi, (path, (name, mode)) in enumerate(zip(paths, meta)):
        d = np.load(path)
        rows = _stable_rows(name)
        mine = [by_task[(path, sd, False)] for sd in SEEDS]
        _deviations(out, name, mine, rows, d["x"][rows], d["fun"][rows], d["nit"][rows], d["success"][rows], d["y"][rows])
        # frozen stack: deviations from the frozen fixture's row on the rows its test uses
        fz = np.load(os.path.join(HERE, f"frozen_voxels_{name}.npz"))
        frows = _frozen_rows(name, mode)
        if mode == "rician":
            fmine = [by_task[(path, sd, True)] for sd in SEEDS]
        else:  # the same perturbed fits (numpy_legacy leaves these objectives alone), the frozen rows among them
            at = np.searchsorted(rows, frows)
            assert np.array_equal(rows[at], frows)
            fmine = [tuple(a[at] for a in r) for r in mine]
        _deviations(out, "frozen/" + name, fmine, frows, fz["x"][frows], fz["fun"][frows], fz["nit"][frows],
                    fz["success"][frows], d["y"][frows], per_seed=mode == "rician")
        # traces
        first = int(d["trace_first_row"])
        trows = np.array([v for v in range(first, first + d["trace_f"].shape[0]) if v in set(rows.tolist())], np.int32)
        tf = np.full((len(trows), TRACE_LEN), np.nan)
        ts = np.full((len(trows), TRACE_LEN), np.nan)
        for j in range(K_SEEDS):
            for i, (got_f, got_s) in enumerate(traces[pi * K_SEEDS + j]):
                want_f = d["trace_f"][trows[i] - first]
                want_f = want_f[np.isfinite(want_f)]
                want_s = d["trace_step"][trows[i] - first][: len(want_f)]
                n_pairs += 1
                n_len += int(len(got_f) != len(want_f))
                df, ds = trace_deviation(got_f, got_s, want_f, want_s, d["y"][trows[i]])
                tf[i, : len(df)] = np.fmax(tf[i, : len(df)], df)
                ts[i, 1: 1 + len(ds)] = np.fmax(ts[i, 1: 1 + len(ds)], ds)
        out[name + "/trace_rows"] = trows
        out[name + "/trace_f_dev"] = tf.astype(np.float32)
        out[name + "/trace_step_dev"] = ts.astype(np.float32)
        for stack, key in (("default", name), ("frozen", "frozen/" + name)):
            p = pooled.setdefault((stack, mode), {"k": [], "sigma": [], "fun": [], "t2": [], "left": [], "tf": [], "ts": []})
            p["k"].append(out[key + "/k_rel" + ("" if key + "/k_rel" in out else "_max")].ravel())
            p["fun"].append(out[key + "/fun_dev" + ("" if key + "/fun_dev" in out else "_max")].ravel())
            p["t2"].append(out[key + "/t2_abs_max"])
            p["left"].append(out[key + "/left_stable"])
            if key + "/sigma_rel_max" in out:
                p["sigma"].append(out[key + "/sigma_rel" + ("" if key + "/sigma_rel" in out else "_max")].ravel())
            if stack == "default":
                p["tf"].append(tf.ravel())
                p["ts"].append(ts.ravel())
    out["trace_len_differs_share"] = np.float64(n_len / max(n_pairs, 1))
    out["trace_pairs"] = np.int64(n_pairs)
    out["k_seeds"] = np.int64(K_SEEDS)
    out["numpy_version"] = np.array(np.__version__)
    out["scipy_version"] = np.array(scipy.__version__)
    for (stack, mode), p in pooled.items():
        left = np.concatenate(p["left"])
        print(f"{stack:7s} {mode:16s} stable rows {len(left):4d}  some seed leaves the 1e-3 ms stable rule today: {left.mean():.4f}  "
              f"T2 abs max {np.concatenate(p['t2']).max():.3g} ms")
        for what in ("k", "sigma", "fun", "tf", "ts"):
            if p[what]:
                q = (50, 90, 100) if what in ("tf", "ts") else (50, 99, 100)
                print(f"    {what:5s} p{q[0]} / p{q[1]} / max: " + " / ".join(f"{v:.3g}" for v in deviation_stats(np.concatenate(p[what]), q)))
    print(f"trace length differs on {n_len} of {n_pairs} (row, seed) pairs")
    np.savez_compressed(os.path.join(HERE, "param_floor.npz"), **out)
    print(f"param_floor.npz: {os.path.getsize(os.path.join(HERE, 'param_floor.npz'))} bytes, {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
