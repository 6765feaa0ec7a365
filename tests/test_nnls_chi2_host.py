"""The chi^2 rule of the T2-spectrum fit without a GPU: the statement (fetal_t2mapping_amd/_nnls.py: solve_voxel_chi2,
solve_chi2, misfit) against the rule written a second time in plain Python floats, the bracket it must end with, the
monotone misfit it relies on, every rule code, the degenerate parameter sets, the aggregation of nit and status, the
ordering of the chosen weight with the noise, every refusal of the C entry points that needs no device, the CLI flags
and refusals, and -- recorded, not bounded -- the geometric-mean T2 error on the phantom of tools/nnls_mu_sweep.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import nnls_chi2_cases as Q
import nnls_cases as K
from fetal_t2mapping_amd import _abi, _nnls as N


@pytest.fixture(scope="module")
def lib():
    from fetal_t2mapping_amd import build
    from fetal_t2mapping_amd._lib import load

    build.build()
    return load()


def _run(y, b, mu, **kw):
    """One solve at weight `mu` and its misfit in Python floats: ``(ss, x, P, nit, status)``."""
    x, P, nit, status = N.solve_voxel(y, b.with_mu(mu), **kw)
    r = [float(v) for v in np.asarray(y, np.float32)]
    for k in P:
        r = [ri - float(b.A[i, k]) * float(x[k]) for i, ri in enumerate(r)]
    ss = 0.0
    for ri in r:
        ss = ss + ri * ri
    return ss, x, P, nit, status


def _rule_again(y, b, factor=1.02, mu_first=1e-3, grow=4.0, n_grow=6, n_bisect=5, exact_rel=1e-12, mu_exact=0.03, **kw):
    """The rule of include/t2fit.h once more, in Python floats: ``(x, P, nit, status, mu, ratio, solves, rule)``."""
    runs = [_run(y, b, 0.0, **kw)]
    ss0 = runs[0][0]
    yy = 0.0
    for v in np.asarray(y, np.float32):
        yy = yy + float(v) * float(v)
    if not ss0 > exact_rel * yy:
        runs.append(_run(y, b, mu_exact, **kw))
        rule, mu = N.RULE_EXACT, mu_exact
    else:
        target, lo, mu, g, rule = factor * ss0, 0.0, mu_first, 0, N.RULE_HIGH
        while True:
            runs.append(_run(y, b, mu, **kw))
            if runs[-1][0] >= target:
                rule = N.RULE_LOW if g == 0 else N.RULE_FOUND
                break
            lo = mu
            if g == n_grow:
                break
            g, mu = g + 1, mu * grow
        if rule == N.RULE_FOUND:
            hi = mu
            for _ in range(n_bisect):
                mid = math.sqrt(lo * hi)
                runs.append(_run(y, b, mid, **kw))
                lo, hi = (mid, hi) if runs[-1][0] < target else (lo, mid)
            mu = math.sqrt(lo * hi)
            runs.append(_run(y, b, mu, **kw))
    ss, x, P = runs[-1][:3]
    return x, P, sum(r[3] for r in runs), max(r[4] for r in runs), mu, 0.0 if rule == N.RULE_EXACT else ss / ss0, len(runs), rule


@pytest.mark.parametrize("n_te,n_basis,kind,params,max_iter", [
    (8, 40, "noisy", "default", 0), (8, 40, "noisier", "other", 0), (8, 40, "noisy", "low", 0), (8, 40, "noisy", "high", 0),
    (8, 40, "noisy", "no_bisect", 0), (8, 40, "noisy", "no_grow", 0), (8, 40, "exact", "default", 0), (3, 17, "noisy", "default", 0),
    (8, 40, "noisy", "default", 12), (31, 63, "noisy", "default", 0)])
def test_the_rule_written_again_in_python_floats(n_te, n_basis, kind, params, max_iter):
    y, ref, _ = Q.reference(n_te, n_basis, kind, 12, seed=5, params=params, max_iter=max_iter)
    b = K.basis(n_te, n_basis, 0.0)
    for v in range(y.shape[1]):
        got = N.solve_voxel_chi2(y[:, v], b, max_iter=max_iter, **Q.PARAMS[params][0])
        want = _rule_again(y[:, v], b, max_iter=max_iter, **Q.PARAMS[params][0])
        assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2:] == want[2:], (v, got[2:], want[2:])
        x, P, nit, status, mu, ratio, solves, rule = got
        func, amp, rmse = N.outputs_voxel(y[:, v], b, x, P)
        assert rmse == np.float32(math.sqrt(N.misfit(y[:, v], b, x, P) / n_te))  # misfit is the RMSE's sum
        for k, value in (("x", x.astype(np.float32)), ("func", func), ("amp", amp), ("rmse", rmse), ("nit", nit), ("status", status),
                         ("mu", np.float32(mu)), ("ratio", np.float32(ratio)), ("solves", solves), ("rule", rule)):
            assert np.array_equal(ref[k][..., v], value), (v, k)
    assert ref["mu"].dtype == ref["ratio"].dtype == np.float32 and ref["solves"].dtype == ref["rule"].dtype == np.int32


def test_found_voxels_end_with_a_bracket_of_the_target():
    """With [lo, hi] as the bisection leaves them: ss(lo) < target <= ss(hi), lo <= mu <= hi, hi / lo <= grow^(2^-n_bisect)."""
    for params in ("default", "no_bisect", "other"):
        kw = {**N.CHI2_DEFAULTS, **Q.PARAMS[params][0]}
        kind = "noisier" if params == "other" else "noisy"
        y, ref, stats = Q.reference(8, 40, kind, 12, seed=5, params=params)
        b = K.basis(8, 40, 0.0)
        found = np.flatnonzero(ref["rule"] == N.RULE_FOUND)
        assert found.size >= 8
        for v in found:
            st = stats[v]
            mu = math.sqrt(st["lo"] * st["hi"])
            assert _run(y[:, v], b, st["lo"])[0] < st["target"] <= _run(y[:, v], b, st["hi"])[0]
            assert st["lo"] <= mu <= st["hi"] and np.float32(mu) == ref["mu"][v] and st["target"] == kw["factor"] * st["ss0"]
            assert st["hi"] / st["lo"] <= kw["grow"] ** (2.0 ** -kw["n_bisect"]) * (1 + 1e-12)
            assert len(st["trace"]) == ref["solves"][v] and st["trace"][0][0] == 0.0 and st["trace"][-1][0] == mu


def test_the_misfit_does_not_decrease_with_the_weight():
    weights = [0.0] + [1e-4 * 2.0 ** k for k in range(16)]
    for n_te, n_basis, seed in ((8, 40, 5), (32, 64, 6), (3, 17, 7)):
        b = K.basis(n_te, n_basis, 0.0)
        y = K.decays(n_te, 6, seed)
        for v in range(y.shape[1]):
            ss = [_run(y[:, v], b, mu)[0] for mu in weights]
            assert all(later >= earlier for earlier, later in zip(ss, ss[1:])), (n_te, n_basis, v, ss)


def test_every_rule_code_is_reached():
    count = lambda ref, rule: int((ref["rule"] == rule).sum())
    # three echoes, 17 columns: the unregularised fit is exact to rounding wherever the noisy decay lies in the columns' cone
    _, ref, _ = Q.reference(3, 17, "noisy", 12, seed=5)
    exact = ref["rule"] == N.RULE_EXACT
    assert exact.sum() >= 6 and np.all(ref["mu"][exact] == np.float32(0.03)) and not ref["ratio"][exact].any() and np.all(ref["solves"][exact] == 2)
    assert np.all(ref["ratio"][~exact] >= 1)
    # decays built from two columns.  Not every one is judged exact: at weight 0 the normal equations are ill-conditioned and
    # the solve may stop short of the exact fit (tests/nnls_cases.py: MEASURED_RESIDUAL_GAP_MU0)
    y, ref, _ = Q.reference(8, 40, "exact", 12, seed=5)
    exact = ref["rule"] == N.RULE_EXACT
    assert exact.sum() >= 6 and np.all(ref["amp"] > 0)
    want = N.solve(y, K.basis(8, 40, 0.03))  # the result is the fallback weight's
    assert all(ref[k][..., exact].tobytes() == want[k][..., exact].tobytes() for k in ("x", "func", "amp", "rmse"))
    _, ref, _ = Q.reference(8, 40, "noisy", 12, seed=5, params="low")
    assert count(ref, N.RULE_LOW) == 12 and np.all(ref["mu"] == np.float32(0.5)) and np.all(ref["solves"] == 2) and np.all(ref["ratio"] >= 1.02)
    _, ref, _ = Q.reference(8, 40, "noisy", 12, seed=5, params="high")
    assert count(ref, N.RULE_HIGH) == 12 and np.all(ref["mu"] == np.float32(4e-6)) and np.all(ref["solves"] == 3) and np.all(ref["ratio"] < 1.02)
    _, ref, _ = Q.reference(8, 40, "noisy", 12, seed=5)
    assert count(ref, N.RULE_FOUND) >= 10 and count(ref, N.RULE_FOUND) + count(ref, N.RULE_LOW) == 12
    found = ref["rule"] == N.RULE_FOUND
    assert np.all(ref["ratio"][found] >= 1) and np.all(ref["solves"][found] == np.log(ref["mu"][found] / 1e-3) // np.log(4.0) + 1 + 8)
    print("misfit ratios of the FOUND voxels:", np.sort(ref["ratio"][found]))


def test_no_bisection_and_no_growth():
    _, ref, stats = Q.reference(8, 40, "noisy", 12, seed=5, params="no_bisect")
    _, full, _ = Q.reference(8, 40, "noisy", 12, seed=5)
    found = ref["rule"] == N.RULE_FOUND
    assert np.array_equal(ref["rule"], full["rule"]) and np.array_equal(ref["solves"][found], full["solves"][found] - 5)
    for v in np.flatnonzero(found):  # the weight is the geometric middle of two steps of the bracket
        lo = [1e-3 * 4.0 ** k for k in range(7)]
        assert any(np.float32(math.sqrt(a * a * 4.0)) == ref["mu"][v] for a in lo)
    _, ref, _ = Q.reference(8, 40, "noisy", 12, seed=5, params="no_grow")  # one weight: above the target (LOW) or not (HIGH)
    assert set(ref["rule"].tolist()) <= {N.RULE_LOW, N.RULE_HIGH} and np.all(ref["mu"] == np.float32(1e-3)) and np.all(ref["solves"] == 2)
    assert (ref["rule"] == N.RULE_HIGH).sum() >= 10


def test_nit_is_summed_and_the_status_is_the_largest():
    """A step limit of 12: some solves of a voxel reach it and others do not."""
    y, ref, stats = Q.reference(8, 40, "noisy", 12, seed=5, max_iter=12)
    b = K.basis(8, 40, 0.0)
    assert (ref["status"] == N.ST_MAXITER).sum() >= 6 and (ref["status"] == N.ST_OK).sum() >= 1
    hidden = 0
    for v in range(12):
        each = [_run(y[:, v], b, mu, max_iter=12)[3:] for mu, _ in stats[v]["trace"]]
        assert ref["nit"][v] == sum(n for n, _ in each) and ref["status"][v] == max(s for _, s in each) and ref["nit"][v] <= 12 * ref["solves"][v]
        hidden += each[-1][1] == N.ST_OK and ref["status"][v] == N.ST_MAXITER
    assert hidden >= 1  # a step limit in an earlier solve shows although the final one is fine


def test_edge_voxels_and_masks():
    y, ref, _ = Q.reference(8, 40, "edge", 14, seed=5)
    names = K.edge_voxels(8)[1]
    at = names.index
    for name in ("nan", "inf", "minus_inf_last"):
        v = at(name)
        assert ref["status"][v] == N.ST_NONFINITE and ref["rule"][v] == N.RULE_NONE and ref["solves"][v] == 0
        assert not any(ref[k][..., v].any() for k in Q.OUTPUTS if k not in ("status", "rule"))
    for name in ("zeros", "negative", "minus_zero"):  # nothing to fit: the misfit is sum y^2, no weight changes it
        v = at(name)
        assert ref["status"][v] == N.ST_OK and ref["nit"][v] == 0 and ref["amp"][v] == 0
    assert ref["rule"][at("zeros")] == N.RULE_EXACT and ref["rule"][at("negative")] == N.RULE_HIGH and ref["ratio"][at("negative")] == 1
    assert np.isfinite(ref["ratio"]).all() and np.isfinite(ref["mu"]).all()
    mask = K.holes_mask(30, 3)
    _, want = Q.tiled(30, mask, n_te=8, n_basis=40, kind="edge", n_unique=14, seed=5)
    got = N.solve_chi2(np.ascontiguousarray(y[:, np.arange(30) % 14]), K.basis(8, 40, 0.0), mask)
    assert all(got[k].tobytes() == want[k].tobytes() for k in Q.OUTPUTS)
    off = mask == 0
    assert np.all(got["rule"][off] == N.RULE_NONE) and np.all(got["status"][off] == N.ST_MASKED) and not got["mu"][off].any()
    with pytest.raises(ValueError, match="mu 0"):
        N.solve_voxel_chi2(y[:, 0], K.basis(8, 40, 1e-3))
    with pytest.raises(TypeError, match="unknown"):
        N.solve_chi2(y, K.basis(8, 40, 0.0), facter=1.02)


def test_noisier_voxels_get_a_larger_weight():
    """decays(8, 24, 5): measured medians 0.0082 at sigma 10 and 0.050 at sigma 50; the ordering is what is asserted."""
    b = K.basis(8, 40, 0.0)
    quiet = N.solve_chi2(K.decays(8, 24, 5, sigma=10.0), b)["mu"]
    noisy = N.solve_chi2(K.decays(8, 24, 5, sigma=50.0), b)["mu"]
    print(f"median chosen mu: sigma 10 {np.median(quiet):.4g}, sigma 50 {np.median(noisy):.4g}")
    assert np.median(noisy) > np.median(quiet)


def test_refusals_without_a_device(lib):
    err = lambda: lib.t2fit_last_error().decode()
    p, c = _abi.T2FitNnlsParams(), _abi.T2FitNnlsChi2Params()
    assert lib.t2fit_nnls_params_default(C.byref(p)) == _abi.OK
    assert lib.t2fit_nnls_chi2_params_default(None) == _abi.E_INVALID and "NULL" in err()
    assert lib.t2fit_nnls_chi2_params_default(C.byref(c)) == _abi.OK
    assert {k: getattr(c, k) for k in N.CHI2_DEFAULTS} == N.CHI2_DEFAULTS and C.sizeof(c) == 48
    from fetal_t2mapping_amd import _gpu_nnls

    assert _gpu_nnls.chi2_params(factor=1.1, n_bisect=2).factor == 1.1 and _gpu_nnls.chi2_params(n_bisect=2).n_bisect == 2
    assert _gpu_nnls.chi2_params().mu_exact == _gpu_nnls.DEFAULT_MU
    ptr = C.c_void_p(4096)
    names = ("params", "chi2", "y", "n_te", "n_vox", "mask", "packed", "x", "func", "amp", "rmse", "nit", "status", "mu", "ratio", "solves", "rule")

    def dev(**kw):
        a = {n: ptr for n in names}
        a.update(params=C.byref(p), chi2=C.byref(c), n_te=8, n_vox=10, mask=None)
        a.update(kw)
        return lib.t2fit_nnls_chi2_dev(*(a[n] for n in names), None)

    for name in ("params", "chi2", "y", "packed", "amp", "rmse", "nit", "status", "mu", "ratio", "solves", "rule"):
        assert dev(**{name: None}) == _abi.E_INVALID and "NULL" in err() and "t2fit_nnls_chi2_dev" in err(), name
    assert dev(n_te=1) == _abi.E_INVALID and "n_te" in err()
    assert dev(n_te=33) == _abi.E_INVALID and "n_te" in err()
    assert dev(n_vox=-1) == _abi.E_INVALID and "negative" in err()
    for name in ("y", "x", "func", "amp", "mu", "ratio", "solves", "rule"):
        assert dev(**{name: C.c_void_p(4098)}) == _abi.E_INVALID and "4 bytes" in err(), name
    assert dev(packed=C.c_void_p(4104)) == _abi.E_INVALID and "16 bytes" in err()
    for field, value in (("tol_rel", -1.0), ("piv_rel", float("inf")), ("max_iter", -1), ("max_blocks", -2)):
        q = _abi.T2FitNnlsParams()
        lib.t2fit_nnls_params_default(C.byref(q))
        setattr(q, field, value)
        assert dev(params=C.byref(q)) == _abi.E_INVALID and field in err(), field
    nan, inf = float("nan"), float("inf")
    for field, values in (("factor", (1.0, 0.5, nan, inf)), ("grow", (1.0, -4.0, nan, inf)), ("mu_first", (0.0, -1e-3, nan, inf)),
                          ("exact_rel", (-1e-12, nan, inf)), ("mu_exact", (-0.03, nan, inf)), ("n_grow", (-1, 65)), ("n_bisect", (-1, 65))):
        for value in values:
            q = _gpu_nnls.chi2_params(**{field: value})
            assert dev(chi2=C.byref(q)) == _abi.E_INVALID and field in err(), (field, value)
            with pytest.raises(ValueError, match=field):
                N.check_chi2(**{**N.CHI2_DEFAULTS, field: value})
    for field, value in (("n_grow", 0), ("n_grow", 64), ("n_bisect", 0), ("n_bisect", 64), ("exact_rel", 0.0), ("mu_exact", 0.0)):
        assert dev(chi2=C.byref(_gpu_nnls.chi2_params(**{field: value})), n_vox=0) == _abi.OK  # the ends of the ranges; a no-op
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "t2fit.h")).read()
    for name in _abi.NNLS_CHI2_SYMBOLS:
        assert name + "(" in header and hasattr(lib, name) and name in _abi.LOOKED_UP
    for const in ("FOUND", "EXACT", "LOW", "HIGH"):
        value = getattr(_abi, "NNLS_RULE_" + const)
        assert f"#define T2FIT_NNLS_RULE_{const} {value}" in header and getattr(N, "RULE_" + const) == value
    assert lib.t2fit_abi_version() == 5


def test_cli_flags(tmp_path, capsys):
    from fetal_t2mapping_amd import cli as R

    base = ["--path", str(tmp_path), "--csv", "log.csv", "--in_vivo", "--lf", "--sim", "1", "--gaussian"]
    nnls = ["--solver", "nnls", "--nnls_t2", "10:2000:40"]
    plain = {"t2": (10.0, 2000.0, 40), "mu": R.NNLS_DEFAULT_MU, "windows": {}, "write_spectrum": False}
    assert R.parse_arguments(base + nnls).nnls_args == plain  # without the flag: no new key
    args = R.parse_arguments(base + nnls + ["--nnls_chi2"])
    assert args.nnls_args == {**plain, "mu": 0.0, "chi2": {"factor": 1.02, "mu_exact": R.NNLS_DEFAULT_MU}} and R.NNLS_CHI2_FACTOR == 1.02
    assert R.build_spectrum_basis(args.nnls_args, [114.0, 202.0, 299.0]).mu == 0.0
    args = R.parse_arguments(base + ["--nnls_chi2", "1.05", "--nnls_chi2_fallback", "0.1"] + nnls + ["--write_spectrum"])
    assert args.nnls_args == {**plain, "mu": 0.0, "write_spectrum": True, "chi2": {"factor": 1.05, "mu_exact": 0.1}}
    assert R.parse_arguments(base + nnls + ["--nnls_chi2", "--nnls_chi2_fallback", "0"]).nnls_args["chi2"] == {"factor": 1.02, "mu_exact": 0.0}
    refused = [
        (nnls + ["--nnls_chi2", "--nnls_mu", "0.1"], "cannot be combined with --nnls_mu"),
        (nnls + ["--nnls_chi2", "1.0"], "above 1"),
        (nnls + ["--nnls_chi2", "0.5"], "above 1"),
        (nnls + ["--nnls_chi2", "nan"], "above 1"),
        (nnls + ["--nnls_chi2", "inf"], "above 1"),
        (nnls + ["--nnls_chi2", "--nnls_chi2_fallback", "-0.1"], "--nnls_chi2_fallback"),
        (nnls + ["--nnls_chi2", "--nnls_chi2_fallback", "nan"], "--nnls_chi2_fallback"),
        (nnls + ["--nnls_chi2_fallback", "0.1"], "no effect without --nnls_chi2"),
        (["--nnls_chi2"], "no effect without --solver nnls"),
        (["--solver", "lm", "--nnls_chi2", "1.02"], "no effect without --solver nnls"),
        (["--solver", "lm", "--nnls_chi2_fallback", "0.1"], "no effect without --solver nnls"),
    ]
    for extra, word in refused:
        with pytest.raises(SystemExit):
            R.parse_arguments(base + extra)
        assert word in capsys.readouterr().err, extra


def test_the_sweep_phantom_under_the_rule():
    """The phantom and the voxels of tools/nnls_mu_sweep.py: the median relative error of the geometric-mean T2 under the
    rule, printed beside the fixed weight's (0.15 at mu 0.03, all vials).  Recorded in DESIGN.md section 8w; no bound is
    asserted on it -- only that the rule ran on every voxel."""
    from fetal_t2mapping_amd import synth

    echoes, mask, label, te, gt = synth.phantom_volume()
    grid = N.log_grid(10, 2000, 40)
    b = N.Basis(N.monoexp_basis(te, grid), 0.0)
    rng = np.random.default_rng(0)
    rows = []
    for i, v in enumerate(gt):
        idx = np.flatnonzero(label.reshape(-1) == i + 1)
        rows += [(j, v) for j in rng.choice(idx, 25, replace=False)][:5]  # the sweep's draw; its first 5 voxels per vial
    y = echoes.reshape(len(te), -1)
    ln_t2 = N.ln_t2_functional(grid)
    err, mid, mus, rules = [], [], [], []
    for j, v in rows:
        x, P, nit, status, mu, ratio, solves, rule = N.solve_voxel_chi2(y[:, j], b)
        g = np.exp((ln_t2 * x).sum() / x.sum())
        err.append(abs(g - v) / v)
        mus.append(mu)
        rules.append(rule)
        if 40 <= v <= 700:
            mid.append(abs(g - v) / v)
    print(f"chi2 rule, {len(rows)} voxels: median relative error of the geometric-mean T2, all vials {np.median(err):.4f}, vials of "
          f"40 .. 700 ms {np.median(mid):.4f}; median mu {np.median(mus):.4g}; rules {np.bincount(rules, minlength=4).tolist()}")
    assert len(err) == 5 * len(gt) and np.all(np.isfinite(err)) and min(rules) >= 0
