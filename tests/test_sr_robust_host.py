"""The outlier weighting of the super-resolution loop without a device: the numpy statement (fetal_t2mapping_amd/_sr.py
robust_slice_sums, robust_scale, robust_apply, robust_step) against the definition written with Python floats in
tests/sr_robust_cases.py; the median, the order of the stacks, the edge cases; the step-size argument; the refusals of the
library, of Python and of the command line; the CSV of slice weights; the symbols; and the corrupted phantom."""
import ctypes as C
import os

import numpy as np
import pytest

import sr_cases as K
import sr_robust_cases as RC
from fetal_t2mapping_amd import _sr as S


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_statement_equals_the_definition_in_python_floats(name):
    r, N, masks, params, ref = RC.case(name)
    got = S.robust_step(r, N, masks, params or True)
    for a, b in zip(got[0], ref[0]):
        assert RC.same_bits(a, b)
    for a, b in zip(got[1], ref[1]):
        assert RC.same_bits(a, b)
    assert RC.same_bits(got[2], ref[2]) and RC.same_bits(got[3], ref[3])
    assert all(np.all((w > 0.0) & (w <= 1.0)) for w in got[1])
    assert any(np.any(w < 1.0) for w in got[1]) == (name != "none_eligible")


def test_edge_cases():
    r, N, masks, _, ref = RC.case("edges")
    out, weights, sigma2, sums = S.robust_step(r, N, masks, True)
    c = sums[0, :, 0]
    assert c[0] == 0.0 and c[1] == 15.0 and c[2] == 16.0
    m = sums[0, :, 1] / np.where(c > 0, c, 1.0)
    eligible = c >= 16
    assert not eligible[0] and not eligible[1] and eligible[2]
    assert weights[0][0, 0] == 1.0 and weights[0][0, 1] == 1.0  # not eligible: weight 1 whatever the residual
    assert m[3] == m[4] and weights[0][0, 3] == weights[0][0, 4]  # the tie
    assert sigma2[0] == 0.5 * (np.sort(m[eligible])[(eligible.sum() - 1) // 2] + np.sort(m[eligible])[eligible.sum() // 2])
    # non-finite samples: out of the sums, written as +0.0
    assert c[5] == 16 * 16 - 2 and c[6] == 16 * 16 - 1 and np.isfinite(sums).all()
    for z, y, x in ((5, 3, 3), (5, 3, 4), (6, 0, 0)):
        assert out[0][0, z, y, x] == 0.0 and not np.signbit(out[0][0, z, y, x])
    assert out[1][0, 0, 2, 2] == 0.0 and np.isfinite(out[0][0]).all()
    # samples that are not counted (mask 0) become +0.0
    assert np.all(out[0][0][masks[0] == 0] == 0.0) and not np.signbit(out[0][0][masks[0] == 0]).any()
    # all residuals zero: robustness off, the residual returned unchanged (NaN and -0.0 included), sigma2 reported as 0
    assert sigma2[1] == 0.0 and np.all(weights[0][1] == 1.0) and np.all(weights[1][1] == 1.0)
    assert RC.same_bits(out[0][1], r[0][1]) and np.isnan(out[0][1, 3, 1, 2]) and np.signbit(out[0][1, 3, 1, 1])
    # the floor takes over; a huge min_count leaves no eligible slice
    assert np.all(RC.case("floor")[4][2] == 10000.0)
    off = RC.case("none_eligible")
    assert np.all(off[4][2] == 0.0) and all(RC.same_bits(a, b) for a, b in zip(off[4][0], off[0]))


@pytest.mark.parametrize("n", [1, 2, 3, 6, 7])
def test_median_against_sorted_for_odd_and_even_counts_and_ties(n):
    rng = np.random.default_rng(80 + n)
    m = rng.uniform(1.0, 9.0, n)
    if n >= 3:
        m[1] = m[n // 2] = m[0]  # ties
    c = np.full(n, 32.0)
    sums = np.stack([c, m * c], axis=-1)[None]
    sums = np.concatenate([sums, np.array([[[3.0, 1e9]]])], axis=1)  # an ineligible slice with a huge residual joins nothing
    weights, sigma2 = S.robust_scale(sums, True)
    v = sorted(float(a) / 32.0 for a in m * c)
    assert sigma2[0] == 0.5 * (v[(n - 1) // 2] + v[n // 2])
    assert weights[0, -1] == 1.0


def test_the_order_of_the_stacks_changes_no_bit_of_sigma2_or_a_slice_weight():
    r, N, masks, params, ref = RC.case("six_stacks")
    for perm in ([5, 4, 3, 2, 1, 0], [2, 0, 5, 1, 4, 3]):
        got = S.robust_step([r[i] for i in perm], [N[i] for i in perm], [masks[i] for i in perm], params)
        assert RC.same_bits(got[2], ref[2])
        for k, i in enumerate(perm):
            assert RC.same_bits(got[1][k], ref[1][i]) and RC.same_bits(got[0][k], ref[0][i])


def test_frozen_weights_do_not_increase_the_weighted_data_term():
    """omega <= 1, so ||Omega^(1/2) A|| <= ||A|| and the plain step size stays valid: with the weights frozen and no TV the
    weighted data term 1/2 sum omega r^2 does not increase over five steps (float64 throughout)."""
    cases = [K.small_case(o) for o in ("ax", "cor", "sag")]
    hr = cases[0].hr.shape
    rng = np.random.default_rng(81)
    B, rels, masks = [c.B for c in cases], [c.rel for c in cases], [c.mask for c in cases]
    x = rng.normal(500.0, 100.0, (2,) + hr)
    y = [rng.normal(500.0, 100.0, (2,) + c.stack.shape) for c in cases]
    y[1][:, 1] *= 0.3
    N = [S.forward(None, B[s], cases[s].stack.shape, "box", rels[s], hr_shape=hr)[1] for s in range(3)]
    col = [S.adjoint([S.counted(N[s], masks[s])], [N[s]], [B[s]], "box", [rels[s]], hr, masks=[masks[s]], out_dtype=np.float64).max()
           for s in range(3)]
    tau = S.step_size(col)
    res = lambda v: [S.forward(v, B[s], cases[s].stack.shape, "box", rels[s], y=y[s], mask=masks[s], out_dtype=np.float64)[0]
                     for s in range(3)]
    r0 = res(x)
    _, weights, sigma2, _ = S.robust_step([v.astype(np.float32) for v in r0], N, masks, {"min_count": 8})
    assert np.all(sigma2 > 0.0) and weights[1][:, 1].max() < 1.0
    delta = 2.5 * np.sqrt(sigma2)[:, None, None, None]
    omega = [weights[s][:, :, None, None] * np.where(np.abs(r0[s]) <= delta, 1.0, delta / np.maximum(np.abs(r0[s]), 1e-300))
             for s in range(3)]
    assert all(np.all((w > 0.0) & (w <= 1.0)) for w in omega) and any(np.any(w < 1.0) for w in omega)
    term = lambda r: 0.5 * sum(float(np.sum(w * v * v)) for w, v in zip(omega, r))
    last = term(r0)
    for _ in range(5):
        r = res(x)
        x = S.adjoint([w * v for w, v in zip(omega, r)], N, B, "box", rels, hr, masks=masks, x=x, tau=tau, out_dtype=np.float64)
        now = term(res(x))
        assert now <= last * (1.0 + 1e-12), (now, last)
        last = now
    assert last < 0.9 * term(r0)


def test_python_refusals_and_defaults():
    assert S.robust_params(None) is None and S.robust_params(True) == RC.DEFAULTS == S.ROBUST_DEFAULTS
    assert S.robust_params({"huber": 3})["huber"] == 3.0
    for bad in ({"slice_threshold": 0.0}, {"slice_threshold": np.nan}, {"huber": -1.0}, {"huber": np.inf}, {"min_count": 0},
                {"min_count": 2.5}, {"sigma_floor": -1.0}, {"sigma_floor": np.inf}, {"threshold": 1.0}, "yes", 3):
        with pytest.raises(ValueError):
            S.robust_params(bad)
    stacks, geoms = K.phantom()[:2]
    with pytest.raises(ValueError):
        S.reconstruct_sr(stacks, geoms, n_iter=0, robust={"huber": 0.0})
    with pytest.raises(ValueError, match="4096"):
        S.robust_scale(np.ones((1, 4097, 2)))
    x, _, info = S.reconstruct_sr(stacks, geoms, n_iter=0, robust=True, return_info=True)
    assert info["slice_weights"] is None and info["sigma2"] is None
    assert "slice_weights" not in S.reconstruct_sr(stacks, geoms, n_iter=0, return_info=True)[2]


@pytest.fixture(scope="module")
def lib():
    from fetal_t2mapping_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        from fetal_t2mapping_amd import build

        build.build()
    return _lib.load()


def test_symbols_and_library_refusals_without_a_device(lib):
    from fetal_t2mapping_amd import _abi, build

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "t2fit.h")).read()
    names = {n for n, _, _ in _abi.SYMBOLS}
    older = (_abi.ADDITIVE + _abi.REGISTER_SYMBOLS + _abi.ATLAS_SYMBOLS + _abi.N4_SYMBOLS + _abi.MI_SYMBOLS + _abi.SR_SYMBOLS
             + _abi.SR_SLICE_SYMBOLS + _abi.SVR_SYMBOLS)
    assert len(_abi.SR_ROBUST_SYMBOLS) == 3
    for name in _abi.SR_ROBUST_SYMBOLS:
        assert hasattr(lib, name) and name in names and name + "(" in header and name in _abi.LOOKED_UP and name not in older
    assert lib.t2fit_abi_version() == 5 and "#define T2FIT_ABI_VERSION 5" in header
    assert "#define T2FIT_SR_ROBUST_MAX_SLICES 4096" in header and _abi.SR_ROBUST_MAX_SLICES == S.ROBUST_MAX_SLICES == 4096
    assert any(src.endswith("t2fit_sr_robust.hip") for src in build.SOURCES)
    err = lambda: lib.t2fit_last_error().decode()
    p = _abi.T2FitSrRobustParams()
    assert lib.t2fit_sr_robust_params_default(C.byref(p)) == 0 and lib.t2fit_sr_robust_params_default(None) == _abi.E_INVALID
    assert (p.slice_threshold, p.huber, p.sigma_floor, p.min_count, p.flags) == (1.5, 2.5, 0.0, 16, 0)
    assert {"slice_threshold": p.slice_threshold, "huber": p.huber, "min_count": p.min_count, "sigma_floor": p.sigma_floor} == S.ROBUST_DEFAULTS
    need = C.c_size_t(0)
    lo = (C.c_int32 * 6)(5, 19, 21, 4, 16, 16)
    up = lambda v: (v + 255) // 256 * 256
    assert lib.t2fit_sr_robust_workspace_bytes(2, lo, 5, C.byref(need)) == 0
    assert need.value == up(16 * 5 * 9) + up(8 * 5 * 9) + up(8 * 5)
    assert lib.t2fit_sr_robust_workspace_bytes(2, lo, 5, None) == _abi.E_INVALID and "NULL" in err()
    assert lib.t2fit_sr_robust_workspace_bytes(0, lo, 5, C.byref(need)) == _abi.E_INVALID and "n_stacks" in err()
    assert lib.t2fit_sr_robust_workspace_bytes(2, lo, 0, C.byref(need)) == _abi.E_INVALID
    assert lib.t2fit_sr_robust_workspace_bytes(1, (C.c_int32 * 3)(4097, 1, 1), 1, C.byref(need)) == _abi.E_INVALID and "MAX_SLICES" in err()
    assert lib.t2fit_sr_robust_workspace_bytes(1, (C.c_int32 * 3)(4096, 1, 1), 1, C.byref(need)) == 0
    # the call itself refuses before HIP is touched: made-up pointers are never followed
    P = lambda v: (C.c_void_p * len(v))(*v)
    fake_r, fake_n = P([4096, 8192]), P([4096, 8192])

    def call(n_s=2, r=fake_r, N=fake_n, lo=lo, n_vol=5, par=p, sums=4096, w=4096, s2=4096):
        return lib.t2fit_sr_robust_dev(n_s, r, N, None, lo, n_vol, None if par is None else C.byref(par), sums, w, s2, None)

    def tuned(**kw):
        q = _abi.T2FitSrRobustParams(1.5, 2.5, 0.0, 16, 0)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    for kw, word in ((dict(r=None), "NULL"), (dict(N=None), "NULL"), (dict(lo=None), "NULL"), (dict(par=None), "NULL"),
                     (dict(sums=None), "NULL"), (dict(w=None), "NULL"), (dict(s2=None), "NULL"), (dict(n_s=0), "n_stacks"),
                     (dict(n_s=7), "n_stacks"), (dict(n_vol=0), ">= 1"), (dict(lo=(C.c_int32 * 6)(5, 0, 21, 4, 16, 16)), ">= 1"),
                     (dict(n_s=1, lo=(C.c_int32 * 3)(5000, 2, 2)), "MAX_SLICES"), (dict(r=P([None, 8192])), "NULL"),
                     (dict(N=P([4096, None])), "NULL"), (dict(r=P([4098, 8192])), "aligned"), (dict(N=P([4100, 8192])), "aligned"),
                     (dict(w=4100), "aligned"), (dict(par=tuned(slice_threshold=0.0)), "slice_threshold"),
                     (dict(par=tuned(slice_threshold=float("inf"))), "slice_threshold"), (dict(par=tuned(huber=float("nan"))), "huber"),
                     (dict(par=tuned(huber=0.0)), "huber"), (dict(par=tuned(min_count=0)), "min_count"),
                     (dict(par=tuned(sigma_floor=-0.5)), "sigma_floor"), (dict(par=tuned(sigma_floor=float("nan"))), "sigma_floor"),
                     (dict(par=tuned(flags=2)), "flags")):
        assert call(**kw) == _abi.E_INVALID and word in err(), (kw, err())


def test_command_line_flags_parse_and_are_refused_without_the_sr_method(tmp_path):
    from fetal_t2mapping_amd import cli, recon

    for f in ("sr_robust", "sr_robust_slice", "sr_robust_huber", "sr_write_slice_weights"):
        assert f in recon.SR_FLAGS
    base = ["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo", "--lf"]
    plain = recon.parse_arguments(base + ["--recon_method", "sr"]).sr_args
    assert "robust" not in plain and "write_slice_weights" not in plain
    assert recon.parse_arguments(base + ["--recon_method", "sr", "--sr_robust"]).sr_args["robust"] is True
    args = recon.parse_arguments(base + ["--recon_method", "sr", "--sr_robust", "--sr_robust_slice", "2", "--sr_robust_huber=3.5",
                                         "--sr_write_slice_weights", "w.csv"])
    assert args.sr_args["robust"] == {"slice_threshold": 2.0, "huber": 3.5} and args.sr_args["write_slice_weights"] == "w.csv"
    for bad in (["--sr_robust"], ["--sr_robust_slice", "2"], ["--sr_robust_huber=2"], ["--sr_write_slice_weights", "w.csv"],
                ["--recon_method", "average", "--sr_robust"],
                ["--recon_method", "sr", "--sr_robust_slice", "2"], ["--recon_method", "sr", "--sr_robust_huber", "2"],
                ["--recon_method", "sr", "--sr_write_slice_weights", "w.csv"],
                ["--recon_method", "sr", "--sr_robust", "--sr_robust_slice", "0"],
                ["--recon_method", "sr", "--sr_robust", "--sr_robust_huber", "nan"],
                ["--recon_method", "sr", "--sr_robust", "--sr_estimate_slices", "1", "--sr_write_slice_weights", "w.csv"]):
        with pytest.raises(SystemExit):
            recon.parse_arguments(base + bad)
    fit = base + ["--gaussian", "--sim", "s"]
    args = cli.parse_arguments(fit + ["--reconstruct", "--recon_method", "sr", "--recon_sr_robust", "--recon_sr_robust_huber", "3"])
    assert args.reconstruct_args["sr"]["robust"] == {"huber": 3.0}
    for bad in (["--reconstruct", "--recon_sr_robust"], ["--recon_sr_robust"],
                ["--reconstruct", "--recon_method", "sr", "--recon_sr_robust_slice", "2"]):
        with pytest.raises(SystemExit):
            cli.parse_arguments(fit + bad)


def test_the_csv_of_slice_weights_reads_back(tmp_path):
    from fetal_t2mapping_amd import recon

    r, N, masks, params, ref = RC.case("tuned")
    _, weights, sigma2, sums = ref
    path = str(tmp_path / "sub" / "weights.csv")
    recon.save_slice_weights(path, ["ax", "cor", "sag"], weights, sums, sigma2)
    lines = open(path).read().splitlines()
    assert lines[0] == "stack,slice,echo,weight,count,mean_square_residual" and lines[-1].startswith("sigma,2,")
    rows, sigma = recon.load_slice_weights(path)
    n_slices = sums.shape[1]
    assert len(rows) == 3 * n_slices and len(lines) == 1 + 3 * n_slices + 3
    first = {"ax": 0, "cor": weights[0].shape[1], "sag": weights[0].shape[1] + weights[1].shape[1]}
    for o, k, e, w, c, ms in rows:
        assert w == weights[["ax", "cor", "sag"].index(o)][e, k]
        assert c == sums[e, first[o] + k, 0] and ms == (sums[e, first[o] + k, 1] / c if c else 0.0)
    assert sigma == {e: float(np.sqrt(sigma2[e])) for e in range(3)}
    open(path, "w").write("a,b\n")
    with pytest.raises(ValueError):
        recon.load_slice_weights(path)


def test_the_corrupted_phantom():
    """Measured with the statement (defaults, slice_threshold 1.5, huber 2.5): interior RMSE plain on clean data 102.43,
    plain on corrupted data 267.06, robust on clean data 100.43, robust on corrupted data 120.19; at the last iteration the
    largest weight of a corrupted slice is 0.250 and the smallest of a clean slice 0.931."""
    clean, bad, geoms, truth, grid = RC.corrupted_phantom()
    rmse, info = {}, None
    for key, stacks, robust in (("pc", clean, None), ("pb", bad, None), ("rc", clean, True), ("rb", bad, True)):
        if key == "pc":  # the plain loop on the clean phantom is shared with the other super-resolution tests
            x, hi, info = K.phantom_statement(S.DEFAULT_N_ITER, S.DEFAULT_PROX_ITER)
        else:
            x, hi, info = S.reconstruct_sr(stacks, geoms, robust=robust, return_info=True)
        rmse[key] = K.interior_rmse(x, truth, grid, hi.GetOrigin())
    assert info["sigma2"].shape == (3,) and [w.shape for w in info["slice_weights"]] == [(3, 12)] * 3
    RC.check_phantom_conditions(rmse["pc"], rmse["pb"], rmse["rc"], rmse["rb"], info["slice_weights"], ["ax", "cor", "sag"])
