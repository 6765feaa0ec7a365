"""Host side of the TV-Chambolle denoiser (no device): the numpy statement of the definition (fetal_t2mapping_amd/_tv.py)
against properties that pin it independently of any implementation, against the two independent references of
tests/denoise_cases.py (Chambolle's iteration in long double over the table of edge shapes, the exact 1-D minimiser),
mutations of the statement that must each miss those bars, the stop-rule cases' distance from a marginal stop, the ABI of
the built library (version still 5, the
three additive entry points, the workspace arithmetic, every argument check refused with a message before HIP is
touched), and the --denoise flags of the CLI.  tests/test_denoise_gpu.py runs the kernels."""
import ctypes as C
import os

import numpy as np
import pytest

import denoise_cases as K


def _slice(seed=0, sigma=20.0, shape=(96, 80)):
    """A piecewise-constant slice under Rician noise, and the clean slice."""
    rng = np.random.default_rng(seed)
    y, x = shape
    yy, xx = np.meshgrid(np.arange(y), np.arange(x), indexing="ij")
    clean = np.where((yy > y // 5) & (xx > x // 6), 300.0, 0.0)
    clean = np.where((yy > y // 2) & (xx < x // 2), 900.0, clean)
    clean = np.where((yy - y / 2) ** 2 + (xx - x / 2) ** 2 < (min(y, x) / 5) ** 2, 1500.0, clean)
    noisy = np.hypot(clean + rng.normal(scale=sigma, size=shape), rng.normal(scale=sigma, size=shape))
    return noisy.astype(np.float32), clean


def _tv_norm(u):
    g0 = np.zeros_like(u)
    g1 = np.zeros_like(u)
    g0[:-1] = np.diff(u, axis=0)
    g1[:, :-1] = np.diff(u, axis=1)
    return float(np.sqrt(g0 ** 2 + g1 ** 2).sum())


def _rof(u, f, weight):
    return float(((u - f) ** 2).sum()) / (2.0 * weight) + _tv_norm(u)


def test_constant_image_is_a_fixed_point_and_the_mean_is_preserved():
    from fetal_t2mapping_amd import _tv

    flat = np.full((17, 23), 700.0, np.float32)
    out, n_iter, e = _tv.tv_problem(flat, 5.0, 2e-4, 50)
    # E = 0 at every iteration: |E_prev - E| < eps * E_init is 0 < 0, never true, so the loop runs out
    assert np.array_equal(out, flat) and n_iter == 49 and e == 0.0
    f, _ = _slice(1)
    for dtype, tol in ((np.float32, 2e-6), (np.float64, 1e-13)):
        out, n_iter, _ = _tv.tv_problem(f, 20.0, 2e-4, 200, dtype)
        assert 1 < n_iter < 199
        assert abs(out.astype(np.float64).mean() - f.astype(np.float64).mean()) <= tol * f.mean()


def test_transpose_commutes_with_the_result_and_a_flip_nearly_does():
    from fetal_t2mapping_amd import _tv

    f, _ = _slice(2, shape=(48, 40))
    base, n0, e0 = _tv.tv_problem(f, 20.0, 0.0, 30, np.float64)
    out, n, e = _tv.tv_problem(np.ascontiguousarray(f.T), 20.0, 0.0, 30, np.float64)
    # the axes enter symmetrically up to the order of the additions in d: the transpose of the result, to rounding
    assert n == n0 and np.max(np.abs(out - base.T)) <= 1e-12 * np.max(np.abs(base)) and abs(e - e0) <= 1e-12 * e0
    # a flip turns the forward differences into backward ones: another discretisation of the same model, so the result
    # is close (a fraction of the noise level) and not equal
    for op in (lambda a: a[::-1], lambda a: a[:, ::-1]):
        out, n, _ = _tv.tv_problem(np.ascontiguousarray(op(f)), 20.0, 0.0, 30, np.float64)
        diff = np.abs(out - op(base))
        assert n == n0 and 0.0 < np.sqrt(np.mean(diff ** 2)) < 5.0


def test_result_lowers_the_rof_energy_and_the_rmse():
    from fetal_t2mapping_amd import _tv

    f, clean = _slice(3)
    f64 = f.astype(np.float64)
    weight = 20.0
    out, n_iter, _ = _tv.tv_problem(f, weight, 2e-4, 200, np.float64)
    box = np.pad(f64, 1, mode="edge")
    box = sum(box[1 + dy:1 + dy + f.shape[0], 1 + dx:1 + dx + f.shape[1]] for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9.0
    assert _rof(out, f64, weight) < _rof(f64, f64, weight) and _rof(out, f64, weight) < _rof(box, f64, weight)
    rmse = lambda u: float(np.sqrt(np.mean((u - clean) ** 2)))  # noqa: E731
    inside = clean > 0  # where the Rician mean is the signal
    assert np.sqrt(np.mean((out - clean)[inside] ** 2)) < 0.5 * np.sqrt(np.mean((f64 - clean)[inside] ** 2))
    assert rmse(out) < rmse(f64)
    # the reference's setting: weight 0.1 on intensities of hundreds stops after one update and changes next to nothing
    ref, n_ref, _ = _tv.tv_problem(f, 0.1, 2e-4, 200, np.float32)
    assert n_ref == 1 and np.max(np.abs(ref - f)) < 0.5


def test_stack_is_the_slices_one_by_one_and_eps_zero_runs_out():
    from fetal_t2mapping_amd import _tv

    vol = np.stack([_slice(s, shape=(24, 20))[0] for s in range(3)])
    out, n_iter, energy = _tv.denoise_tv(vol[None], 15.0, 2e-4, 200, 2, "f32")
    assert out.shape == (1, 3, 24, 20) and out.dtype == np.float32 and n_iter.shape == (3,)
    for k in range(3):
        o, n, e = _tv.tv_problem(vol[k], 15.0, 2e-4, 200, np.float32)
        assert np.array_equal(out[0, k], o) and n_iter[k] == n and energy[k] == e
    out3, n3, _ = _tv.denoise_tv(vol, 15.0, 0.0, 9, 3, "f64")
    assert n3.shape == (1,) and n3[0] == 8 and not np.array_equal(out3, out[0])
    thin, n_thin, _ = _tv.denoise_tv(np.ones((2, 5, 1), np.float32) * np.arange(5, dtype=np.float32)[None, :, None], 1.0, 0.0, 4)
    assert thin.shape == (2, 5, 1) and np.all(n_thin == 3)


# ---- the statement against the independent references of denoise_cases.py ---------------------------------------------------
@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_statement_equals_the_long_double_reference(case):
    """out within TOL_p eps_p max |f| and the energy within TOL_p eps_p relative, after 1, 2, 7 and 40 updates, on every
    problem of every case of the table, in both precisions (denoise_cases.TOL)."""
    for precision in ("f32", "f64"):
        r_out, r_e = K.check_statement(*case, precision)
        print(f"{K.case_id(case)} {precision}: out {r_out:.3f} energy {r_e:.3f} (bar {K.TOL[precision]:.0f})")


def test_the_measured_ratios_are_the_largest_the_statement_shows():
    """TOL is 16 times MEASURED_RATIO; each figure is reached (to the digits written) on the case named beside it."""
    for precision in ("f32", "f64"):
        want_out, want_e = K.MEASURED_RATIO[precision]
        r_out = K.statement_ratios(*K.WORST_OUT, precision)[0]
        r_e = K.statement_ratios(*K.WORST_ENERGY, precision)[1]
        print(precision, r_out, r_e)
        assert 0.99 * want_out <= r_out <= want_out and 0.99 * want_e <= r_e <= want_e
        assert K.TOL[precision] == 16 * max(want_out, want_e)


def test_the_reference_by_its_own_definition():
    """The long-double reference at a size where the definition can be written out by hand: two voxels in a row."""
    f = np.array([[100.0, 160.0]])
    w = 25.0
    assert np.array_equal(K.ref_updates(f, w, 0), f) and K.ref_energy(f, w, 0) == w * 60.0 / 2
    # one update: p_x(0) = -tau 60 / (1 + tau 60 / w), everything else 0; u = f - div p moves the two towards each other
    p = -0.25 * 60.0 / (1.0 + 0.25 * 60.0 / w)
    u = K.ref_updates(f, w, 1)
    assert np.allclose(u.astype(np.float64), [[100.0 - p, 160.0 + p]], rtol=1e-15) and p < 0
    assert abs(float(K.ref_energy(f, w, 1)) - (2 * p * p + w * (60.0 + 2 * p)) / 2) < 1e-12
    assert K.tiles((1, 1, 1025, 65), 2) == 66 and K.tiles((2, 33, 57, 5), 3) == 72 and K.tiles((1, 1, 1, 1), 3) == 1


def test_one_dimensional_problems_reach_the_exact_minimiser():
    """The float64 statement with eps = 0 against the minimiser bounded least squares finds from the dual (its KKT
    conditions are asserted where it is computed): within 1e-6 after K iterations as a column, a row and a volume, K the
    smallest such count, and within rounding of the solver's u after 20000."""
    worst = K.check_1d(K.K, 1e-6)
    print(f"K = {K.K}: largest distance {worst:.4g}")
    assert 0.99 * K.STATEMENT_DISTANCE["f64"] <= worst <= K.STATEMENT_DISTANCE["f64"]
    assert K.statement_1d(48, 60.0, "volume", K.K - 1)[1] > 1e-6  # K is the smallest
    worst32 = max(K.statement_1d(n, w, form, K.K, "f32")[1] for n, w in K.ONE_D for form in K.ONE_D_FORMS)
    print(f"float32 statement at K: largest distance {worst32:.4g}")
    assert 0.99 * K.STATEMENT_DISTANCE["f32"] <= worst32 <= K.STATEMENT_DISTANCE["f32"]
    for n, w in K.ONE_D:
        f, u = K.exact_1d(n, w)
        dist = K.statement_1d(n, w, "row", 20000)[1]
        print(f"n = {n}, weight {w}: {dist:.3g} from the exact minimiser after 20000 iterations")
        # u = f - D^T z is itself rounded: up to n roundings of values of max |f|, and as many in the statement's
        assert dist <= 2 * n * 2.0 ** -53 * float(np.max(f)) and dist <= K.ONE_D_CONVERGED
        # another scaling of the weight is far away: the minimiser moves by 5 units and more between weight and 2 weight
        assert np.max(np.abs(K.exact_1d(n, 2 * w)[1] - u)) > 5.0


@pytest.mark.parametrize("name", sorted(K.MUTATIONS))
def test_a_mutated_statement_fails(name):
    """Each wrong variant of a step of _tv misses a bar on the case named beside it, in both precisions; the statement
    itself passes there before and after."""
    where = K.MUTATIONS[name][2]

    def check():
        if where == "1d":
            K.statement_1d.cache_clear()
            K.check_1d(K.K, 1e-6)
        else:
            for precision in ("f32", "f64"):
                K.check_statement(*where, precision)

    def fails():
        if where == "1d":
            K.statement_1d.cache_clear()
            with pytest.raises(AssertionError):
                K.check_1d(K.K, 1e-6)
        else:
            for precision in ("f32", "f64"):
                with pytest.raises(AssertionError):
                    K.check_statement(*where, precision)

    check()
    with K.mutated(name):
        fails()
    check()  # (the statement is itself again)


def test_stop_rule_cases_are_not_marginal():
    """The cases of test_denoise_gpu.py's stop-rule test, by the statement: on every iteration of every problem
    |E_prev - E| is at least 1e-9 E_init away from the threshold (the kernel sums the energy in another order than
    np.sum, to about 1e-12), and one call stops problems at odd and at even counts (the finish kernel picks the half of
    the ping-pong pair by parity)."""
    both = False
    for a in K.stop_stacks():
        for dims, precision in ((2, "f32"), (2, "f64"), (3, "f32"), (3, "f64")):
            for weight in K.STOP_WEIGHTS:
                n_iter, margin = K.stop_margins(a, weight, dims, precision)
                print(f"{a.shape} dims {dims} {precision} weight {weight}: n_iter {n_iter.tolist()} margin {margin:.3g}")
                assert margin >= K.STOP_MARGIN, (a.shape, dims, precision, weight, margin)
                stopped = n_iter[n_iter < 199]
                both = both or (np.any(stopped % 2 == 0) and np.any(stopped % 2 == 1))
    assert both


def test_built_library_keeps_abi_5_and_refuses_bad_denoise_arguments_without_a_device():
    from fetal_t2mapping_amd import _abi, build

    assert _abi.ABI_VERSION == 5
    names = [s[0] for s in _abi.SYMBOLS]
    header = open(os.path.join(os.path.dirname(build.PKG), "include", "t2fit.h")).read()
    assert "#define T2FIT_ABI_VERSION 5" in header
    for sym in ("t2fit_tv_params_default", "t2fit_tv_workspace_bytes", "t2fit_tv_denoise_dev"):
        assert sym in names and sym + "(" in header and sym in _abi.ADDITIVE
    assert any(src.endswith("t2fit_denoise.hip") for src in build.SOURCES)
    import torch  # noqa: F401  (one HIP runtime per process: see _lib.load)

    lib = _abi.bind(C.CDLL(build.build()))
    assert lib.t2fit_abi_version() == 5
    par = _abi.T2FitTvParams()
    assert C.sizeof(par) == 32
    assert lib.t2fit_tv_params_default(C.byref(par)) == _abi.OK
    assert (par.weight, par.eps, par.max_iter, par.dims, par.precision, par.flags) == (0.1, 2e-4, 200, 2, _abi.PREC_F32, 0)
    assert lib.t2fit_tv_params_default(None) == _abi.E_INVALID

    up = lambda v: (v + 255) // 256 * 256  # noqa: E731
    cdiv = lambda a, b: (a + b - 1) // b  # noqa: E731

    def want_bytes(dims, elem, n_vol, nz, ny, nx):
        problems = n_vol * nz if dims == 2 else n_vol
        tiles = problems * (cdiv(ny, 32) * cdiv(nx, 64) if dims == 2 else cdiv(nz, 4) * cdiv(ny, 8) * cdiv(nx, 64))
        return 2 * up(dims * n_vol * nz * ny * nx * elem) + up(16 * tiles) + up(32 * problems)

    need = C.c_size_t()
    for dims in (2, 3):
        for prec, elem in ((_abi.PREC_F32, 4), (_abi.PREC_F64, 8)):
            for size in ((8, 256, 256, 256), (6, 180, 256, 256), (1, 1, 1, 1), (2, 5, 37, 53), (3, 16, 17, 1)):
                par.dims, par.precision = dims, prec
                assert lib.t2fit_tv_workspace_bytes(C.byref(par), *size, C.byref(need)) == _abi.OK
                assert need.value == want_bytes(dims, elem, *size), (dims, prec, size)
    assert lib.t2fit_tv_params_default(C.byref(par)) == _abi.OK
    assert lib.t2fit_tv_workspace_bytes(C.byref(par), 1, 4, 4, 4, None) == _abi.E_INVALID

    p = 4096  # never dereferenced: every call below is refused first
    ok_size = (2, 3, 8, 8)
    assert lib.t2fit_tv_workspace_bytes(C.byref(par), *ok_size, C.byref(need)) == _abi.OK

    def refused(fragment, par=par, src=p, dst=p, size=ok_size, ws=p, ws_bytes=None):
        rc = lib.t2fit_tv_denoise_dev(C.byref(par) if par is not None else None, src, dst, *size, ws,
                                      need.value if ws_bytes is None else ws_bytes, None, None, None)
        msg = lib.t2fit_last_error().decode()
        assert rc == _abi.E_INVALID and fragment in msg, (fragment, rc, msg)

    refused("NULL", src=None)
    refused("NULL", dst=None)
    refused("NULL", ws=None)
    refused("params is NULL", par=None)
    refused("workspace too small", ws_bytes=need.value - 1)
    refused("not aligned to 256", ws=p + 64)
    refused("not aligned to 4", src=p + 2)
    for size in ((0, 3, 8, 8), (2, 0, 8, 8), (2, 3, -1, 8), (2, 3, 8, 0)):
        refused(">= 1", size=size)
    refused("2^40", size=(2 ** 31 - 1, 2 ** 31 - 1, 2, 2))
    refused("2^40", size=(2 ** 20, 2 ** 20, 2, 1))
    refused("tiles", size=(2 ** 15, 2 ** 16, 1, 1))

    def with_(**kw):
        q = _abi.T2FitTvParams()
        lib.t2fit_tv_params_default(C.byref(q))
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    for kw, fragment in (({"weight": 0.0}, "weight"), ({"weight": -1.0}, "weight"), ({"weight": float("nan")}, "weight"),
                         ({"weight": float("inf")}, "weight"), ({"eps": -1e-9}, "eps"), ({"eps": float("nan")}, "eps"),
                         ({"max_iter": 0}, "max_iter"), ({"dims": 1}, "dims"), ({"dims": 4}, "dims"),
                         ({"precision": 2}, "precision"), ({"flags": 1}, "flags")):
        refused(fragment, par=with_(**kw))
        assert lib.t2fit_tv_workspace_bytes(C.byref(with_(**kw)), 1, 4, 4, 4, C.byref(need)) == _abi.E_INVALID


def test_cli_denoise_flags(capsys):
    from fetal_t2mapping_amd import cli as R

    base = ["--path", "/x", "--csv", "a.csv", "--in_vivo", "--gaussian", "--lf", "--sim", "1"]
    assert R.parse_arguments(base).denoise_args is None
    a = R.parse_arguments(base + ["--denoise", "tv"])
    assert a.denoise_args == {"weight": ("abs", 0.1), "dims": 2, "eps": 2e-4, "max_iter": 200}
    a = R.parse_arguments(base + ["--denoise", "tv", "--denoise_weight", "0.5sigma", "--denoise_dims", "3", "--denoise_eps", "0",
                                  "--denoise_iter", "50"])
    assert a.denoise_args == {"weight": ("sigma", 0.5), "dims": 3, "eps": 0.0, "max_iter": 50}
    assert R.parse_denoise_weight("sigma") == ("sigma", 1.0) and R.parse_denoise_weight("2 Sigma") == ("sigma", 2.0)
    assert R.parse_denoise_weight("12.5") == ("abs", 12.5)
    for bad in ("0", "-3", "nan", "abc", "0sigma", "sigmas"):
        with pytest.raises(ValueError):
            R.parse_denoise_weight(bad)
    for extra, word in ((["--denoise_weight", "3"], "without --denoise"), (["--denoise_dims", "3"], "without --denoise"),
                        (["--denoise", "tv", "--bootstrap", "10"], "--bootstrap"), (["--denoise", "nlm"], "invalid choice"),
                        (["--denoise", "tv", "--denoise_weight", "-1"], "positive"),
                        (["--denoise", "tv", "--denoise_iter", "0"], "--denoise_iter"),
                        (["--denoise", "tv", "--denoise_eps", "-1"], "--denoise_eps"),
                        (["--denoise", "tv", "--denoise_dims", "4"], "invalid choice")):
        with pytest.raises(SystemExit):
            R.parse_arguments(base + extra)
        assert word in capsys.readouterr().err, extra


def test_denoise_is_refused_on_a_shared_volume(monkeypatch):
    import pandas as pd

    from fetal_t2mapping_amd import cli as R

    monkeypatch.setattr(R, "_dist_env", lambda: (0, 2, 0))  # two ranks, one subject: the volume would be shared
    md = pd.DataFrame([{"prj": "prj-1", "sub": "sub-1", "ses": "ses-1", "run": "run-01", "EchoTime": 0.114}])
    with pytest.raises(ValueError, match="shared by several ranks"):
        R.process_t2maps(md, "/nowhere/", [114], "gaussian", None, False, True, True, False, False, "1",
                         denoise={"weight": ("abs", 1.0), "dims": 2, "eps": 2e-4, "max_iter": 200})
