"""The T2-spectrum fit without a GPU: the numpy statement (fetal_t2mapping_amd/_nnls.py) against the KKT conditions of
``min |A x - y|^2 + mu^2 |x|^2, x >= 0`` from the definition, against scipy.optimize.nnls on the augmented system, on exact
and hand-built cases (one column, h <= 0, a 2 x 2 problem in Python floats, a first insertion that must leave, a banned
near-dependent column, the step limit), row reuse against refactoring from scratch, the coverage the random cases must
reach, the packed block against t2fit_nnls_pack_host byte for byte, every refusal of the C entry points, the CLI flags
and refusals, the 4-D NIfTI series the CLI writes, and the ABI."""
import ctypes as C
import math

import numpy as np
import pytest

import nnls_cases as K
from fetal_t2mapping_amd import _abi, _nnls as N

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def lib():
    from fetal_t2mapping_amd import build
    from fetal_t2mapping_amd._lib import load

    build.build()
    return load()


@pytest.fixture(scope="module")
def random_runs():
    """Every (basis, voxel) of the random case set, solved once: ``[(basis, y, x, P, nit, status, stats)]``."""
    runs = []
    for c, (n_te, n_basis, mu) in enumerate(K.SCIPY_CASES):
        b = K.basis(n_te, n_basis, mu)
        y = K.decays(n_te, K.SCIPY_VOXELS, seed=1000 + c)
        for v in range(K.SCIPY_VOXELS):
            st = {}
            x, P, nit, status = N.solve_voxel(y[:, v], b, stats=st)
            runs.append((b, y[:, v], x, P, nit, status, st))
    return runs


def test_kkt_conditions_from_the_definition(random_runs):
    """x >= 0; with w = A^T (y - A x) - mu^2 x recomputed by numpy: w <= tol off the support, |w| small on it.  The bound on the
    support: x_P solves (G_PP + E) x = h_P with |E| <= gamma_{3p+1} |L| |L^T| (Cholesky and the two substitutions, Higham
    2002, theorem 10.4), so |h_P - G_PP x_P| <= (3 p + 1) eps p |G|_2 |x|_2 to first order (| |L| |L^T| |_2 <= p |G|_2); forming
    G by ascending sums and recomputing w here each add at most (n_te + p + 2) eps (|A|^T (|y| + |A| |x|) + mu^2 |x|).  A column
    that is banned when the fit ends is off the support with w_j > tol by construction: w_j is the inner product of the
    augmented residual (r, -mu x) with the part of the augmented column (a_j, mu e_j) orthogonal to the passive columns, and
    the squared norm of that part is the exact pivot, which the refusal bounds by piv_rel G_jj up to the factor's rounding
    (3 p + 1) eps p G_jj: w_j <= sqrt((piv_rel + (3 p + 1) eps p) G_jj) |(r, mu x)|_2."""
    worst, n_banned = 0.0, 0
    for b, y, x, P, nit, status, st in random_runs:
        assert status == N.ST_OK and np.all(x >= 0) and sorted(np.flatnonzero(x > 0)) == sorted(P)
        y64 = y.astype(np.float64)
        w = b.A.T @ (y64 - b.A @ x) - b.mu ** 2 * x
        p = len(P)
        solve_err = (3 * p + 1) * EPS * p * np.linalg.norm(b.G, 2) * np.linalg.norm(x)
        eval_err = 2 * (b.n_te + p + 2) * EPS * np.max(np.abs(b.A).T @ (np.abs(y64) + np.abs(b.A) @ x) + b.mu ** 2 * x)
        bound = solve_err + eval_err
        tol = N.TOL_REL * np.max(np.abs(b.A.T @ y64))
        off = np.ones(b.n_basis, bool)
        off[P] = False
        off[st["banned"]] = False
        assert np.all(w[off] <= tol + bound), (b.n_basis, b.mu, w[off].max(), tol, bound)
        r_aug = math.sqrt(float(np.sum((y64 - b.A @ x) ** 2) + b.mu ** 2 * np.sum(x ** 2)))
        for j in st["banned"]:
            n_banned += 1
            assert j not in P and w[j] <= math.sqrt((N.PIV_REL + (3 * p + 1) * EPS * p) * b.G[j, j]) * r_aug + bound, (b.n_basis, b.mu, j, w[j])
        assert np.all(np.abs(w[P]) <= bound), (b.n_basis, b.mu, np.abs(w[P]).max(), bound)
        worst = max(worst, float(np.abs(w[P]).max() / bound))
    print(f"largest |w| on the support relative to its bound: {worst:.3g}; {n_banned} columns end banned")


def test_against_scipy_on_the_augmented_system(random_runs):
    from scipy.optimize import nnls

    res_gap = coef_gap = res_gap0 = 0.0
    for b, y, x, P, nit, status, st in random_runs:
        aug = np.vstack([b.A, b.mu * np.eye(b.n_basis)])
        rhs = np.concatenate([y.astype(np.float64), np.zeros(b.n_basis)])
        xs, rn = nnls(aug, rhs)
        gap = abs(np.linalg.norm(aug @ x - rhs) - rn) / rn
        if b.mu >= 1e-3:
            res_gap = max(res_gap, gap)
            coef_gap = max(coef_gap, float(np.max(np.abs(x - xs)) / np.max(xs)))
        else:
            res_gap0 = max(res_gap0, gap)
    print(f"measured: residual gap {res_gap:.3g}, coefficient gap {coef_gap:.3g}, residual gap at mu = 0 {res_gap0:.3g}")
    assert res_gap <= 10 * K.MEASURED_RESIDUAL_GAP
    assert coef_gap <= 10 * K.MEASURED_COEFFICIENT_GAP
    assert res_gap0 <= 10 * K.MEASURED_RESIDUAL_GAP_MU0


def test_coverage_of_the_random_cases(random_runs):
    """At least half take a removal and at least one fills the passive set: the removal path is hot, and no cap below n_basis
    is safe."""
    removals = sum(st["removals"] > 0 for *_, st in random_runs)
    full = sum(st["max_p"] == b.n_basis for b, *_, st in random_runs)
    print(f"{removals} of {len(random_runs)} take a removal, {full} reach p = n_basis, most outer steps {max(r[4] for r in random_runs)}")
    assert 2 * removals >= len(random_runs) and full >= 1


def test_row_reuse_equals_refactoring_from_scratch(random_runs):
    for b, y, x, P, nit, status, st in random_runs:
        x2, P2, nit2, status2 = N.solve_voxel(y, b, reuse_rows=False)
        assert x2.tobytes() == x.tobytes() and P2 == P and (nit2, status2) == (nit, status)
    # the factor itself: drop a position from a list, recompute from there; against every row from scratch
    b = K.basis(32, 64, 1e-2)
    order = np.random.default_rng(5).permutation(64)[:20]
    L = np.zeros((64, 64))
    for r in range(20):
        assert N.factor_row(L, b.G, order, r, N.PIV_REL)
    for drop in (0, 7, 19):
        kept = np.delete(order, drop)
        reused, scratch = L.copy(), np.zeros((64, 64))
        for r in range(drop, 19):
            assert N.factor_row(reused, b.G, kept, r, N.PIV_REL)
        for r in range(19):
            assert N.factor_row(scratch, b.G, kept, r, N.PIV_REL)
        assert reused[:19, :19].tobytes() == scratch[:19, :19].tobytes()
        Lk = np.tril(scratch[:19, :19])
        assert np.allclose(Lk @ Lk.T, b.G[np.ix_(kept, kept)], rtol=1e-12, atol=0)


def test_one_column_gives_that_column_alone():
    """mu = 0.  In the decay basis the last column has the largest norm, so it is the first candidate and nothing follows; in
    a table with orthogonal columns every column is recovered."""
    A = K.basis(8, 40, 0.0).A.astype(np.float32).astype(np.float64)  # (the samples are float32: the column must be one)
    b = N.Basis(A, 0.0)
    x, P, nit, status = N.solve_voxel(A[:, -1].astype(np.float32), b)
    assert P == [39] and nit == 1 and status == N.ST_OK and abs(x[39] - 1.0) <= 4 * EPS and not x[:39].any()
    H = np.array([[1.0]])
    for _ in range(3):
        H = np.block([[H, H], [H, -H]])  # the 8 x 8 Hadamard matrix: orthogonal columns of +-1
    Q = H[:, :5] * (1.0 + np.arange(5))[None, :]
    assert np.count_nonzero(Q.T @ Q - np.diag(np.diag(Q.T @ Q))) == 0
    b = N.Basis(Q, 0.0)
    for j in range(5):
        x, P, nit, status = N.solve_voxel((3.0 * Q[:, j]).astype(np.float32), b)
        assert P == [j] and abs(x[j] - 3.0) <= 8 * EPS and status == N.ST_OK


def test_h_not_above_zero_gives_zero_and_no_step():
    b = K.basis(8, 40, 1e-3)
    for y in (-b.A[:, 7], np.zeros(8)):
        x, P, nit, status = N.solve_voxel(y.astype(np.float32), b)
        assert not x.any() and P == [] and nit == 0 and status == N.ST_OK
    out = N.solve(np.stack([-b.A[:, 7], np.zeros(8)], axis=1).astype(np.float32), b)
    assert not out["x"].any() and not out["amp"].any() and out["rmse"][1] == 0 and out["rmse"][0] > 0 and not out["status"].any()


def test_two_by_two_by_hand():
    """Every step of the definition in Python floats: column 1 goes in, then column 0, both stay."""
    (a00, a01), (a10, a11) = K.HAND_A.tolist()
    y0, y1 = (float(v) for v in K.HAND_Y)
    m2 = K.HAND_MU * K.HAND_MU
    g00, g01, g11 = (0.0 + a00 * a00 + a10 * a10) + m2, 0.0 + a00 * a01 + a10 * a11, (0.0 + a01 * a01 + a11 * a11) + m2
    h0, h1 = 0.0 + a00 * y0 + a10 * y1, 0.0 + a01 * y0 + a11 * y1
    assert (h0, h1) == (11.0, 18.0)  # column 1 is the first candidate
    l00 = math.sqrt(g11)
    x1 = (h1 / l00) / l00
    assert h0 - g01 * x1 > N.TOL_REL * 18.0  # column 0 is the second: the list is (1, 0)
    l10 = g01 / l00
    l11 = math.sqrt(g00 - l10 * l10)
    z0 = h1 / l00
    z1 = (h0 - l10 * z0) / l11
    s1 = z1 / l11
    s0 = (z0 - l10 * s1) / l00
    assert s0 > 0 and s1 > 0
    b = N.Basis(K.HAND_A, K.HAND_MU)
    assert b.G.tolist() == [[g00, g01], [g01, g11]]
    x, P, nit, status = N.solve_voxel(K.HAND_Y, b)
    assert P == [1, 0] and nit == 2 and status == N.ST_OK and x.tolist() == [s1, s0]
    det = g00 * g11 - g01 * g01
    assert np.allclose(x, [(h0 * g11 - g01 * h1) / det, (g00 * h1 - g01 * h0) / det], rtol=1e-14)
    func, amp, rmse = N.outputs_voxel(K.HAND_Y, N.Basis(K.HAND_A, K.HAND_MU, [[1.0, -2.0]], ("w",)), x, P)
    assert func[0] == np.float32(0.0 + 1.0 * x[0] + -2.0 * x[1]) and amp == np.float32(0.0 + x[0] + x[1])
    r0, r1 = (y0 - a01 * x[1]) - a00 * x[0], (y1 - a11 * x[1]) - a10 * x[0]
    assert rmse == np.float32(math.sqrt((0.0 + r0 * r0 + r1 * r1) / 2.0))


def test_first_inserted_coefficient_leaves():
    b = N.Basis(K.FIRST_LEAVES_A, 0.0)
    assert int(np.argmax(b.A.T @ K.FIRST_LEAVES_Y)) == 2
    st = {}
    x, P, nit, status = N.solve_voxel(K.FIRST_LEAVES_Y, b, stats=st)
    assert P == [0] and st["removals"] == 1 and status == N.ST_OK and x[1] == 0 and x[2] == 0 and abs(x[0] - 1.1) < 1e-15


def test_near_dependent_pair_is_banned():
    b = N.Basis(K.BAN_A, 0.0)
    st = {}
    x, P, nit, status = N.solve_voxel(K.BAN_Y, b, stats=st)
    assert st["bans"] == 1 and P == [0] and x[1] == 0 and abs(x[0] - 1.0) <= 4 * EPS and status == N.ST_OK
    assert nit == 2  # the refused insertion counts as an outer step
    # with the pivot test off nothing is banned: the column goes in on a pivot that is rounding error
    st = {}
    N.solve_voxel(K.BAN_Y, b, piv_rel=0.0, stats=st)
    assert st["bans"] == 0 and st["max_p"] == 2


def test_step_limit():
    b = K.basis(8, 40, 1e-3)
    y = K.decays(8, 1, seed=3)[:, 0]
    x, P, nit, status = N.solve_voxel(y, b, max_iter=1)
    assert status == N.ST_MAXITER and nit == 1 and len(P) == 1
    full = N.solve_voxel(y, b)
    assert full[3] == N.ST_OK and full[2] > 1 and N.solve_voxel(y, b, max_iter=full[2])[3] == N.ST_OK
    assert N.solve_voxel(y, b, max_iter=full[2] - 1)[3] == N.ST_MAXITER


def test_volume_statement_masks_and_non_finite():
    b = K.basis(3, 17, 1e-3, n_func=2)
    y, names = K.edge_voxels(3)
    mask = np.ones(len(names), np.uint8)
    mask[names.index("huge")] = 0
    out = N.solve(y, b, mask)
    for n in ("nan", "inf", "minus_inf_last"):
        v = names.index(n)
        assert out["status"][v] == N.ST_NONFINITE and not out["x"][:, v].any() and out["amp"][v] == 0 and out["nit"][v] == 0
    v = names.index("huge")
    assert out["status"][v] == N.ST_MASKED and not out["x"][:, v].any() and out["rmse"][v] == 0
    assert out["status"][names.index("zeros")] == N.ST_OK and out["amp"][names.index("one_sample")] > 0
    d = N.derived(out["func"], out["amp"], b.names)
    assert set(d) == {"gmt2", "shortfraction"} and d["gmt2"][names.index("zeros")] == 0
    ok = out["amp"] > 0
    assert np.all((d["gmt2"][ok] >= 10 * (1 - 1e-6)) & (d["gmt2"][ok] <= 2000 * (1 + 1e-6)))
    assert np.all((d["shortfraction"] >= 0) & (d["shortfraction"] <= 1 + 1e-6))


@pytest.mark.parametrize("n_te,n_basis,n_func", [(2, 2, 0), (3, 17, 1), (8, 40, 4), (31, 63, 8), (32, 64, 8)])
def test_pack_equals_the_library_byte_for_byte(lib, n_te, n_basis, n_func):
    from fetal_t2mapping_amd import _gpu_nnls

    b = K.basis(n_te, n_basis, 0.03, n_func)
    want = N.pack(b)
    got = _gpu_nnls.pack(b)
    assert got.dtype == np.uint8 and got.size == N.layout(n_te, n_basis, n_func)[3] and got.tobytes() == want.tobytes()
    assert np.array_equal(b.G, b.G.T)


def test_refusals_of_the_c_entry_points(lib):
    err = lambda: lib.t2fit_last_error().decode()
    need = C.c_size_t(0)
    assert lib.t2fit_nnls_params_default(None) == _abi.E_INVALID and "NULL" in err()
    assert lib.t2fit_nnls_pack_bytes(8, 40, 4, None) == _abi.E_INVALID and "NULL" in err()
    for n_te, n_basis, n_func, word in ((1, 40, 0, "n_te"), (33, 40, 0, "n_te"), (8, 1, 0, "n_basis"), (8, 65, 0, "n_basis"), (8, 40, -1, "n_func"),
                                        (8, 40, 9, "n_func")):
        assert lib.t2fit_nnls_pack_bytes(n_te, n_basis, n_func, C.byref(need)) == _abi.E_INVALID and word in err()
    assert lib.t2fit_nnls_pack_bytes(8, 40, 4, C.byref(need)) == _abi.OK and need.value == N.layout(8, 40, 4)[3]
    A = np.ascontiguousarray(K.basis(8, 40, 0.0).A)
    W = np.ascontiguousarray(K.basis(8, 40, 0.0).W)
    out = np.zeros(need.value, np.uint8)
    pack = lambda n_te=8, n_basis=40, n_func=4, a=A, mu=0.01, w=W, o=out, size=None: lib.t2fit_nnls_pack_host(
        n_te, n_basis, n_func, None if a is None else a.ctypes.data, mu, None if w is None else w.ctypes.data, None if o is None else o.ctypes.data,
        o.nbytes if size is None and o is not None else (size or 0))
    assert pack() == _abi.OK
    assert pack(n_te=1) == _abi.E_INVALID and "n_te" in err()
    assert pack(n_basis=65) == _abi.E_INVALID and "n_basis" in err()
    assert pack(n_func=9) == _abi.E_INVALID and "n_func" in err()
    assert pack(a=None) == _abi.E_INVALID and "NULL" in err()
    assert pack(w=None) == _abi.E_INVALID and "NULL" in err()
    assert pack(o=None) == _abi.E_INVALID and "NULL" in err()
    assert pack(n_func=0, w=None) == _abi.OK  # no functional, no table
    assert pack(size=need.value - 1) == _abi.E_INVALID and "bytes" in err()
    for mu in (-1e-3, float("nan"), float("inf")):
        assert pack(mu=mu) == _abi.E_INVALID and "mu" in err()
    for bad in (np.nan, np.inf):
        a = A.copy()
        a[3, 5] = bad
        assert pack(a=a) == _abi.E_INVALID and "non-finite" in err() and "echo 3" in err() and "column 5" in err()
        w = W.copy()
        w[2, 1] = bad
        assert pack(w=w) == _abi.E_INVALID and "functional 2" in err()
    # the device entry refuses these before HIP is touched
    p = _abi.T2FitNnlsParams()
    assert lib.t2fit_nnls_params_default(C.byref(p)) == _abi.OK and (p.tol_rel, p.piv_rel, p.max_iter, p.max_blocks) == (1e-10, 1e-12, 0, 0)
    ptr = C.c_void_p(4096)
    dev = lambda params=C.byref(p), y=ptr, n_te=8, n_vox=10, packed=ptr, x=ptr, func=ptr, amp=ptr, rmse=ptr, nit=ptr, status=ptr: lib.t2fit_nnls_dev(
        params, y, n_te, n_vox, None, packed, x, func, amp, rmse, nit, status, None)
    for kw in ({"params": None}, {"y": None}, {"packed": None}, {"amp": None}, {"rmse": None}, {"nit": None}, {"status": None}):
        assert dev(**kw) == _abi.E_INVALID and "NULL" in err(), kw
    assert dev(n_te=1) == _abi.E_INVALID and "n_te" in err()
    assert dev(n_te=33) == _abi.E_INVALID and "n_te" in err()
    assert dev(n_vox=-1) == _abi.E_INVALID and "negative" in err()
    assert dev(y=C.c_void_p(4098)) == _abi.E_INVALID and "4 bytes" in err()
    assert dev(x=C.c_void_p(4097)) == _abi.E_INVALID and "4 bytes" in err()
    assert dev(packed=C.c_void_p(4104)) == _abi.E_INVALID and "16 bytes" in err()
    for field, value in (("tol_rel", -1.0), ("tol_rel", float("nan")), ("piv_rel", float("inf")), ("max_iter", -1), ("max_blocks", -2)):
        q = _abi.T2FitNnlsParams()
        lib.t2fit_nnls_params_default(C.byref(q))
        setattr(q, field, value)
        assert dev(params=C.byref(q)) == _abi.E_INVALID and field in err(), field
    assert dev(n_vox=0) == _abi.OK  # a no-op: nothing is read
    # through the statement
    for kw, word in (({"A": np.ones((1, 4))}, "n_te"), ({"A": np.ones((4, 65))}, "n_basis"), ({"A": np.ones((4, 4)), "mu": -1.0}, "mu"),
                     ({"A": np.ones((4, 4)), "W": np.ones((9, 4))}, "n_func"), ({"A": np.full((4, 4), np.nan)}, "non-finite")):
        with pytest.raises(ValueError, match=word):
            N.Basis(**kw)


def test_builders():
    grid = N.log_grid(10.0, 2000.0, 40)
    assert grid[0] == 10.0 and grid[-1] == 2000.0 and np.allclose(np.diff(np.log(grid)), np.log(200.0) / 39)
    A = N.monoexp_basis([80.0, 160.0], grid)
    assert A.shape == (2, 40) and A.dtype == np.float64 and A[1, 3] == np.exp(-160.0 / grid[3])
    W, names = N.window_functionals(grid, {"csf": (1000.0, 2000.0), "all": (0.0, 1e9)})
    assert names == ("csf", "all") and W[1].all() and W[0].sum() == np.count_nonzero(grid >= 1000.0) and set(np.unique(W)) == {0.0, 1.0}
    assert np.array_equal(N.ln_t2_functional(grid), np.log(grid))
    with pytest.raises(ValueError, match="LO <= HI"):
        N.window_functionals(grid, {"bad": (5.0, 1.0)})
    from fetal_t2mapping_amd import _gpu_nnls

    b = _gpu_nnls.spectrum_basis([80.0, 160.0, 240.0], grid, 0.05, {"csf": (1000.0, 2000.0)})
    assert b.names == ("lnT2", "csf") and b.mu == 0.05 and b.n_func == 2 and np.array_equal(b.t2_grid, grid)


def test_launch_shape_comes_from_the_library(lib):
    """The wave count the tests and the benchmark tool name voxel counts from is the kernel's own: asked of the library, and
    here held to the rule it documents (the most waves on a CU's 160 KiB and 32 wave slots, at most 8 per workgroup)."""
    from fetal_t2mapping_amd import _gpu_nnls

    for n in range(2, 65):
        waves, lds, per_cu = _gpu_nnls.workgroup(n)
        assert lds == (n * n + waves * (n * (n + 1) // 2 + 96)) * 8 and 1 <= waves <= _abi.NNLS_MAX_WAVES
        assert per_cu == min(160 * 1024 // lds, 32 // waves) >= 1 and _gpu_nnls.workgroup_waves(n) == waves
        for w in range(1, _abi.NNLS_MAX_WAVES + 1):  # no other workgroup size holds more waves on a CU
            other = (n * n + w * (n * (n + 1) // 2 + 96)) * 8
            assert w * min(160 * 1024 // other, 32 // w) <= waves * per_cu
    assert [_gpu_nnls.workgroup(n) for n in (17, 40, 64)] == [(8, 18248, 4), (8, 71424, 2), (7, 154624, 1)]
    out = (C.c_int(0), C.c_size_t(0), C.c_int(0))
    for n in (1, 65):
        assert lib.t2fit_nnls_workgroup(n, *(C.byref(o) for o in out)) == _abi.E_INVALID and b"n_basis" in lib.t2fit_last_error()
    assert lib.t2fit_nnls_workgroup(40, None, C.byref(out[1]), C.byref(out[2])) == _abi.E_INVALID and b"NULL" in lib.t2fit_last_error()


def test_cli_flags(tmp_path, capsys):
    from fetal_t2mapping_amd import cli as R

    base = ["--path", str(tmp_path), "--csv", "log.csv", "--in_vivo", "--lf", "--sim", "1"]
    args = R.parse_arguments(base + ["--gaussian", "--solver", "nnls", "--nnls_t2", "10:2000:40"])
    assert args.solver == "nnls" and args.dict_args is None
    assert args.nnls_args == {"t2": (10.0, 2000.0, 40), "mu": R.NNLS_DEFAULT_MU, "windows": {}, "write_spectrum": False}
    from fetal_t2mapping_amd import _gpu_nnls

    assert R.NNLS_DEFAULT_MU == _gpu_nnls.DEFAULT_MU
    args = R.parse_arguments(base + ["--gaussian", "--solver", "nnls", "--nnls_t2", "10:2000:64", "--nnls_mu", "0.1", "--nnls_window",
                                     "csf=1000:2000", "--nnls_window", "short=10:40", "--write_spectrum"])
    assert args.nnls_args == {"t2": (10.0, 2000.0, 64), "mu": 0.1, "windows": {"csf": (1000.0, 2000.0), "short": (10.0, 40.0)},
                              "write_spectrum": True}
    b = R.build_spectrum_basis(args.nnls_args, [114.0, 202.0, 299.0])
    assert (b.n_te, b.n_basis, b.mu, b.names) == (3, 64, 0.1, ("lnT2", "csf", "short"))
    assert R.parse_arguments(base + ["--gaussian"]).nnls_args is None
    assert R.parse_arguments(base + ["--gaussian", "--solver", "dict", "--dict_t2", "20:2000:64"]).nnls_args is None
    nnls = ["--gaussian", "--solver", "nnls", "--nnls_t2", "10:2000:40"]
    refused = [
        (["--rician", "--solver", "nnls", "--nnls_t2", "10:2000:40"], "--gaussian only"),
        (["--gaussian_rician", "--solver", "nnls", "--nnls_t2", "10:2000:40"], "--gaussian only"),
        (["--gaussian", "--solver", "nnls"], "needs a T2 grid"),
        (["--gaussian", "--solver", "nnls", "--nnls_t2", "10:2000"], "expected LO:HI:N"),
        (["--gaussian", "--solver", "nnls", "--nnls_t2", "10:2000:65"], "N in 2 .. 64"),
        (["--gaussian", "--solver", "nnls", "--nnls_t2", "10:2000:1"], "N in 2 .. 64"),
        (["--gaussian", "--solver", "nnls", "--nnls_t2", "2000:10:40"], "0 < LO < HI"),
        (nnls + ["--nnls_mu", "-0.1"], "--nnls_mu"),
        (nnls + ["--nnls_mu", "nan"], "--nnls_mu"),
        (nnls + ["--nnls_window", "csf"], "expected NAME=LO:HI"),
        (nnls + ["--nnls_window", "csf=1000"], "expected NAME=LO:HI"),
        (nnls + ["--nnls_window", "c_f=1000:2000"], "letters and digits"),
        (nnls + ["--nnls_window", "lnT2=1000:2000"], "not lnT2"),
        (nnls + ["--nnls_window", "a=10:20", "--nnls_window", "a=30:40"], "given once"),
        (nnls + ["--nnls_window", "a=20:10"], "0 < LO <= HI"),
        (nnls + [v for i in range(8) for v in ("--nnls_window", f"w{i}=10:20")], "7 times at most"),
        (nnls + ["--bootstrap", "8"], "--bootstrap"),
        (nnls + ["--norm"], "--norm"),
        (nnls + ["--gpus", "2"], "--gpus 1"),
        (["--gaussian", "--solver", "lm", "--nnls_t2", "10:2000:40"], "no effect without --solver nnls"),
        (["--gaussian", "--solver", "dict", "--dict_t2", "20:2000:64", "--nnls_mu", "0.1"], "no effect without --solver nnls"),
        (["--gaussian", "--write_spectrum"], "no effect without --solver nnls"),
        (nnls + ["--dict_t2", "20:2000:64"], "no effect without --solver dict"),
    ]
    for extra, word in refused:
        with pytest.raises(SystemExit):
            R.parse_arguments(base + extra)
        assert word in capsys.readouterr().err, extra
    with pytest.raises(ValueError, match="go together"):
        R.process_t2maps(None, str(tmp_path), [114.0], "gaussian", {}, False, True, True, False, False, "1", solver="nnls")
    with pytest.raises(ValueError, match="go together"):
        R.process_t2maps(None, str(tmp_path), [114.0], "gaussian", {}, False, True, True, False, False, "1", solver="lm", spectrum={})


def test_nnls_is_refused_on_a_shared_volume(monkeypatch):
    import pandas as pd

    from fetal_t2mapping_amd import cli as R

    monkeypatch.setattr(R, "_dist_env", lambda: (0, 2, 0))  # two ranks, one subject: the volume would be shared
    md = pd.DataFrame([{"prj": "prj-1", "sub": "sub-1", "ses": "ses-1", "run": "run-01", "EchoTime": 0.114}])
    spec = {"t2": (10.0, 2000.0, 40), "mu": R.NNLS_DEFAULT_MU, "windows": {}, "write_spectrum": False}
    with pytest.raises(ValueError, match="--solver nnls is not run on a volume that is shared by several ranks"):
        R.process_t2maps(md, "/nowhere/", [114], "gaussian", None, False, True, True, False, False, "1", solver="nnls", spectrum=spec)


def test_nifti_series_round_trip(tmp_path):
    """--write_spectrum writes a (T, Z, Y, X) series; volumes keep reading and writing as before."""
    from fetal_t2mapping_amd import nifti

    arr = np.arange(5 * 4 * 3 * 2, dtype=np.float32).reshape(5, 4, 3, 2)
    for name in ("s.nii", "s.nii.gz"):
        path = str(tmp_path / name)
        nifti.WriteImage(nifti.Image(arr, (1.5, 2.0, 2.5), (3.0, -4.0, 5.0)), path)
        with pytest.raises(ValueError, match="expected a 3-D volume"):
            nifti.ReadImage(path)  # the readers of echoes and masks keep refusing a series
        got = nifti.ReadImage(path, series=True)
        assert got.arr.shape == arr.shape and got.arr.tobytes() == arr.tobytes()
        assert np.allclose(got.GetSpacing(), (1.5, 2.0, 2.5)) and np.allclose(got.GetOrigin(), (3.0, -4.0, 5.0))
    path = str(tmp_path / "v.nii.gz")
    nifti.WriteImage(nifti.GetImageFromArray(arr[0]), path)
    assert nifti.ReadImage(path).arr.tobytes() == arr[0].tobytes()
    with pytest.raises(ValueError, match="series"):
        nifti.GetImageFromArray(np.zeros((2, 2)))


def test_abi_is_five_and_the_symbols_are_there(lib):
    import os
    import re

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "t2fit.h")).read()
    assert re.search(r"#define\s+T2FIT_ABI_VERSION\s+5\b", header) and _abi.ABI_VERSION == 5 and lib.t2fit_abi_version() == 5
    assert _abi.NNLS_SYMBOLS == ("t2fit_nnls_params_default", "t2fit_nnls_workgroup", "t2fit_nnls_pack_bytes", "t2fit_nnls_pack_host",
                                 "t2fit_nnls_dev")
    for name in _abi.NNLS_SYMBOLS:
        assert name in header and hasattr(lib, name) and name in _abi.LOOKED_UP
    assert C.sizeof(_abi.T2FitNnlsParams) == 24
    for const in ("MAX_BASIS", "MAX_FUNC", "CHUNK", "MAX_WAVES", "OK", "MAXITER", "BREAKDOWN", "NONFINITE"):
        assert int(re.search(rf"#define\s+T2FIT_NNLS_{const}\s+(\d+)", header).group(1)) == getattr(_abi, "NNLS_" + const)
    assert (N.MAX_BASIS, N.MAX_FUNC, N.ST_MASKED, N.ST_OK, N.ST_MAXITER, N.ST_BREAKDOWN, N.ST_NONFINITE) == (
        _abi.NNLS_MAX_BASIS, _abi.NNLS_MAX_FUNC, _abi.NNLS_MASKED, _abi.NNLS_OK, _abi.NNLS_MAXITER, _abi.NNLS_BREAKDOWN, _abi.NNLS_NONFINITE)
    from fetal_t2mapping_amd import build, t2map

    assert any(src.endswith("t2fit_nnls.hip") for src in build.SOURCES) and t2map.spectrum.solve is not None
