"""The numpy statement of the MP-PCA denoiser (fetal_t2mapping_amd/_mppca.py) against a from-definition reference written
patch by patch with np.linalg.eigh (tests/mppca_cases.py), its parts against hand-written loops, known spectra and values
worked by hand, the edge and mask semantics, every refusal (the statement's and the library's, without a device), the CLI
flags, the ABI, and the benefit on the multi-echo phantom.  tests/test_mppca_gpu.py holds the device to the statement."""
import ctypes as C
import os

import numpy as np
import pytest

import mppca_cases as K
import tvj_cases as T

from fetal_t2mapping_amd import _mppca


@pytest.mark.parametrize("shape,dims,radius,seed", K.REF_CASES, ids=[f"{d}d-r{r}-" + "x".join(map(str, s)) for s, d, r, _ in K.REF_CASES])
def test_statement_against_the_patch_by_patch_reference(shape, dims, radius, seed):
    """Eigenvalues within 1e-12 of the largest, the same rank at every centre (seeds for which no decision is within 1e-9
    of a tie, asserted), the output within 1e-6 max|x|, cnt equal.  sigma^2 is a mean of eigenvalues over N, so it carries
    their bound, 1e-12 lambda_max / N; sigma that bound through the square root plus one float32 rounding."""
    x = K.ref_input(shape, seed)
    for estimator in (2, 1):
        ref = K.ref_case(shape, dims, radius, seed, estimator)
        got = _mppca.mppca_parts(x, radius, dims, estimator)
        assert ref["margin"] > 1e-9, ref["margin"]
        assert got["done"].all() and ref["done"].all()
        assert np.abs(got["eig"] - ref["eig"]).max() <= 1e-12 * ref["eig"].max()
        assert np.array_equal(got["cut"], ref["cut"])
        n_window = (2 * radius + 1) ** dims
        tol = 1e-12 * ref["eig"].max() / n_window
        assert np.abs(got["sigsq"] - ref["sigsq"]).max() <= tol and ref["sigsq"].min() > 0.0
        assert np.array_equal(got["cnt"], ref["cnt"]) and got["cnt"].min() >= 1
        assert got["out"].dtype == np.float32 and np.abs(got["out"] - ref["out"]).max() <= 1e-6 * np.abs(x).max()
        assert np.array_equal(got["rank"], ref["rank"])
        assert got["sigma"].dtype == np.float32
        assert np.all(np.abs(got["sigma"] - ref["sigma"]) <= 2.0 ** -24 * ref["sigma"] + tol / (2.0 * ref["sigma"]))
        assert got["sweeps"].max() < _mppca.MAX_SWEEPS  # every centre converged: off == 0 before the cap
    if shape[0] >= 3:  # (two echoes leave nothing between rank 1 and rank 2 to tell apart)
        kept = shape[0] - ref["cut"]
        assert (kept == 1).any() and (kept == 2).any()


def test_the_device_cases_of_every_echo_count_are_legal_ragged_and_not_degenerate():
    """What tests/test_mppca_gpu.py assumes of mppca_cases.EVERY_M, with the statement alone: every M from 2 to 16 is there,
    the centres fill more than one wave of 64 and end in a ragged one, every centre is processed and keeps a component."""
    assert sorted({c[0] for c in K.EVERY_M}) == list(range(2, K.MAX_TE + 1))
    for case in K.EVERY_M:
        m, nz, ny, nx, dims, r = case
        _mppca.check(case[:4], r, dims, 2)
        centres = (nz - 2 * r if dims == 3 else nz) * (ny - 2 * r) * (nx - 2 * r)
        assert centres > 64 and centres % 64 != 0, case
        for estimator in (2, 1):
            out, sigma, rank = K.gpu_want(case, estimator)
            assert np.isfinite(out).all() and (sigma > 0).all() and 1 <= rank.min() and rank.max() < m, (case, estimator)


def test_ordered_window_sum_against_a_triple_loop_bit_for_bit():
    rng = np.random.default_rng(5)
    a = rng.normal(size=(6, 9, 11)) * 10.0 ** rng.integers(-8, 8, size=(6, 9, 11))  # (rounding differs with the order)
    for dims in (2, 3):
        for r in (1, 2):
            got = _mppca.window_sum(a, r, dims)
            want = K.loop_window_sum(a, r, dims)
            assert got.shape == want.shape and got.tobytes() == want.tobytes()
            assert _mppca.window_sum(a[::-1, ::-1, ::-1], r, dims)[::-1, ::-1, ::-1].tobytes() != want.tobytes()
    g = _mppca.gram(np.stack([a, 2.0 * a]).astype(np.float32), 1, 3)
    a32 = a.astype(np.float32).astype(np.float64)
    assert g[..., 0, 1].tobytes() == K.loop_window_sum(a32 * (2.0 * a32), 1, 3).tobytes()
    assert g[..., 0, 1].tobytes() == g[..., 1, 0].tobytes()


def test_jacobi_on_known_spectra_the_sweep_cap_and_the_negligible_pair_rule():
    rng = np.random.default_rng(9)
    q, _ = np.linalg.qr(rng.normal(size=(4, 4)))
    u = rng.normal(size=5)
    batch4 = np.stack([np.diag([3.0, -1.0, 7.0, 0.5]),          # diagonal: no sweep
                       np.zeros((4, 4)),                        # zero: no sweep
                       q @ np.diag([2.0, 2.0, 5.0, 5.0]) @ q.T,  # repeated eigenvalues
                       q @ np.diag([1e-8, 1.0, 1e8, 1e12]) @ q.T])
    batch4 = (batch4 + batch4.transpose(0, 2, 1)) / 2.0
    w, v, sweeps = _mppca.jacobi(batch4)
    assert sweeps[0] == 0 and sweeps[1] == 0 and 1 <= sweeps[2] < 16 and 1 <= sweeps[3] < 16
    assert w[0].tolist() == [3.0, -1.0, 7.0, 0.5] and np.array_equal(v[0], np.eye(4))
    assert not w[1].any() and np.array_equal(v[1], np.eye(4))
    assert np.allclose(np.sort(w[2]), [2.0, 2.0, 5.0, 5.0], rtol=1e-14, atol=0.0)
    assert np.allclose(np.sort(w[3]), np.linalg.eigvalsh(batch4[3]), rtol=0.0, atol=1e-15 * 1e12)
    for i in range(4):  # V is orthogonal and diagonalises: V^T G V = diag(w)
        assert np.abs(v[i].T @ v[i] - np.eye(4)).max() < 1e-14
        assert np.abs(v[i].T @ batch4[i] @ v[i] - np.diag(w[i])).max() <= 1e-14 * max(np.abs(w[i]).max(), 1.0)
    # rank 1: one eigenvalue |u|^2, the others 0 to rounding
    w1, v1, s1 = _mppca.jacobi(np.outer(u, u)[None])
    assert np.isclose(w1[0].max(), u @ u, rtol=1e-14) and np.sort(np.abs(w1[0]))[:4].max() <= 1e-15 * (u @ u) and s1[0] < 16
    # the sweep cap: one sweep does not diagonalise a full matrix, and is counted
    wc, vc, sc = _mppca.jacobi(batch4[2:3], max_sweeps=1)
    assert sc[0] == 1 and np.abs(vc[0].T @ batch4[2] @ vc[0] - np.diag(wc[0])).max() > 1e-8
    # the negligible-pair rule: an off-diagonal that cannot change either diagonal entry is set to zero without a rotation,
    # and the next sweep's off == 0 stops the matrix; an off-diagonal whose square underflows stops it at once
    tiny = np.array([[[1.0, 1e-20], [1e-20, 1.0]], [[1e300, 1e-300], [1e-300, 1.0]]])
    wt, vt, st = _mppca.jacobi(tiny)
    assert st.tolist() == [1, 0] and np.array_equal(vt[0], np.eye(2)) and wt.tolist() == [[1.0, 1.0], [1e300, 1.0]]
    # order: ascending, ties by index
    assert _mppca.order(np.array([[2.0, 1.0, 2.0, 0.0]])).tolist() == [[2, 1, 3, 0]]


def test_both_estimators_against_values_worked_by_hand_on_a_3_x_27_case():
    """M = 3, N = 27 (dims 3, radius 1), eigenvalues 27 (1, 3.45, 100), q = 27, lam_r = 1.
    Estimator 2: p = 0: a = 1, b = 0, so cut = 1.  p = 1: gamma = 2 / 26, a = 4.45 / 2 = 2.225,
    b = 2.45 / (4 sqrt(1 / 13)) = 2.2084 < a, so cut = 2 and sigma^2 = 2.225.  p = 2: gamma = 3 / 27, a = 104.45 / 3 = 34.82,
    b = 99 / (4 / 3) = 74.25: no.  Rank 1.
    Estimator 1: p = 1: gamma = 2 / 27, b = 2.45 / (4 sqrt(2 / 27)) = 2.2505 > 2.225: no, so cut = 1, sigma^2 = 1.  Rank 2."""
    s = 27.0 * np.array([[1.0, 3.45, 100.0]])
    cut2, sig2 = _mppca.rank_sigma(s, 27, 2)
    cut1, sig1 = _mppca.rank_sigma(s, 27, 1)
    assert cut2.tolist() == [2] and np.isclose(sig2[0], 2.225, rtol=1e-15)
    assert cut1.tolist() == [1] and np.isclose(sig1[0], 1.0, rtol=1e-15)
    # the same spectrum as a 3 x 3 x 3 window of three echoes, through the whole statement (float32 samples: 1e-7 off)
    rng = np.random.default_rng(2)
    u, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    wmat, _ = np.linalg.qr(rng.normal(size=(27, 3)))
    x = (u @ np.diag(np.sqrt(s[0])) @ wmat.T).astype(np.float32).reshape(3, 3, 3, 3)
    for estimator, cut, sigsq in ((2, 2, 2.225), (1, 1, 1.0)):
        parts = _mppca.mppca_parts(x, 1, 3, estimator)
        assert parts["cut"].tolist() == [[[cut]]] and np.isclose(parts["sigsq"][0, 0, 0], sigsq, rtol=1e-5)
        assert np.allclose(parts["eig"][0, 0, 0], s[0], rtol=1e-5)
        assert np.all(parts["rank"] == 3 - cut) and np.all(parts["sigma"] == np.float32(np.sqrt(parts["sigsq"][0, 0, 0])))
        assert np.all(parts["cnt"] == 1)
        # one centre: the output is the projection of every voxel's decay onto the kept eigenvectors
        w, v = np.linalg.eigh(parts["G"][0, 0, 0])
        proj = v[:, cut:] @ v[:, cut:].T
        want = np.tensordot(proj, x.astype(np.float64), axes=(1, 0))
        assert np.abs(parts["out"] - want).max() <= 1e-6 * np.abs(x).max()


def test_edges_masks_and_one_nan():
    shape, r = (4, 2, 12, 13), 2
    x = K.ref_input(shape, 21)
    full = _mppca.mppca_parts(x, r, 2)
    # sigma and rank of a rim voxel are those of the nearest centre
    assert full["sigma"][0, 0, 0] == full["sigma"][0, r, r] and full["rank"][1, 11, 12] == full["rank"][1, 11 - r, 12 - r]
    assert full["sigma"][0, 5, 0] == full["sigma"][0, 5, r] and full["sigma"][0, 5, 1] == full["sigma"][0, 5, r]
    assert full["cnt"][0, 0, 0] == 1 and full["cnt"][0, 6, 6] == 25 and full["cnt"][0, 0, 6] == 5
    # an empty mask: no centre is processed, cnt = 0 everywhere, the input comes back byte for byte
    none = _mppca.mppca_parts(x, r, 2, mask=np.zeros(shape[1:], np.uint8))
    assert none["out"].tobytes() == x.tobytes() and not none["cnt"].any() and not none["sigma"].any() and not none["rank"].any()
    # one centre in the mask: its window is projected, every other voxel keeps its samples
    one = np.zeros(shape[1:], np.uint8)
    one[1, 5, 6] = 1
    got = _mppca.mppca_parts(x, r, 2, mask=one)
    inside = np.zeros(shape[1:], bool)
    inside[1, 3:8, 4:9] = True
    assert np.array_equal(got["cnt"] == 1, inside) and got["out"][:, ~inside].tobytes() == x[:, ~inside].tobytes()
    assert (got["out"][:, inside] != x[:, inside]).any() and got["done"].sum() == 1
    assert got["sigma"][1, 5, 6] == full["sigma"][1, 5, 6] and np.count_nonzero(got["sigma"]) == 1
    # an unprocessed centre contributes nothing: the mask with holes against the reference run with the same mask
    holes = K.holes_mask(shape[1:])
    got = _mppca.mppca_parts(x, r, 2, mask=holes)
    ref = K.ref_mppca(x, r, 2, mask=holes)
    assert np.array_equal(got["done"], ref["done"]) and 0 < got["done"].sum() < got["done"].size
    assert np.array_equal(got["cnt"], ref["cnt"]) and (got["cnt"] == 0).any()
    assert np.abs(got["out"] - ref["out"]).max() <= 1e-6 * np.abs(x).max()
    assert np.array_equal(got["rank"], ref["rank"]) and not got["P"][~got["done"]].any()
    assert got["out"][:, got["cnt"] == 0].tobytes() == x[:, got["cnt"] == 0].tobytes()
    # one NaN unprocesses exactly the centres whose window holds it and changes nothing farther than 2 r away
    for dims, at in ((2, (1, 6, 7)), (3, (2, 6, 7))):
        shape3 = (3, 5, 12, 13)
        y = np.array(K.ref_input(shape3, 22))
        clean = _mppca.mppca_parts(y, 1, dims)
        y[1][at] = np.nan
        bad = _mppca.mppca_parts(y, 1, dims)
        zz, yy, xx = np.meshgrid(*[np.arange(n) for n in shape3[1:]], indexing="ij")
        dist = np.maximum(np.abs(yy - at[1]), np.abs(xx - at[2]))
        dist = np.maximum(dist, np.abs(zz - at[0])) if dims == 3 else np.where(zz == at[0], dist, 99)
        rz = 1 if dims == 3 else 0
        holds = (dist <= 1)[rz:shape3[1] - rz, 1:-1, 1:-1]
        assert np.array_equal(~bad["done"], holds) and clean["done"].all()
        far = dist > 2
        assert bad["out"][:, far].tobytes() == clean["out"][:, far].tobytes()
        assert bad["sigsq"][~holds].tobytes() == clean["sigsq"][~holds].tobytes() and not bad["sigsq"][holds].any()
        assert np.array_equal(bad["cut"][~holds], clean["cut"][~holds]) and not bad["P"][holds].any()
        assert bad["sigma"][at] == 0.0 and bad["rank"][at] == 0 and clean["sigma"][at] > 0.0
        assert bad["cnt"][at] == 0 and np.isnan(bad["out"][1][at]) and bad["out"][0][at] == y[0][at]
        near = (dist <= 2) & (dist > 0)
        assert np.isfinite(bad["out"][:, near]).all() and (bad["cnt"][near] < clean["cnt"][near]).all()


def test_the_statement_refuses_what_the_library_refuses():
    ok = np.zeros((3, 3, 5, 5), np.float32)
    _mppca.check(ok.shape, 1, 2, 2)
    for shape, radius, dims, estimator, word in (((3, 3, 5, 5), 0, 2, 2, "radius"), ((3, 3, 5, 5), 5, 2, 2, "radius"),
                                                 ((3, 3, 5, 5), 1, 1, 2, "dims"), ((3, 3, 5, 5), 1, 4, 2, "dims"),
                                                 ((3, 3, 5, 5), 1, 2, 0, "estimator"), ((3, 3, 5, 5), 1, 2, 3, "estimator"),
                                                 ((1, 3, 5, 5), 1, 2, 2, "echoes"), ((17, 3, 9, 9), 2, 2, 2, "echoes"),
                                                 ((9, 3, 5, 5), 1, 2, 2, "more voxels"), ((10, 3, 5, 5), 1, 2, 2, "more voxels"),
                                                 ((3, 3, 5, 4), 2, 2, 2, "at least 5"), ((3, 3, 2, 5), 1, 2, 2, "at least 3"),
                                                 ((3, 2, 5, 5), 1, 3, 2, "at least 3"), ((3, 5, 5), 1, 2, 2, "(M, Z, Y, X)")):
        with pytest.raises(ValueError, match=word.replace("(", r"\(").replace(")", r"\)")):
            _mppca.check(shape, radius, dims, estimator)
    with pytest.raises(ValueError, match="mask shape"):
        _mppca.mppca(ok, 1, 2, 2, mask=np.ones((3, 5, 4), np.uint8))


def test_header_abi_and_library_agree_and_every_refusal_leaves_the_device_alone():
    from fetal_t2mapping_amd import _abi, build

    names = [s[0] for s in _abi.SYMBOLS]
    header = open(os.path.join(os.path.dirname(build.PKG), "include", "t2fit.h")).read()
    assert _abi.ABI_VERSION == 5 and "#define T2FIT_ABI_VERSION 5" in header
    assert _abi.MPPCA_SYMBOLS == ("t2fit_mppca_params_default", "t2fit_mppca_workspace_bytes", "t2fit_mppca_dev")
    for sym in _abi.MPPCA_SYMBOLS:
        assert sym in names and sym + "(" in header and sym in _abi.LOOKED_UP
    assert f"#define T2FIT_MPPCA_MAX_TE {_abi.MPPCA_MAX_TE}" in header and _abi.MPPCA_MAX_TE == K.MAX_TE == _mppca.MAX_TE == 16
    assert f"#define T2FIT_MPPCA_MAX_RADIUS {_abi.MPPCA_MAX_RADIUS}" in header and _abi.MPPCA_MAX_RADIUS == _mppca.MAX_RADIUS
    assert "typedef struct t2fit_mppca_params" in header and C.sizeof(_abi.T2FitMppcaParams) == 16
    assert "t2fit_mppca.hip" in [os.path.basename(s) for s in build.SOURCES]
    import torch  # noqa: F401  (one HIP runtime per process: see _lib.load)

    lib = _abi.bind(C.CDLL(build.build()))
    assert lib.t2fit_abi_version() == 5
    par = _abi.T2FitMppcaParams(9, 9, 9, 9)
    assert lib.t2fit_mppca_params_default(C.byref(par)) == _abi.OK
    assert (par.radius, par.dims, par.estimator, par.flags) == (2, 2, 2, 0)
    assert lib.t2fit_mppca_params_default(None) == _abi.E_INVALID

    up = lambda v: (v + 255) // 256 * 256  # noqa: E731
    need = C.c_size_t()
    for dims in (2, 3):
        for radius in (1, 2, 4):
            for m, nz, ny, nx in ((8, 256, 256, 256), (6, 9, 37, 70), (2, 9, 9, 9), (8, 11, 10, 9)):
                par.radius, par.dims = radius, dims
                centres = (nz - 2 * radius if dims == 3 else nz) * (ny - 2 * radius) * (nx - 2 * radius)
                assert lib.t2fit_mppca_workspace_bytes(C.byref(par), m, nz, ny, nx, C.byref(need)) == _abi.OK
                assert need.value == up(8 * (m * (m + 1) // 2) * centres) + up(centres), (dims, radius, m, nz, ny, nx)
    assert lib.t2fit_mppca_params_default(C.byref(par)) == _abi.OK
    assert lib.t2fit_mppca_workspace_bytes(C.byref(par), 3, 4, 8, 8, None) == _abi.E_INVALID

    p = 4096  # never dereferenced: every call below is refused first
    ok_size = (3, 3, 8, 8)
    assert lib.t2fit_mppca_workspace_bytes(C.byref(par), *ok_size, C.byref(need)) == _abi.OK

    def refused(fragment, par=par, src=p, mask=None, dst=p, sigma=p, rank=p, size=ok_size, ws=p, ws_bytes=None):
        rc = lib.t2fit_mppca_dev(C.byref(par) if par is not None else None, src, mask, dst, sigma, rank, *size, ws,
                                 need.value if ws_bytes is None else ws_bytes, None)
        msg = lib.t2fit_last_error().decode()
        assert rc == _abi.E_INVALID and fragment in msg and "t2fit_mppca_dev" in msg, (fragment, rc, msg)

    refused("in_dev is NULL", src=None)
    refused("nothing to compute", dst=None, sigma=None, rank=None)
    refused("params is NULL", par=None)
    refused("workspace_dev is NULL", ws=None)
    refused("workspace too small", ws_bytes=need.value - 1)
    refused("workspace too small", ws_bytes=0)
    refused("not aligned to 256", ws=p + 64)
    refused("not aligned to 4", src=p + 2)
    refused("not aligned to 4", dst=p + 1)
    refused("not aligned to 4", sigma=p + 3)
    for size in ((3, 0, 8, 8), (3, 3, -1, 8), (3, 3, 8, 0)):
        refused(">= 1", size=size)
    for size in ((1, 3, 8, 8), (0, 3, 8, 8), (-3, 3, 8, 8), (K.MAX_TE + 1, 3, 8, 8), (2 ** 31 - 1, 3, 8, 8)):
        refused("T2FIT_MPPCA_MAX_TE", size=size)
    refused("at least 2 radius + 1 = 5", size=(3, 3, 4, 8))
    refused("at least 2 radius + 1 = 5", size=(3, 3, 8, 4))

    def with_(**kw):
        q = _abi.T2FitMppcaParams()
        lib.t2fit_mppca_params_default(C.byref(q))
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    refused("more voxels than there are echoes", par=with_(radius=1), size=(9, 3, 8, 8))
    refused("more voxels than there are echoes", par=with_(radius=1), size=(K.MAX_TE, 3, 8, 8))
    refused("at least 2 radius + 1 = 3", par=with_(radius=1, dims=3), size=(3, 2, 8, 8))
    for kw, fragment in (({"radius": 0}, "radius"), ({"radius": 5}, "radius"), ({"radius": -1}, "radius"), ({"dims": 1}, "dims"),
                         ({"dims": 4}, "dims"), ({"estimator": 0}, "estimator"), ({"estimator": 3}, "estimator"),
                         ({"flags": 1}, "flags")):
        refused(fragment, par=with_(**kw))
        assert lib.t2fit_mppca_workspace_bytes(C.byref(with_(**kw)), *ok_size, C.byref(need)) == _abi.E_INVALID
    for size in ((1, 3, 8, 8), (K.MAX_TE + 1, 3, 8, 8), (3, 3, 4, 8), (3, 0, 8, 8)):
        assert lib.t2fit_mppca_workspace_bytes(C.byref(par), *size, C.byref(need)) == _abi.E_INVALID


def test_flags(capsys):
    import inspect

    from fetal_t2mapping_amd import cli as R

    base = ["--path", "/x", "--csv", "a.csv", "--in_vivo", "--gaussian", "--lf", "--sim", "1"]
    parse = lambda extra: R.parse_arguments(base + extra)  # noqa: E731
    # every existing argv parses as before
    old = {"weight": ("abs", 0.1), "dims": 2, "eps": 2e-4, "max_iter": 200}
    plain = parse([])
    assert plain.denoise_args is None and plain.noise_map_args is None and plain.bootstrap_noise == "background"
    assert not plain.write_noise_map and plain.denoise_sigma == "background" and plain.denoise_patch == 2
    for extra, want in ((["--denoise", "tv"], old), (["--denoise", "tv_joint"], {**old, "joint": True}),
                        (["--denoise", "tv", "--denoise_weight", "2.4sigma", "--denoise_dims", "3", "--denoise_eps", "0",
                          "--denoise_iter", "50"], {"weight": ("sigma", 2.4), "dims": 3, "eps": 0.0, "max_iter": 50})):
        a = parse(extra)
        assert a.denoise_args == want and a.noise_map_args is None, extra
    a = R.parse_arguments(["--path", "/x", "--csv", "a.csv", "--in_vivo", "--gaussian_rician", "--lf", "--sim", "1", "--bootstrap", "10",
                           "--bootstrap_noise", "sigma_map"])
    assert a.bootstrap_noise == "sigma_map" and a.noise_map_args is None
    assert parse(["--bootstrap", "10", "--bootstrap_noise", "12.5"]).bootstrap_noise == 12.5
    assert parse(["--bootstrap", "10"]).noise_map_args is None
    # the new flags
    assert parse(["--denoise", "mppca"]).denoise_args == {"method": "mppca", "radius": 2, "dims": 2}
    a = parse(["--denoise", "mppca", "--denoise_patch", "1", "--denoise_dims", "3", "--write_noise_map"])
    assert a.denoise_args == {"method": "mppca", "radius": 1, "dims": 3}
    assert a.noise_map_args == {"radius": 1, "dims": 3, "write": True}
    assert parse(["--write_noise_map", "--denoise_patch", "3"]).noise_map_args == {"radius": 3, "dims": 2, "write": True}
    assert parse(["--write_noise_map"]).denoise_args is None
    a = parse(["--bootstrap", "10", "--bootstrap_noise", "mppca", "--denoise_dims", "3"])
    assert a.bootstrap_noise == "mppca" and a.noise_map_args == {"radius": 2, "dims": 3} and a.denoise_args is None
    a = parse(["--denoise", "tv_joint", "--denoise_weight", "2sigma", "--denoise_sigma", "mppca", "--denoise_patch", "3"])
    assert a.denoise_args == {"weight": ("sigma", 2.0), "dims": 2, "eps": 2e-4, "max_iter": 200, "joint": True,
                              "sigma_from": "mppca", "radius": 3}
    assert parse(["--denoise", "tv", "--denoise_weight", "2sigma", "--denoise_sigma", "background"]).denoise_args == \
        {**old, "weight": ("sigma", 2.0)}
    # their refusals
    for extra, word in ((["--denoise", "mppca", "--denoise_weight", "1sigma"], "--denoise_weight belongs to"),
                        (["--denoise", "mppca", "--denoise_eps", "0"], "--denoise_eps belongs to"),
                        (["--denoise", "mppca", "--denoise_iter", "5"], "--denoise_iter belongs to"),
                        (["--denoise", "mppca", "--denoise_sigma", "mppca"], "--denoise_sigma belongs to"),
                        (["--denoise", "mppca", "--bootstrap", "10"], "--bootstrap"),
                        (["--denoise", "mppca", "--denoise_patch", "0"], "1..4"),
                        (["--denoise", "mppca", "--denoise_patch", "5"], "1..4"),
                        (["--denoise_patch", "2"], "MP-PCA window"),
                        (["--denoise", "tv", "--denoise_patch", "2"], "MP-PCA window"),
                        (["--denoise_dims", "3"], "no effect without --denoise"),
                        (["--denoise_sigma", "mppca"], "no effect without --denoise"),
                        (["--denoise", "tv", "--denoise_sigma", "mppca"], "<c>sigma"),
                        (["--denoise", "tv", "--denoise_sigma", "median"], "invalid choice"),
                        (["--bootstrap", "10", "--bootstrap_noise", "pca"], "'mppca' or a number")):
        with pytest.raises(SystemExit):
            parse(extra)
        assert word in " ".join(capsys.readouterr().err.split()), extra
    assert R.parse_bootstrap_noise("mppca") == "mppca"
    with pytest.raises(SystemExit):
        parse(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--denoise_patch" in text and "--write_noise_map" in text and "Rician floor" in " ".join(R.__doc__.split())
    sig = inspect.signature(R.denoise_subject).parameters
    assert sig["method"].default == "tv" and sig["sigma_from"].default == "background" and sig["joint"].default is False
    assert inspect.signature(R.process_t2maps).parameters["noise_map"].default is None


def test_mppca_halves_the_t2_error_of_the_phantom_and_finds_its_noise_level():
    """The 64 x 64 multi-echo phantom of tvj_cases (6 echoes, Rician sigma 25, seed 0), dims 2, radius 2, T2 from an
    unweighted log-linear fit.  Measured with this statement: T2 RMSE 13.08 ms against 24.50 ms without denoising, a ratio
    of 0.534 (the bound is that ratio plus 0.03); median sigma over the centres 23.76 = 0.950 x 25 (the Rician floor of the
    late echoes biases it low; the bound is 0.90 .. 1.02); mean rank 1.28."""
    noisy, _ = T.phantom()
    parts = _mppca.mppca_parts(noisy[:, None], 2, 2, 2)
    none, rmse = T.t2_rmse(noisy), T.t2_rmse(parts["out"][:, 0])
    sigma = float(np.median(np.sqrt(parts["sigsq"])))
    rank = float((noisy.shape[0] - parts["cut"]).mean())
    print(f"T2 RMSE (ms): none {none:.2f}, MP-PCA {rmse:.2f}, ratio {rmse / none:.3f}; median sigma {sigma:.2f}; mean rank {rank:.2f}")
    assert parts["done"].all()
    assert rmse / none < 0.534 + 0.03
    assert 0.90 <= sigma / T.PH_SIGMA <= 1.02
    assert 1.0 <= rank <= 2.0
