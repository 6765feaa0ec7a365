"""Host side of the orthogonal-stack reconstruction (no device): the numpy statement of the definition
(fetal_t2mapping_amd/_resample.py) against properties that pin it independently of any implementation, the two facts
about the reference's merge that can be pinned to its own scipy / numpy calls, the ABI of the built library (version
still 5, three additive entry points, every argument check refused with a message before HIP is touched), and the flags
of recon.py and cli.py --reconstruct.  tests/test_recon_gpu.py runs the kernels."""
import ctypes as C
import os

import numpy as np
import pytest

from fetal_t2mapping_amd import _resample as R


def _vol(shape, seed=0):
    return np.random.default_rng(seed).normal(500.0, 200.0, size=shape).astype(np.float32)


def _rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    m = {0: [[1, 0, 0], [0, c, -s], [0, s, c]], 1: [[c, 0, s], [0, 1, 0], [-s, 0, c]], 2: [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis]
    return np.array(m, np.float64)


def test_resample_onto_the_own_geometry_is_the_identity_bit_for_bit():
    v = _vol((7, 9, 11))
    v[3, 4, 5] = np.inf  # a node next to an Inf must not become NaN
    for direction in (np.eye(3), np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0.0]]), np.array([[0, -1, 0], [0, 0, -1], [1, 0, 0.0]])):
        g = R.Geometry((11, 9, 7), (0.8, 1.0, 4.5), (3.3, -2.1, 7.7), direction.ravel())
        A = R.index_affine(g, g)
        assert np.array_equal(A, np.hstack([np.eye(3), np.zeros((3, 1))]))
        assert np.array_equal(R.resample(v, A, v.shape), v)
        assert np.array_equal(R.resample(v, A, v.shape, "nearest"), v)
    stack = np.stack([v, v + 1])
    assert np.array_equal(R.resample(stack, A, v.shape), stack)


def test_interior_agrees_with_scipy_map_coordinates():
    from scipy.ndimage import map_coordinates

    v = _vol((12, 14, 16), 1)
    src = R.Geometry((16, 14, 12), (1.0, 1.2, 3.0), (1.0, 2.0, 3.0), (_rot(2, 10.0) @ _rot(0, -7.0)).ravel())
    dst = R.Geometry((20, 18, 30), (0.7, 0.7, 1.1), (3.0, 3.5, 6.0), _rot(1, 4.0).ravel())
    A = R.index_affine(dst, src)
    got = R.resample(v, A, dst.shape)
    c = R._coords(A, dst.shape)
    interior = np.ones(dst.shape, bool)
    for k, n in enumerate((16, 14, 12)):
        interior &= (c[k] >= 0) & (c[k] <= n - 1)
    assert interior.sum() > 500
    want = map_coordinates(v.astype(np.float64), [c[2][interior], c[1][interior], c[0][interior]], order=1)
    assert np.allclose(got[interior], want.astype(np.float32), rtol=1e-6, atol=0)
    # the float64 value before the rounding, restated without the zero-weight rule, to 1e-12
    b = [np.floor(c[k][interior]).astype(int) for k in range(3)]
    d = [c[k][interior] - b[k] for k in range(3)]
    v64 = v.astype(np.float64)
    hi = [np.minimum(b[k] + 1, n - 1) for k, n in enumerate((16, 14, 12))]
    x00 = v64[b[2], b[1], b[0]] * (1 - d[0]) + v64[b[2], b[1], hi[0]] * d[0]
    x01 = v64[b[2], hi[1], b[0]] * (1 - d[0]) + v64[b[2], hi[1], hi[0]] * d[0]
    x10 = v64[hi[2], b[1], b[0]] * (1 - d[0]) + v64[hi[2], b[1], hi[0]] * d[0]
    x11 = v64[hi[2], hi[1], b[0]] * (1 - d[0]) + v64[hi[2], hi[1], hi[0]] * d[0]
    tri = (x00 * (1 - d[1]) + x01 * d[1]) * (1 - d[2]) + (x10 * (1 - d[1]) + x11 * d[1]) * d[2]
    assert np.allclose(want, tri, rtol=1e-12, atol=1e-9)
    assert np.allclose(got[interior].astype(np.float64), tri, rtol=2e-7)


def test_outside_is_default_and_the_rim_replicates_the_edge():
    v = _vol((4, 5, 6), 2)
    A = np.hstack([np.eye(3), np.zeros((3, 1))])
    A[0, 3] = -0.75  # c_x = ix - 0.75
    out = R.resample(v, A, v.shape, default=-7.0)
    assert np.all(out[:, :, 0] == -7.0)  # c_x = -0.75 < -0.5
    A[0, 3] = -0.25
    out = R.resample(v, A, v.shape, default=-7.0)
    assert np.array_equal(out[:, :, 0], v[:, :, 0])  # c_x = -0.25: on the rim, the edge value
    A[0, 3] = 0.25
    out = R.resample(v, A, v.shape, default=-7.0)
    assert np.array_equal(out[:, :, 5], v[:, :, 5])  # c_x = 5.25 < 5.5: the upper rim
    A[0, 3] = 0.5
    assert np.all(R.resample(v, A, v.shape, default=-7.0)[:, :, 5] == -7.0)  # c_x = 5.5 is outside (half-open)
    assert np.all(R.resample(v, A, v.shape, "nearest", default=-7.0)[:, :, 5] == -7.0)


def test_isotropic_geometry_rounds_halves_to_even():
    g = R.Geometry((10, 7, 5), (1.25, 1.5, 4.5), (1.0, 2.0, 3.0))
    h = R.isotropic_geometry(g, 1.0)
    # 12.5 -> 12, 10.5 -> 10, 22.5 -> 22: Python's round, not floor(x + .5)
    assert h.GetSize() == (12, 10, 22) and h.GetSpacing() == (1.0, 1.0, 1.0)
    assert h.GetOrigin() == g.GetOrigin() and h.GetDirection() == g.GetDirection()
    assert R.isotropic_geometry(R.Geometry((3, 3, 3), (1.5, 2.5, 3.5)), 1.0).GetSize() == (4, 8, 10)
    with pytest.raises(ValueError):
        R.isotropic_geometry(R.Geometry((1, 1, 1), (0.2, 1, 1)), 1.0)


def test_nearest_on_an_int32_label_volume():
    lab = np.random.default_rng(3).integers(0, 9, size=(5, 6, 7)).astype(np.int32)
    g = R.Geometry((7, 6, 5), (2.0, 2.0, 2.0))
    h = R.isotropic_geometry(g, 1.0)
    out = R.resample(lab, R.index_affine(h, g), h.shape, "nearest", default=-1)
    assert out.dtype == np.int32 and out.shape == (10, 12, 14)
    # c = i / 2: floor(c + .5) takes 0, 1, 1, 2, 2, ... (a tie goes up); the last index (c = n - .5) is outside
    idx = lambda n: np.minimum(np.floor(np.arange(2 * n) / 2 + 0.5).astype(int), n - 1)
    want = lab[np.ix_(idx(5), idx(6), idx(7))]
    want[-1], want[:, -1], want[:, :, -1] = -1, -1, -1
    assert np.array_equal(out, want)
    with pytest.raises(ValueError):
        R.resample(lab.astype(np.int16), np.eye(3, 4), lab.shape, "nearest")


def test_integer_cast_truncates_toward_zero_and_clamps():
    v = np.array([[[-3.0, 4.0, 40000.0, -40000.0, 1.0]]], np.float32)
    A = np.hstack([np.eye(3), np.zeros((3, 1))])
    A[0, 3] = 0.25  # between neighbours: -1.25, 10003, 20000, -29999.75
    plain = R.resample(v, A, v.shape)
    cast = R.resample(v, A, v.shape, integer_cast=True)
    assert np.array_equal(plain[0, 0, :4], np.float32([-1.25, 10003.0, 20000.0, -29999.75]))
    assert np.array_equal(cast[0, 0, :4], np.float32([-1.0, 10003.0, 20000.0, -29999.0]))
    A[0, 3] = 0.0
    assert np.array_equal(R.resample(v, A, v.shape, integer_cast=True)[0, 0], np.float32([-3, 4, 32767, -32768, 1]))


def test_the_reference_merge_is_the_mean_of_three_arrays_in_a_fixed_order():
    """reconstruct_vol_trilinear (utils/qmri_utils.py:82-136): RegularGridInterpolator over the fixed grid's own linspace
    nodes returns each volume unchanged, and np.mean over the list is ((a + b) + c) / 3."""
    from scipy.interpolate import RegularGridInterpolator

    rng = np.random.default_rng(4)
    shape = (17, 23, 19)
    origin, spacing = (-101.37, 55.2, 7.05), (1.0, 1.0, 1.0)
    z = np.linspace(origin[2], origin[2] + spacing[2] * (shape[0] - 1), shape[0])
    y = np.linspace(origin[1], origin[1] + spacing[1] * (shape[1] - 1), shape[1])
    x = np.linspace(origin[0], origin[0] + spacing[0] * (shape[2] - 1), shape[2])
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    points = np.array([Z.ravel(), Y.ravel(), X.ravel()]).T
    vols = [rng.normal(500, 300, size=shape) for _ in range(3)]
    interpolated = [RegularGridInterpolator((z, y, x), v, method="linear")(points) for v in vols]
    for v, got in zip(vols, interpolated):
        assert np.array_equal(got.reshape(shape), v)
    mean = np.mean(interpolated, axis=0).reshape(shape)
    assert np.array_equal(mean, ((vols[0] + vols[1]) + vols[2]) / 3)
    assert np.array_equal(R.merge(*[v.astype(np.float32) for v in vols]),
                          np.mean([v.astype(np.float32).astype(np.float64) for v in vols], axis=0).astype(np.float32))


def test_index_affine_composed_two_ways_with_oblique_directions_and_a_rigid_transform():
    src = R.Geometry((16, 14, 12), (0.9, 1.1, 4.5), (-80.0, 13.0, 40.5), (_rot(2, 12.0) @ _rot(0, -8.0)).ravel())
    dst = R.Geometry((30, 28, 26), (1.0, 1.0, 1.0), (-75.0, 10.0, 42.0), (_rot(1, 5.0) @ _rot(2, -3.0)).ravel())
    T = np.eye(4)
    T[:3, :3] = _rot(0, 4.0) @ _rot(1, -2.0)
    T[:3, 3] = (1.5, -2.25, 0.75)
    A = R.index_affine(dst, src, T)
    rng = np.random.default_rng(5)
    idx = rng.integers(0, 26, size=(200, 3)).astype(np.float64)
    Dd, Ds = np.array(dst.GetDirection()).reshape(3, 3), np.array(src.GetDirection()).reshape(3, 3)
    for i in idx:
        p = np.array(dst.GetOrigin()) + Dd @ (np.array(dst.GetSpacing()) * i)
        q = T[:3, :3] @ p + T[:3, 3]
        c = (Ds.T @ (q - np.array(src.GetOrigin()))) / np.array(src.GetSpacing())  # D orthonormal: D^-1 = D^T
        assert np.allclose(A[:, :3] @ i + A[:, 3], c, rtol=1e-12, atol=1e-10)
    assert np.allclose(R.index_affine(dst, src, np.eye(4)), R.index_affine(dst, src), rtol=1e-14, atol=1e-12)
    with pytest.raises(ValueError):
        R.index_affine(dst, src, np.eye(3))


def _stacks(n_vol=2, seed=6):
    """Three thick-slice stacks of the same 24 mm cube: ax thick along z, cor along y, sag along x (axis-aligned, the
    direction matrices permute the axes as the scanner's do)."""
    rng = np.random.default_rng(seed)
    geoms = {
        "ax": R.Geometry((24, 24, 6), (1.0, 1.0, 4.0), (-12.0, -12.0, -10.5)),
        "cor": R.Geometry((24, 24, 6), (1.0, 1.0, 4.0), (-12.0, -10.5, -12.0), (1, 0, 0, 0, 0, 1, 0, 1, 0)),
        "sag": R.Geometry((24, 24, 6), (1.0, 1.0, 4.0), (-10.5, -12.0, -12.0), (0, 0, 1, 1, 0, 0, 0, 1, 0)),
    }
    stacks = {o: rng.normal(600, 150, size=(n_vol, 6, 24, 24)).astype(np.float32) for o in geoms}
    return stacks, geoms


def test_reconstruct_is_two_stages_and_the_mean_and_needs_three_orientations():
    stacks, geoms = _stacks()
    out, g, st = R.reconstruct(stacks, geoms, return_stages=True)
    assert out.shape == (2, 24, 24, 24) and out.dtype == np.float32
    assert g.GetOrigin() == geoms["ax"].GetOrigin() and g.GetSpacing() == (1.0, 1.0, 1.0)
    assert np.array_equal(out, ((st["H"][0].astype(np.float64) + st["R"][0]) + st["R"][1]).__truediv__(3).astype(np.float32))
    # stage 1 of the ax stack at a slice centre is the slice: H index 4 k along z lies on node k
    assert np.array_equal(st["H"][0][:, 0], stacks["ax"][:, 0]) and np.array_equal(st["H"][0][:, 4], stacks["ax"][:, 1])
    # fixed = sag puts the result on the sag grid; the moving order is then ax, cor
    out_s, g_s = R.reconstruct(stacks, geoms, fixed="sag")
    assert g_s.GetDirection() == geoms["sag"].GetDirection() and R.moving_order("sag") == ["ax", "cor"]
    two = {o: stacks[o] for o in ("ax", "cor")}
    with pytest.raises(ValueError, match="three orientations"):
        R.reconstruct(two, {o: geoms[o] for o in two})
    with pytest.raises(ValueError):
        R.reconstruct(stacks, geoms, transforms={"ax": np.eye(4)})  # the fixed one has no transform


# ---- the built library ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from fetal_t2mapping_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        from fetal_t2mapping_amd import build

        build.build()
    return _lib.load()


def _err(lib):
    return lib.t2fit_last_error().decode()


def test_library_keeps_abi_5_and_exports_the_three_symbols(lib):
    from fetal_t2mapping_amd import _abi

    assert lib.t2fit_abi_version() == 5 == _abi.ABI_VERSION
    for name in ("t2fit_resample_dev", "t2fit_reconstruct_workspace_bytes", "t2fit_reconstruct_dev"):
        assert hasattr(lib, name) and name in _abi.ADDITIVE
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "t2fit.h")).read()
    for name in ("t2fit_resample_dev", "t2fit_reconstruct_workspace_bytes", "t2fit_reconstruct_dev", "T2FIT_RECON_CHAIN"):
        assert name in header
    assert "#define T2FIT_ABI_VERSION 5" in header


def test_resample_refuses_bad_arguments_without_a_device(lib):
    from fetal_t2mapping_amd import _abi

    A = (C.c_double * 12)(*np.eye(3, 4).ravel())
    src, dst = 0x1000, 0x2000  # never dereferenced: every call below is refused first

    def call(src=src, stype=0, n=(4, 5, 6), A=A, dst=dst, o=(4, 5, 6), n_vol=1, interp=0, default=0.0, flags=0):
        return lib.t2fit_resample_dev(src, stype, *n, A, dst, *o, n_vol, interp, default, flags, None)

    for kwargs, text in (({"src": None}, "NULL"), ({"dst": None}, "NULL"), ({"A": None}, "NULL"),
                         ({"n": (0, 5, 6)}, ">= 1"), ({"o": (4, 5, -1)}, ">= 1"), ({"n_vol": 0}, ">= 1"),
                         ({"interp": 2}, "unknown interp"), ({"stype": 7}, "unknown src_type"),
                         ({"stype": 1}, "int32 source"), ({"flags": 4}, "not defined"), ({"flags": 2}, "not defined"),
                         ({"flags": 1, "interp": 1}, "INTEGER_CAST"), ({"src": 0x1001}, "aligned"),
                         ({"dst": src}, "must not be src_dev"), ({"stype": 1, "interp": 1, "default": 3e9}, "default_value")):
        assert call(**kwargs) == _abi.E_INVALID, kwargs
        assert text in _err(lib), (kwargs, _err(lib))
    for bad in (np.nan, np.inf):
        B = (C.c_double * 12)(*np.eye(3, 4).ravel())
        B[7] = bad
        assert call(A=B) == _abi.E_INVALID and "non-finite" in _err(lib)


def test_reconstruct_workspace_arithmetic_and_refusals_without_a_device(lib):
    from fetal_t2mapping_amd import _abi

    lo = (C.c_int32 * 9)(6, 24, 24, 6, 24, 25, 7, 24, 24)
    hi = (C.c_int32 * 9)(24, 24, 24, 24, 24, 25, 28, 24, 24)
    need = C.c_size_t(123)
    assert lib.t2fit_reconstruct_workspace_bytes(3, lo, hi, 0, C.byref(need)) == 0 and need.value == 0  # fused: none
    assert lib.t2fit_reconstruct_workspace_bytes(3, lo, hi, _abi.RECON_CHAIN, C.byref(need)) == 0
    up = lambda v: (v + 255) // 256 * 256
    assert need.value == up(4 * 3 * 24 * 24 * 25) + up(4 * 3 * 28 * 24 * 24) + 2 * up(4 * 3 * 24 ** 3)
    assert lib.t2fit_reconstruct_workspace_bytes(3, lo, hi, 0, None) == _abi.E_INVALID
    assert lib.t2fit_reconstruct_workspace_bytes(0, lo, hi, 0, C.byref(need)) == _abi.E_INVALID and ">= 1" in _err(lib)
    assert lib.t2fit_reconstruct_workspace_bytes(3, lo, hi, 8, C.byref(need)) == _abi.E_INVALID and "not defined" in _err(lib)
    assert lib.t2fit_reconstruct_workspace_bytes(3, None, hi, 0, C.byref(need)) == _abi.E_INVALID

    A1 = (C.c_double * 36)(*np.tile(np.eye(3, 4).ravel(), 3))
    A2 = (C.c_double * 24)(*np.tile(np.eye(3, 4).ravel(), 2))
    ptrs = (C.c_void_p * 3)(0x1000, 0x2000, 0x3000)
    out = 0x10000

    def call(ptrs=ptrs, lo=lo, A1=A1, hi=hi, A2=A2, out=out, n_vol=3, flags=0, ws=None, ws_bytes=0):
        return lib.t2fit_reconstruct_dev(ptrs, lo, A1, hi, A2, out, n_vol, flags, ws, ws_bytes, None)

    null_entry = (C.c_void_p * 3)(0x1000, None, 0x3000)
    same = (C.c_void_p * 3)(0x1000, out, 0x3000)
    bad_hi = (C.c_int32 * 9)(24, 24, 24, 24, 0, 25, 28, 24, 24)
    nan2 = (C.c_double * 24)(*np.tile(np.eye(3, 4).ravel(), 2))
    nan2[13] = np.nan
    for kwargs, text in (({"ptrs": None}, "NULL"), ({"out": None}, "NULL"), ({"A1": None}, "NULL"), ({"A2": None}, "NULL"),
                         ({"ptrs": null_entry}, "NULL"), ({"ptrs": same}, "out_dev"), ({"hi": bad_hi}, ">= 1"),
                         ({"n_vol": 0}, ">= 1"), ({"A2": nan2}, "non-finite"), ({"flags": 4}, "not defined"),
                         ({"flags": _abi.RECON_CHAIN}, "needs workspace_dev"),
                         ({"flags": _abi.RECON_CHAIN, "ws": 0x100100, "ws_bytes": need.value - 1}, "workspace too small"),
                         ({"flags": _abi.RECON_CHAIN, "ws": 0x100104, "ws_bytes": need.value}, "aligned to 256")):
        assert call(**kwargs) == _abi.E_INVALID, kwargs
        assert text in _err(lib), (kwargs, _err(lib))


# ---- flags ------------------------------------------------------------------------------------------------------
def test_recon_flag_parsing(tmp_path):
    from fetal_t2mapping_amd import recon

    base = ["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo", "--lf"]
    a = recon.parse_arguments(base)
    assert (a.fixed, a.res, a.transforms, a.write_resamp, a.no_denoise) == ("ax", 1.0, None, False, False)
    a = recon.parse_arguments(base + ["--fixed", "sag", "--res", "0.8", "--transforms", str(tmp_path), "--write_resamp",
                                      "--no_denoise"])
    assert (a.fixed, a.res, a.transforms, a.write_resamp, a.no_denoise) == ("sag", 0.8, str(tmp_path), True, True)
    for bad in (["--fixed", "oblique"], ["--res", "0"], ["--transforms", str(tmp_path / "nowhere")]):
        with pytest.raises(SystemExit):
            recon.parse_arguments(base + bad)
    with pytest.raises(SystemExit):
        recon.parse_arguments(["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo"])  # --lf | --hf is required
    # a transform file is read per moving orientation; a missing one is the identity (absent from the dict)
    acq = {"sub": "sub-001", "ses": "ses-01"}
    m = np.eye(4)
    m[0, 3] = 2.5
    np.savetxt(recon.transform_path(str(tmp_path), acq, "cor"), m)
    got = recon.load_transforms(str(tmp_path), acq, "ax")
    assert list(got) == ["cor"] and np.array_equal(got["cor"], m)
    assert recon.load_transforms(None, acq, "ax") == {}
    np.savetxt(recon.transform_path(str(tmp_path), acq, "sag"), np.eye(3))
    with pytest.raises(ValueError, match="4 x 4"):
        recon.load_transforms(str(tmp_path), acq, "ax")


def test_recon_groups_each_echo_once():
    import pandas as pd

    from fetal_t2mapping_amd import recon

    rows = [{"prj": "prj-900", "sub": "sub-001", "ses": "ses-01", "run": f"run-{i:02d}", "EchoTime": te,
             "ImageOrientationPatientSTR": o, "CoilString": "HeadNeck"}
            for i, (te, o) in enumerate([(0.114, "ax"), (0.114, "cor"), (0.114, "sag"), (0.202, "ax"), (0.202, "sag")])]
    groups = recon.echo_groups(pd.DataFrame(rows))
    assert len(groups) == 1 and groups[0][:3] == ("prj-900", "sub-001", "ses-01")
    echoes = groups[0][3]
    assert [te for te, _ in echoes] == [0.114, 0.202]
    assert sorted(echoes[0][1]) == ["ax", "cor", "sag"] and sorted(echoes[1][1]) == ["ax", "sag"]


def test_cli_reconstruct_flags_and_the_shared_volume_refusal(tmp_path, monkeypatch):
    import pandas as pd

    from fetal_t2mapping_amd import cli

    base = ["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo", "--gaussian", "--lf", "--sim", "s"]
    a = cli.parse_arguments(base)
    assert a.reconstruct is False and a.reconstruct_args is None  # off by default
    a = cli.parse_arguments(base + ["--reconstruct"])
    assert a.reconstruct_args == {"fixed": "ax", "res": 1.0, "transforms_dir": None}
    a = cli.parse_arguments(base + ["--reconstruct", "--recon_fixed", "cor", "--recon_res", "1.5", "--denoise", "tv"])
    assert a.reconstruct_args == {"fixed": "cor", "res": 1.5, "transforms_dir": None} and a.denoise_args is not None
    for bad in (["--recon_fixed", "sag"], ["--recon_res", "2"], ["--reconstruct", "--recon_res", "-1"],
                ["--reconstruct", "--recon_transforms", str(tmp_path / "nowhere")]):
        with pytest.raises(SystemExit):
            cli.parse_arguments(base + bad)
    # one subject, two ranks: the volume would be shared, which --reconstruct refuses before anything is read
    rows = [{"prj": "prj-900", "sub": "sub-001", "ses": "ses-01", "run": "run-01", "EchoTime": 0.114,
             "ImageOrientationPatientSTR": "ax", "CoilString": "HeadNeck"}]
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("LOCAL_RANK", "0")
    fit, fit_params = cli.t2map.set_fit_params(a)
    with pytest.raises(ValueError, match="--reconstruct is not run on a volume that is shared"):
        cli.process_t2maps(pd.DataFrame(rows), str(tmp_path) + "/", [114], fit, fit_params, False, True, True, False, False,
                           "s", reconstruct=a.reconstruct_args)


# ---- the statement against the reference written from the definition (tests/resample_cases.py) ------------------------
import resample_cases as K  # noqa: E402



def _statement(case, volumes=None):
    src = case.src if volumes is None else case.src[:volumes]
    with np.errstate(over="ignore"):
        return R.resample(src, case.A, case.out_shape, case.interp, case.default, case.integer_cast)


@pytest.mark.parametrize("group", sorted(K.SINGLE_STAGE_GROUPS))
def test_statement_meets_the_reference_from_the_definition(group):
    """Equality on the dyadic cases, the derived bar |got - e| <= ulp32(e)/2 + 32 * 2^-53 * M elsewhere; non-finite
    results by class and position, nearest by bits."""
    worst = (0.0, 0.0)
    for case in K.SINGLE_STAGE_GROUPS[group]():
        ref = K.reference(case)
        assert ref.inside.any() and ref.coord_ratio <= 1.0, case
        worst = max(worst, K.check(case, _statement(case)))
        if case.n_vol == 3:
            K.check(case, _statement(case, 1), volumes=1)
    print(f"{group}: worst ratio to the bar {worst[0]:.4f}, excess over ulp32/2 in units of 32 * 2^-53 * M {worst[1]:.4f}")


def test_the_cases_contain_what_they_are_there_for():
    """The reference alone: the named cases reach the edges they are meant to reach."""
    on = K.reference(K.cast_cases()[0])
    exact = on.exact[on.inside & (on.cls == K.FINITE)]
    assert on.negzero.any() and (exact == 32767).any() and (exact == -32768).any() and (on.cls == K.NAN).any()
    assert any(e not in (32767, -32768, 0) and e < 0 for e in exact)
    for case in K.non_finite_cases():
        ref = K.reference(case)
        cls = ref.cls[ref.inside]
        assert all((cls == c).any() for c in (K.FINITE, K.POS_INF, K.NEG_INF, K.NAN)), case
    whole = K.reference(K.non_finite_cases()[0])
    assert whole.taps[whole.inside].max() == 4  # not 8: the whole-voxel axis has weight 0
    for la in K.LANE_AXES:
        for case in K.brick_cases(la):
            ref = K.reference(case)
            assert ref.inside.any() and (case.out_shape == (1, 1, 1) or not ref.inside.all()), case
    for case in K.nearest_cases():
        bits = K.reference(case).bits
        wanted = (K.NAN_QUIET, K.NAN_SIGNALLING, 0x80000000) if case.src.dtype == np.float32 else (0x80000000, 0x7FFFFFFF, 16777217, 16777219)
        assert all((bits == w).any() for w in wanted), case


@pytest.mark.parametrize("la", K.LANE_AXES)
def test_rim_and_tie_facts_of_the_statement_on_every_axis(la):
    for case in K.rim_cases(la):
        K.rim_facts(case, _statement(case))


def test_merge_meets_the_reference_in_the_order_of_the_definition():
    a, b, c = K.merge_inputs()
    K.check_merge(R.merge(a, b, c), a, b, c)
    assert R.merge(np.float32([2.0 ** 60]), np.float32([-2.0 ** 60]), np.float32([1.0]))[0] == np.float32(1.0 / 3.0)


RECON_HOST_CASES = [(f, r, 1, "both") for f in K.RECON_FIXED for r in K.RECON_RES] + [("sag", 1.0, 3, "far"), ("ax", 1.0, 1, "cast")]


@pytest.mark.parametrize("fixed,res,n_vol,kind", RECON_HOST_CASES)
def test_reconstruct_meets_the_reference_stage_by_stage(fixed, res, n_vol, kind):
    stacks, geoms, kw = K.recon_case(fixed, res, n_vol, kind)
    with np.errstate(all="ignore"):
        merged, grid, stages = R.reconstruct(stacks, geoms, return_stages=True, **kw)
    assert merged.shape[0] == n_vol and (K.ragged(merged.shape) if res != 1.0 else merged.shape[-3:] == (8, 8, 9))
    K.recon_facts(kind, stages)
    print(f"{fixed} {res} {n_vol} {kind}: worst ratio to the bar {K.check_reconstruction(stacks, geoms, kw, merged, stages):.6f}")


def test_resample_volume_refuses_labels_that_do_not_fit_int32_before_any_launch():
    from fetal_t2mapping_amd import _gpu_resample

    g = R.Geometry((4, 3, 2))
    for bad, text in ((np.full((2, 3, 4), 2 ** 32 + 7, np.int64), "4294967303"), (np.full((2, 3, 4), 2 ** 31, np.uint32), "2147483648"),
                      (np.array([[[-2 ** 31 - 1, 5]]], np.int64), "-2147483649"), (np.full((1, 1, 1), 2 ** 63, np.uint64), str(2 ** 63))):
        with pytest.raises(ValueError, match="int32") as err:
            _gpu_resample.resample_volume(bad, g, like=g, interp="nearest")
        assert text in str(err.value), str(err.value)
    import torch

    # torch's unsigned 32- and 64-bit tensors too (torch does not reduce them: their bits are read as the signed type)
    for bad, text in ((torch.tensor([[[7, 2 ** 31 + 1, 3]]], dtype=torch.int64).to(torch.uint32), f"[3, {2 ** 31 + 1}]"),
                      (torch.tensor([[[2 ** 63, 5]]], dtype=torch.uint64), f"[5, {2 ** 63}]"),
                      (torch.tensor([[[7, 2 ** 40]]], dtype=torch.uint64), f"[7, {2 ** 40}]"),
                      (torch.full((2, 3, 4), -2 ** 31 - 1, dtype=torch.int64), str(-2 ** 31 - 1))):
        with pytest.raises(ValueError, match="int32") as err:
            _gpu_resample.resample_volume(bad, g, like=g, interp="nearest")
        assert text in str(err.value), str(err.value)
