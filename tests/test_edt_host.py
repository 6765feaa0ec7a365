"""The distance transform without a GPU: the numpy statement (fetal_t2mapping_amd/_edt.py) against the brute-force
minimum and against scipy.ndimage.distance_transform_edt, the two traps of the tie rule, the degenerate site sets, what is
built on the statement (balls in millimetres against _morph, surface distances against a scipy formulation, island
reassignment), every refusal of the three C entry points (all made before HIP is touched), and the symbols.  The
drivers' flags are in test_edt_drivers_host.py; the device is held to the statement in test_edt_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest
from scipy import ndimage as ndi

import edt_cases as K
from fetal_t2mapping_amd import _abi, _edt, _morph

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(shape, density, invert) for shape in K.SMALL_SHAPES for density in K.DENSITIES for invert in (0, 1)]


@pytest.fixture(scope="module")
def lib():
    from fetal_t2mapping_amd import build
    from fetal_t2mapping_amd._lib import load

    build.build()
    return load()


# ---- the statement ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spacing", K.SPACINGS, ids=str)
def test_against_the_brute_force(spacing):
    for shape, density, invert in CASES:
        a = K.as_input(K.sites(shape, density), invert)
        d2, index = _edt.nearest(a, invert, spacing)
        want_d2, want_index = _edt.brute(a, invert, spacing)
        assert d2.dtype == np.float64 and index.dtype == np.int32 and d2.shape == index.shape == shape
        assert np.array_equal(d2, want_d2), (shape, density, invert)  # for ANY spacing
        if spacing in K.EXACT:
            assert np.array_equal(index, want_index), (shape, density, invert)
        else:  # the site found is one that attains the minimum
            z, y, x = np.indices(shape)
            qz, qy, qx = np.unravel_index(np.where(index >= 0, index, 0), shape)
            tz, ty, tx = (z - qz) * spacing[0], (y - qy) * spacing[1], (x - qx) * spacing[2]
            assert np.array_equal(np.where(index >= 0, (tz * tz + ty * ty) + tx * tx, np.inf), d2)


@pytest.mark.parametrize("spacing", K.SPACINGS, ids=str)
def test_against_scipy(spacing):
    compared = 0
    for shape, density, invert in CASES:
        a = K.as_input(K.sites(shape, density), invert)
        site = (a == 0) if invert else (a != 0)
        if not site.any():
            continue  # scipy has no answer without a background voxel; test_no_site_at_all holds ours
        d2, index = _edt.nearest(a, invert, spacing)
        want, at = ndi.distance_transform_edt(~site, sampling=spacing, return_indices=True)
        compared += 1
        if spacing in K.EXACT:
            assert np.array_equal(np.sqrt(d2), want), (shape, density, invert)
            z, y, x = np.indices(shape)
            tz, ty, tx = (z - at[0]) * spacing[0], (y - at[1]) * spacing[1], (x - at[2]) * spacing[2]
            assert np.array_equal((tz * tz + ty * ty) + tx * tx, d2)  # scipy's site is as near as ours; it need not be ours
        else:
            # five roundings of the expression are about 6e-16; a wrong site changes the value by parts in 10^3 here
            np.testing.assert_allclose(np.sqrt(d2), want, rtol=1e-12, atol=0.0)
        if invert:
            assert np.array_equal(_edt.edt(a, spacing), np.sqrt(d2)) and np.array_equal(_edt.edt(a, spacing, squared=True), d2)
    assert compared > 30


@pytest.mark.parametrize("name", list(K.traps()))
@pytest.mark.parametrize("invert", (0, 1))
def test_tie_traps(name, invert):
    a, query, want = K.traps()[name]
    d2, index = _edt.nearest(K.as_input(a, invert), invert)
    assert index[query] == K.linear(a.shape, want)
    assert d2[query] == (2.0 if name == "scan_order" else 25.0)
    bd2, bindex = _edt.brute(K.as_input(a, invert), invert)
    assert np.array_equal(d2, bd2) and np.array_equal(index, bindex)


def test_no_site_at_all():
    for shape in ((1, 1, 1), (3, 4, 5)):
        for invert, a in ((0, np.zeros(shape, np.uint8)), (1, np.ones(shape, np.uint8))):
            d2, index = _edt.nearest(a, invert, (2.0, 1.0, 0.5))
            assert np.all(d2 == np.inf) and np.all(index == -1)
        assert np.all(_edt.edt(np.ones(shape, np.uint8)) == np.inf)


def test_every_voxel_a_site():
    shape = (3, 4, 5)
    d2, index = _edt.nearest(np.ones(shape, bool), 0, (0.8, 1.1, 1.0))
    assert np.all(d2 == 0.0) and np.array_equal(index.reshape(-1), np.arange(60))
    d2, index = _edt.nearest(np.zeros(shape, np.int32), 1)
    assert np.all(d2 == 0.0) and np.array_equal(index.reshape(-1), np.arange(60))


def test_one_site_in_a_corner():
    shape, s = (4, 5, 6), (4.5, 1.0, 1.0)
    a = K.sites(shape, "corner")
    d2, index = _edt.nearest(a, 0, s)
    z, y, x = np.indices(shape)
    assert np.array_equal(d2, (((3 - z) * 4.5) ** 2 + (4 - y) ** 2.0) + (5 - x) ** 2.0) and np.all(index == 4 * 5 * 6 - 1)


def test_refusals_of_the_statement():
    a = np.zeros((2, 2, 2), np.uint8)
    for bad in ((1, 1), (1, 1, 0), (1, -1, 1), (1, np.inf, 1), (np.nan, 1, 1)):
        with pytest.raises(ValueError, match="spacing"):
            _edt.nearest(a, 0, bad)
    with pytest.raises(ValueError, match="3-D"):
        _edt.nearest(a[0])
    with pytest.raises(ValueError, match="invert"):
        _edt.nearest(a, 2)


# ---- what is built on it -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", (1, 2, 3))
def test_balls_in_millimetres_against_morph(r):
    m = K.blobs()
    grown, shrunk = _edt.dilate_mm(m, r + 0.5), _edt.erode_mm(m, r + 0.5)  # (r + 0.5)^2 is no integer: no ties
    assert grown.dtype == shrunk.dtype == np.uint8
    assert np.array_equal(grown, _morph.dilate(m, _morph.ball(r)))
    assert np.array_equal(shrunk, _morph.erode(m, _morph.ball(r), border_value=1)) and shrunk.any()
    # millimetres: on a 1 x 1 x 4.5 grid a ball of 2.5 mm does not reach the next slice
    thick = _edt.dilate_mm(m, 2.5, (4.5, 1.0, 1.0))
    assert np.array_equal(thick, _morph.dilate(m, _morph.ball((0, 2, 2))))
    assert np.array_equal(_edt.erode_mm(np.ones((3, 3, 3)), 50.0), np.ones((3, 3, 3), np.uint8))  # no site outside the grid


def test_fill_nearest():
    lab = np.arange(24, dtype=np.int32).reshape(2, 3, 4) * 10
    where = np.zeros(lab.shape, np.uint8)
    where[0, 1] = 1
    where[1, 2, 3] = 7
    index = np.full(lab.shape, 5, np.int32)
    index[0, 1, 2] = -1
    out = _edt.fill_nearest(lab, where, index)
    want = lab.copy()
    want[0, 1] = 50
    want[0, 1, 2] = lab[0, 1, 2]
    want[1, 2, 3] = 50
    assert np.array_equal(out, want) and out.dtype == np.int32


def _scipy_surface_distances(a, b, spacing):
    sa, sb = a & ~ndi.binary_erosion(a), b & ~ndi.binary_erosion(b)
    ab = ndi.distance_transform_edt(~sb, sampling=spacing)[sa]
    ba = ndi.distance_transform_edt(~sa, sampling=spacing)[sb]
    return ab, ba


@pytest.mark.parametrize("spacing", (K.UNIT, (4.5, 1.0, 1.0), (1.25, 0.5, 0.5)), ids=str)
def test_surface_distances_of_two_offset_balls(spacing):
    shape, shift = (15, 16, 24), 4
    a, b = K.ball_mask(shape, (7, 7, 8), 5), K.ball_mask(shape, (7, 7, 8 + shift), 5)
    assert np.array_equal(_edt.surface(a), a.astype(bool) & ~ndi.binary_erosion(a.astype(bool)))
    got = _edt.surface_distances(a, b, spacing)
    # b is a shifted along x by 4 voxels: every surface voxel has its image 4 voxels away and b's farthest voxel has
    # nothing of a nearer, so the Hausdorff distance is 4 voxels of x
    assert got["hausdorff"] == shift * spacing[2]
    ab, ba = _scipy_surface_distances(a.astype(bool), b.astype(bool), spacing)
    assert got["n_a"] == ab.size and got["n_b"] == ba.size and got["n_a"] == got["n_b"] > 100
    assert got["hausdorff"] == max(ab.max(), ba.max())
    assert got["hd95"] == max(np.percentile(ab, 95), np.percentile(ba, 95)) and 0 < got["hd95"] <= got["hausdorff"]
    assert got["assd"] == (ab.sum() + ba.sum()) / (ab.size + ba.size) and 0 < got["assd"] < got["hd95"]
    same = _edt.surface_distances(a, a, spacing)
    assert same["hausdorff"] == same["hd95"] == same["assd"] == 0.0
    with pytest.raises(ValueError, match="empty"):
        _edt.surface_distances(a, np.zeros(shape, np.uint8), spacing)
    with pytest.raises(ValueError, match="grid"):
        _edt.surface_distances(a, b[1:], spacing)


def test_surface_at_the_grids_edge():
    full = np.ones((3, 4, 5), np.uint8)
    s = _edt.surface(full)
    assert s.dtype == np.uint8 and s.sum() == 60 - 1 * 2 * 3 and not s[1, 1:3, 1:4].any()


def test_reassign_small():
    c, island = K.slab()
    same, changed = _edt.reassign_small(c, island)  # min_size == the island's size: nothing is small but the speck,
    assert changed == 0 and np.array_equal(same, c) and same.dtype == np.int32  # which takes class 2 again
    out, changed = _edt.reassign_small(c, island + 1)
    assert changed == 2 * island
    want = c.copy()
    want[3:5, 4:6, 3:5] = 1
    want[3:5, 4:6, 9:11] = 2
    assert np.array_equal(out, want) and out[4, 5, 15] == 2  # the speck stays a speck: remove_small's job
    assert np.array_equal(out == 0, c == 0)  # class 0 stays 0, nothing else becomes 0
    # the speck alone, next to class 1: it takes the nearest class
    d = c.copy()
    d[4, 5, 15] = 0
    d[4, 5, 0] = 2
    out, changed = _edt.reassign_small(d, 2)
    assert changed == 1 and out[4, 5, 0] == 1
    # no site: every component is small, the volume comes back unchanged
    out, changed = _edt.reassign_small(c, 10**6)
    assert changed == 0 and np.array_equal(out, c)
    out, changed = _edt.reassign_small(np.zeros((2, 2, 2), np.int32), 5)
    assert changed == 0 and not out.any()
    assert _edt.reassign_small(c, 0)[1] == 0
    # anisotropic spacing decides between two equally many voxels away
    e = np.zeros((5, 1, 5), np.int32)
    e[0], e[:, :, 4] = 1, 2
    e[0, 0, 4] = 1
    e[2, 0, 2] = 3
    assert _edt.reassign_small(e, 2, spacing=(1.0, 1.0, 3.0))[0][2, 0, 2] == 1
    assert _edt.reassign_small(e, 2, spacing=(3.0, 1.0, 1.0))[0][2, 0, 2] == 2
    with pytest.raises(ValueError, match="negative"):
        _edt.reassign_small(c, -1)


# ---- the C entry points, no device ----------------------------------------------------------------------------------------

def _refused(lib, rc, *words):
    assert rc == _abi.E_INVALID
    msg = lib.t2fit_last_error().decode()
    for w in words:
        assert w in msg, msg


def test_workspace_formula_and_refusals(lib):
    need = C.c_size_t(0)
    for shape in ((1, 1, 1), (3, 5, 7), (9, 17, 131), (256, 256, 256), (2048, 2048, 511)):
        assert lib.t2fit_edt_workspace_bytes(*shape, C.byref(need)) == _abi.OK
        n = int(np.prod(np.array(shape, np.int64)))
        assert need.value == 2 * (-(-8 * n // 256) * 256) + 2 * (-(-4 * n // 256) * 256)
    _refused(lib, lib.t2fit_edt_workspace_bytes(4, 4, 4, None), "bytes is NULL")
    _refused(lib, lib.t2fit_edt_workspace_bytes(0, 4, 4, C.byref(need)), "1..2048")
    _refused(lib, lib.t2fit_edt_workspace_bytes(4, -1, 4, C.byref(need)), "1..2048")
    _refused(lib, lib.t2fit_edt_workspace_bytes(4, 4, 2049, C.byref(need)), "1..2048")
    _refused(lib, lib.t2fit_edt_workspace_bytes(2048, 2048, 512, C.byref(need)), "2^31")
    header = open(os.path.join(REPO, "include", "t2fit.h")).read()
    assert f"#define T2FIT_EDT_MAX_AXIS {_edt.MAX_AXIS}\n" in header and _abi.EDT_MAX_AXIS == _edt.MAX_AXIS


def test_edt_refusals_before_hip(lib):
    v, d, i, ws = C.c_void_p(4096), C.c_void_p(8192), C.c_void_p(16384), C.c_void_p(1 << 20)
    big = 1 << 20
    s = (C.c_double * 3)(1.0, 1.0, 1.0)
    call = lib.t2fit_edt_dev
    _refused(lib, call(None, 1, 4, 4, 4, s, d, i, ws, big, None), "vol_dev is NULL")
    _refused(lib, call(v, 1, 4, 4, 4, s, None, None, ws, big, None), "both NULL")
    for invert in (2, -1):
        _refused(lib, call(v, invert, 4, 4, 4, s, d, i, ws, big, None), "invert")
    _refused(lib, call(v, 1, 0, 4, 4, s, d, i, ws, big, None), "1..2048")
    _refused(lib, call(v, 1, 4, 2049, 4, s, d, i, ws, big, None), "1..2048")
    _refused(lib, call(v, 1, 2048, 2048, 512, s, d, i, ws, big, None), "2^31")
    for bad in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("inf")), (float("nan"), 1.0, 1.0)):
        _refused(lib, call(v, 1, 4, 4, 4, (C.c_double * 3)(*bad), d, i, ws, big, None), "spacing")
    _refused(lib, call(v, 1, 4, 4, 4, s, C.c_void_p(8196), i, ws, big, None), "aligned")
    _refused(lib, call(v, 1, 4, 4, 4, s, d, C.c_void_p(16386), ws, big, None), "aligned")
    _refused(lib, call(v, 1, 4, 4, 4, s, d, i, None, big, None), "workspace_dev is NULL")
    _refused(lib, call(v, 1, 4, 4, 4, s, d, i, C.c_void_p((1 << 20) + 64), big, None), "aligned to 256")
    _refused(lib, call(v, 1, 4, 4, 4, None, d, None, ws, 1535, None), "1535", "1536")  # 2 x 512 + 2 x 256; NULL spacing is 1


def test_fill_refusals_before_hip(lib):
    lab, w, i, out = C.c_void_p(4096), C.c_void_p(8192), C.c_void_p(16384), C.c_void_p(32768)
    call = lib.t2fit_edt_fill_dev
    for args in ((None, w, i, 8, out), (lab, None, i, 8, out), (lab, w, None, 8, out), (lab, w, i, 8, None)):
        _refused(lib, call(*args, None), "NULL")
    _refused(lib, call(lab, w, i, 0, out, None), "n must be")
    _refused(lib, call(lab, w, i, 2**31, out, None), "n must be")
    _refused(lib, call(C.c_void_p(4098), w, i, 8, out, None), "aligned to 4")
    _refused(lib, call(lab, w, C.c_void_p(16385), 8, out, None), "aligned to 4")
    _refused(lib, call(lab, w, i, 8, C.c_void_p(32770), None), "aligned to 4")
    _refused(lib, call(lab, w, i, 8, lab, None), "must not be labels_dev")


def test_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(REPO, "include", "t2fit.h")).read()
    names = {n for n, _, _ in _abi.SYMBOLS}
    assert _abi.EDT_SYMBOLS == ("t2fit_edt_workspace_bytes", "t2fit_edt_dev", "t2fit_edt_fill_dev")
    for sym in _abi.EDT_SYMBOLS:
        assert sym in names and sym + "(" in header and sym in _abi.LOOKED_UP and sym not in _abi.ADDITIVE
        assert hasattr(lib, sym) and getattr(lib, sym).argtypes is not None
    assert lib.t2fit_abi_version() == 5
    from fetal_t2mapping_amd import build

    assert any(src.endswith("t2fit_edt.hip") for src in build.SOURCES)


def test_the_namespace_and_the_python_refusals():
    from fetal_t2mapping_amd import _gpu_components, _gpu_edt, t2map

    assert t2map.distance is _gpu_edt and t2map.components.reassign_small is _gpu_components.reassign_small
    for name in ("nearest", "edt", "fill_nearest", "dilate_mm", "erode_mm", "surface", "surface_distances"):
        assert callable(getattr(t2map.distance, name))
    for module in (_edt, _gpu_edt):  # the statement and the binding speak of scipy, neither uses it
        text = open(module.__file__).read()
        assert "import scipy" not in text and "from scipy" not in text
