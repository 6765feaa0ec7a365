"""Connected components without a GPU: the numpy statement (fetal_t2mapping_amd/_components.py) against
scipy.ndimage.label on every case of tests/components_cases.py, the statistics, the selection table, the seed rounding,
the refusals of the four C entry points (all made before HIP is touched), and the symbols.  The drivers' flags are in
test_components_drivers_host.py; the device is held to the statement in test_components_gpu.py.  Every comparison is
integer equality."""
import ctypes as C
import os

import numpy as np
import pytest

import components_cases as K
from fetal_t2mapping_amd import _abi, _components, _register

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASKS = K.mask_cases()
CLASSES = K.class_cases()


@pytest.fixture(scope="module")
def lib():
    from fetal_t2mapping_amd import build
    from fetal_t2mapping_amd._lib import load

    build.build()
    return load()


# ---- the labelling ---------------------------------------------------------------------------------------------------------

def test_the_tile_is_the_headers():
    header = open(os.path.join(REPO, "include", "t2fit.h")).read()
    for axis, n in zip("ZYX", _components.TILE):
        assert f"#define T2FIT_COMPONENTS_TILE_{axis} {n}\n" in header
    assert _abi.COMPONENTS_TILE == _components.TILE


@pytest.mark.parametrize("connectivity", K.CONNECTIVITIES)
@pytest.mark.parametrize("index", range(len(MASKS)), ids=[name for name, _ in MASKS])
def test_masks_against_scipy(index, connectivity):
    a = MASKS[index][1]
    ref, n_ref = K.scipy_label(a, connectivity)
    lab, n = K.statement("mask", index, connectivity)
    assert lab.dtype == np.int32 and lab.shape == a.shape
    assert n == n_ref and np.array_equal(lab, ref)


@pytest.mark.parametrize("connectivity", K.CONNECTIVITIES)
@pytest.mark.parametrize("index", range(len(CLASSES)), ids=[name for name, _ in CLASSES])
def test_classes_against_the_per_class_scipy_loop(index, connectivity):
    a = CLASSES[index][1]
    ref, n_ref = K.scipy_label(a, connectivity)
    lab, n = K.statement("classes", index, connectivity)
    assert n == n_ref and np.array_equal(lab, ref)
    assert n > len(np.unique(a[a != 0])) or a.size < 100  # a class falls into several components


def test_known_counts():
    tz, ty, tx = K.T
    for shape in K.shapes():
        assert _components.label(K.empty(shape))[1] == 0
        assert all(_components.label(K.full(shape), c)[1] == 1 for c in K.CONNECTIVITIES)
    for shape in (K.MID, K.BIG):
        n_vox = int(np.prod(shape))
        assert [_components.label(K.checkerboard(shape), c)[1] for c in (1, 2, 3)] == [(n_vox + 1) // 2, 1, 1]
        assert _components.label(K.corners(shape), 3)[1] == 8
        s = K.serpentine(shape)
        for c in K.CONNECTIVITIES:
            assert _components.label(s, c)[1] == 1
            lab, n = _components.label(K.comb(shape), c)
            assert n == 1 and lab[0, 0, 0] == 1
        for z0 in range(0, shape[0], tz):
            for y0 in range(0, shape[1], ty):
                for x0 in range(0, shape[2], tx):
                    assert s[z0:z0 + tz, y0:y0 + ty, x0:x0 + tx].any()  # the path visits every tile
    for a, counts in K.touching_pairs():
        assert tuple(_components.label(a, c)[1] for c in (1, 2, 3)) == counts


def test_a_plane_is_a_volume_with_one_slice():
    from scipy import ndimage

    a = K.random_mask((1, 23, 31), 0.5, seed=3)
    for c, st in ((1, ndimage.generate_binary_structure(2, 1)), (2, ndimage.generate_binary_structure(2, 2))):
        ref, n_ref = ndimage.label(a[0], st)
        lab, n = _components.label(a, c)
        assert n == n_ref and np.array_equal(lab[0], ref)


def test_label_refusals():
    with pytest.raises(ValueError, match="connectivity"):
        _components.label(np.zeros((2, 2, 2), np.uint8), 4)
    with pytest.raises(ValueError, match="3-D"):
        _components.label(np.zeros((2, 2), np.uint8))
    with pytest.raises(ValueError, match="integer"):
        _components.label(np.zeros((2, 2, 2), np.float32))


# ---- statistics, tables, seeds -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,index", [("mask", i) for i, (name, _) in enumerate(MASKS) if "131" in name or "67" in name or "two" in name]
                         + [("classes", i) for i in range(len(CLASSES))])
def test_stats_against_bincount_and_direct_sums(kind, index):
    lab, n = K.statement(kind, index, 1)
    sizes, bbox, sums = _components.stats(lab, n)
    assert sizes.dtype == np.int64 and bbox.dtype == np.int32 and sums.dtype == np.int64
    assert sizes.shape == (n + 1,) and bbox.shape == (n + 1, 6) and sums.shape == (n + 1, 3)
    assert np.array_equal(sizes, np.bincount(lab.reshape(-1), minlength=n + 1))
    for i in range(min(n + 1, 40)):
        z, y, x = np.nonzero(lab == i)
        if z.size == 0:
            assert tuple(bbox[i]) == (*lab.shape, -1, -1, -1) and tuple(sums[i]) == (0, 0, 0)
            continue
        assert tuple(bbox[i]) == (z.min(), y.min(), x.min(), z.max(), y.max(), x.max())
        assert tuple(sums[i]) == (z.sum(), y.sum(), x.sum())


def test_stats_ignores_other_values_and_reports_absent_labels():
    lab = np.array([[[0, 1, 5, -3], [1, 7, 3, 3]]], np.int32)
    sizes, bbox, sums = _components.stats(lab, 3)
    assert sizes.tolist() == [1, 2, 0, 2]
    assert bbox[2].tolist() == [1, 2, 4, -1, -1, -1] and bbox[3].tolist() == [0, 1, 2, 0, 1, 3]
    assert sums[1].tolist() == [0, 1, 1] and sums[2].tolist() == [0, 0, 0]


LUT_SIZES = [np.array([100, 5, 9, 9, 1, 30, 30, 2], np.int64), np.array([7], np.int64), np.array([0, 4], np.int64),
             np.array([3, 0, 6, 0, 6], np.int64)]


@pytest.mark.parametrize("sizes", LUT_SIZES, ids=["eight", "none", "one", "absent"])
@pytest.mark.parametrize("largest", [False, True])
@pytest.mark.parametrize("renumber", [False, True])
def test_lut_against_the_loop(sizes, largest, renumber):
    for min_size, max_size in ((0, 0), (1, 0), (2, 9), (9, 9), (10, 29), (31, 0), (0, 5), (1000, 0)):
        table, kept = _components.lut(sizes, min_size, max_size, largest, renumber)
        ref, ref_kept = K.loop_lut(sizes.tolist(), min_size, max_size, largest, renumber)
        assert table.dtype == np.int32 and table[0] == 0
        assert np.array_equal(table, ref) and kept == ref_kept, (min_size, max_size)


def test_lut_tie_and_refusals():
    table, kept = _components.lut(LUT_SIZES[0], largest=True)
    assert kept == 1 and table.tolist() == [0, 0, 0, 0, 0, 5, 0, 0]  # 30 twice: the lower label
    assert _components.lut(LUT_SIZES[0], 2, 9, largest=True, renumber=True)[0].tolist() == [0, 0, 1, 0, 0, 0, 0, 0]
    assert _components.largest_lut(LUT_SIZES[0], 3).tolist() == [0, 0, 2, 0, 0, 5, 6, 0]
    with pytest.raises(ValueError, match="negative"):
        _components.lut(LUT_SIZES[0], -1)
    with pytest.raises(ValueError, match="negative"):
        _components.lut(LUT_SIZES[0], 0, -2)


def test_seed_rounding():
    a = np.zeros((4, 5, 9), np.uint8)
    a[1, 2, 3] = 1                 # one voxel: itself
    a[3, 0:2, 6:8] = 1             # centroid (3, 0.5, 6.5): half way, rounds up
    a[0, 4, 0:3] = 1               # centroid (0, 4, 1)
    assert _components.seeds(a) == [[1, 4, 0], [3, 2, 1], [7, 1, 3]]
    assert _components.seeds(a, min_size=2) == [[1, 4, 0], [7, 1, 3]]
    assert _components.seeds(a, min_size=2, max_size=3) == [[1, 4, 0]]
    assert _components.seeds(np.zeros((2, 2, 2), np.uint8)) == []
    sizes, sums = np.array([0, 3, 0, 2]), np.array([[0, 0, 0], [3, 4, 5], [0, 0, 0], [1, 1, 2]])
    assert _components.centroids(sizes, sums).tolist() == [[2, 1, 1], [1, 1, 1]]  # (x, y, z); 5/3 -> 2, 4/3 -> 1, 1/2 -> 1


def test_select_keep_largest_remove_small():
    a = K.two_blobs()
    lab, n = _components.label(a)
    assert n == 4 and _components.stats(lab, n)[0].tolist() == [a.size - 61, 24, 12, 24, 1]
    assert np.array_equal(_components.keep_largest(a), (lab == 1).astype(np.uint8))
    assert np.array_equal(_components.keep_largest(a, 2), np.isin(lab, (1, 3)).astype(np.uint8))
    assert np.array_equal(_components.keep_largest(a, 9), a)
    assert np.array_equal(_components.remove_small(a, 12), np.isin(lab, (1, 2, 3)).astype(np.uint8))
    assert np.array_equal(_components.select(lab, n, min_size=2, max_size=12, renumber=True), (lab == 2).astype(np.int32))
    c = K.random_classes(K.MID)
    out = _components.remove_small(c, 4, 2)
    lab, n = _components.label(c, 2)
    sizes = np.bincount(lab.reshape(-1), minlength=n + 1)
    assert out.dtype == np.int32 and np.array_equal(out, np.where((sizes[lab] >= 4) & (lab > 0), c, 0))
    assert (out != c).any() and (out != 0).any()


def test_build_mask_defaults_are_todays_output():
    """The statement path: with the default keywords build_mask is the composition it was."""
    from fetal_t2mapping_amd import _morph

    vol, _ = K.phantom()
    square = np.ones((5, 5, 1), bool)
    today = _morph.erode(_morph.dilate(_morph.fill_holes(vol > np.float32(1.0), slice_axis=2), square), square).astype(np.uint8)
    got = _register.build_mask(vol)
    assert got.dtype == np.uint8 and np.array_equal(got, today)
    assert np.array_equal(_register.build_mask(vol, keep_largest=0, min_size=0, connectivity=3), today)
    cleaned = _register.build_mask(vol, keep_largest=1)
    assert np.array_equal(cleaned, _components.keep_largest(today)) and 0 < cleaned.sum() < today.sum()
    assert np.array_equal(_register.build_mask(vol, min_size=20), _components.remove_small(today, 20))


# ---- the C entry points, no device ----------------------------------------------------------------------------------------

def _refused(lib, rc, *words):
    assert rc == _abi.E_INVALID
    msg = lib.t2fit_last_error().decode()
    for w in words:
        assert w in msg, msg


def test_workspace_formula_and_refusals(lib):
    need = C.c_size_t(0)
    for shape in ((1, 1, 1), (4, 8, 64), (9, 17, 131), (256, 256, 256), (1, 1, 2**31 - 1)):
        assert lib.t2fit_components_workspace_bytes(*shape, C.byref(need)) == _abi.OK
        n = int(np.prod(np.array(shape, np.int64)))
        chunks = -(-n // 1024)
        assert need.value == 256 + -(-4 * chunks // 256) * 256
    _refused(lib, lib.t2fit_components_workspace_bytes(4, 4, 4, None), "bytes is NULL")
    _refused(lib, lib.t2fit_components_workspace_bytes(0, 4, 4, C.byref(need)), "positive")
    _refused(lib, lib.t2fit_components_workspace_bytes(4, -1, 4, C.byref(need)), "positive")
    _refused(lib, lib.t2fit_components_workspace_bytes(2048, 1024, 1024, C.byref(need)), "2^31")
    _refused(lib, lib.t2fit_components_workspace_bytes(65536, 65536, 1, C.byref(need)), "2^31")


def test_label_refusals_before_hip(lib):
    p, q, ws = C.c_void_p(4096), C.c_void_p(8192), C.c_void_p(1 << 20)
    n = C.c_int32(0)
    big = 1 << 20
    call = lib.t2fit_components_label_dev
    _refused(lib, call(None, _abi.MORPH_U8, 4, 4, 4, 1, q, C.byref(n), ws, big, None), "NULL")
    _refused(lib, call(p, _abi.MORPH_U8, 4, 4, 4, 1, None, C.byref(n), ws, big, None), "NULL")
    _refused(lib, call(p, _abi.MORPH_F32, 4, 4, 4, 1, q, C.byref(n), ws, big, None), "in_type")
    _refused(lib, call(p, 7, 4, 4, 4, 1, q, C.byref(n), ws, big, None), "in_type")
    _refused(lib, call(p, _abi.MORPH_U8, 0, 4, 4, 1, q, C.byref(n), ws, big, None), "positive")
    _refused(lib, call(p, _abi.MORPH_U8, 2048, 1024, 1024, 1, q, C.byref(n), ws, big, None), "2^31")
    for c in (0, 4, -1):
        _refused(lib, call(p, _abi.MORPH_U8, 4, 4, 4, c, q, C.byref(n), ws, big, None), "connectivity")
    _refused(lib, call(p, _abi.MORPH_U8, 4, 4, 4, 1, C.c_void_p(8194), C.byref(n), ws, big, None), "aligned to 4")
    _refused(lib, call(C.c_void_p(4097), _abi.MORPH_I32, 4, 4, 4, 1, q, C.byref(n), ws, big, None), "aligned to 4")
    _refused(lib, call(q, _abi.MORPH_I32, 4, 4, 4, 1, q, C.byref(n), ws, big, None), "must not be in_dev")
    _refused(lib, call(p, _abi.MORPH_U8, 4, 4, 4, 1, q, C.byref(n), None, big, None), "workspace_dev is NULL")
    _refused(lib, call(p, _abi.MORPH_U8, 4, 4, 4, 1, q, C.byref(n), C.c_void_p((1 << 20) + 64), big, None), "aligned to 256")
    _refused(lib, call(p, _abi.MORPH_U8, 4, 4, 4, 1, q, C.byref(n), ws, 511, None), "511", "512")


def test_stats_refusals_before_hip(lib):
    p, s, b = C.c_void_p(4096), C.c_void_p(8192), C.c_void_p(16384)
    call = lib.t2fit_components_stats_dev
    _refused(lib, call(None, 4, 4, 4, 3, s, b, s, None), "NULL")
    _refused(lib, call(p, 4, 0, 4, 3, s, b, s, None), "positive")
    _refused(lib, call(p, 65536, 65536, 1, 3, s, b, s, None), "2^31")
    _refused(lib, call(p, 4, 4, 4, -1, s, b, s, None), "negative")
    _refused(lib, call(p, 4, 4, 4, 3, C.c_void_p(8196), b, s, None), "aligned")
    _refused(lib, call(p, 4, 4, 4, 3, s, C.c_void_p(16386), s, None), "aligned")
    assert call(p, 4, 4, 4, 3, None, None, None, None) == _abi.OK  # nothing asked for: nothing launched


def test_lut_refusals_before_hip(lib):
    s, t = C.c_void_p(8192), C.c_void_p(16384)
    k = C.c_int32(0)
    call = lib.t2fit_components_lut_dev
    _refused(lib, call(None, 3, 0, 0, 0, 0, t, C.byref(k), None), "NULL")
    _refused(lib, call(s, 3, 0, 0, 0, 0, None, C.byref(k), None), "NULL")
    _refused(lib, call(s, -1, 0, 0, 0, 0, t, C.byref(k), None), "n is negative")
    _refused(lib, call(s, 3, -1, 0, 0, 0, t, C.byref(k), None), "negative")
    _refused(lib, call(s, 3, 0, -5, 0, 0, t, C.byref(k), None), "negative")
    _refused(lib, call(s, 3, 0, 0, 2, 0, t, C.byref(k), None), "0 or 1")
    _refused(lib, call(s, 3, 0, 0, 0, -1, t, C.byref(k), None), "0 or 1")
    _refused(lib, call(C.c_void_p(8196), 3, 0, 0, 0, 0, t, C.byref(k), None), "aligned")


def test_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(REPO, "include", "t2fit.h")).read()
    names = {n for n, _, _ in _abi.SYMBOLS}
    assert len(_abi.COMPONENT_SYMBOLS) == 4
    for sym in _abi.COMPONENT_SYMBOLS:
        assert sym in names and sym + "(" in header and sym in _abi.LOOKED_UP and sym not in _abi.ADDITIVE
        assert hasattr(lib, sym) and getattr(lib, sym).argtypes is not None
    assert lib.t2fit_abi_version() == 5 and "#define T2FIT_ABI_VERSION 5" in header
    assert _abi.ADDITIVE == _abi.BOOT_SYMBOLS + _abi.TV_SYMBOLS + _abi.RECON_SYMBOLS + _abi.MORPH_SYMBOLS and len(_abi.ADDITIVE) == 15
    from fetal_t2mapping_amd import build

    assert any(src.endswith("t2fit_components.hip") for src in build.SOURCES)


def test_the_namespace_and_the_python_refusals():
    import fetal_t2mapping_amd as pkg
    from fetal_t2mapping_amd import _gpu_components, t2map

    assert t2map.components is _gpu_components is pkg.components and t2map.components.TILE == _components.TILE
    for name in ("label", "stats", "lut", "select", "keep_largest", "remove_small", "seeds"):
        assert callable(getattr(t2map.components, name))
    assert "components" not in pkg.__all__ and "scipy" not in open(_components.__file__).read().split('"""', 2)[2]
    assert "import scipy" not in open(_gpu_components.__file__).read()
