"""The distance transform on the device (csrc/t2fit_edt.hip) against the numpy statement (fetal_t2mapping_amd/_edt.py):
every bit of d2 (inf included) and every index, for both site conventions, over the shapes, site densities and spacings
of tests/edt_cases.py, the two traps of the tie rule, no site and all sites, one output only, raw calls into guarded
caller-owned buffers, repeatability, inputs of every kind, and what is built on it -- edt, fill_nearest, the balls in
millimetres, the surface distances, reassign_small, segment_em(min_island=) and the tissue dict of atlas_labels.  The
recon.py flag is tested as far as its parsing (test_edt_drivers_host.py): no existing GPU test drives the tissue route
through recon.py, so that route is not short; from there on the keyword tested here is what runs.  Every call is one
that must succeed."""
import ctypes as C

import numpy as np
import pytest

import edt_cases as K
from fetal_t2mapping_amd import _abi, _edt, _morph, _seg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dist():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X")
    from fetal_t2mapping_amd import t2map

    return t2map.distance


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(got, want, what=""):
    """(d2, index) equal in every bit and of the statement's dtypes."""
    assert got[0].dtype == np.float64 and got[1].dtype == np.int32 and got[0].shape == want[0].shape, what
    assert np.array_equal(_bits(got[0]), _bits(want[0])), what
    assert np.array_equal(got[1], want[1]), what


# ---- d2 and index ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("density", K.DENSITIES)
@pytest.mark.parametrize("shape", K.DEVICE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_the_statement(dist, shape, density):
    a = K.sites(shape, density)
    for invert in (0, 1):
        vol = K.as_input(a, invert)
        for spacing in K.DEVICE_SPACINGS:
            _same(dist.nearest(vol, invert, spacing), K.statement(shape, density, invert, spacing), (invert, spacing))


@pytest.mark.parametrize("name", list(K.traps()))
def test_tie_traps(dist, name):
    a, query, want = K.traps()[name]
    for invert in (0, 1):
        vol = K.as_input(a, invert)
        d2, index = dist.nearest(vol, invert)
        assert index[query] == K.linear(a.shape, want) and d2[query] == (2.0 if name == "scan_order" else 25.0)
        _same((d2, index), _edt.nearest(vol, invert))


def test_no_site_and_all_sites(dist):
    for shape in ((1, 1, 1), (3, 70, 66), (2, 3, 300)):
        zeros, ones = np.zeros(shape, np.uint8), np.ones(shape, np.uint8)
        for vol, invert in ((zeros, 0), (ones, 1)):  # no site
            d2, index = dist.nearest(vol, invert, (4.5, 1.0, 1.0))
            assert d2.dtype == np.float64 and np.all(d2 == np.inf) and np.all(index == -1)
        for vol, invert in ((ones, 0), (zeros, 1)):  # every voxel a site
            d2, index = dist.nearest(vol, invert, (0.8, 1.1, 1.0))
            assert np.all(d2 == 0.0) and not np.signbit(d2).any() and np.array_equal(index.reshape(-1), np.arange(vol.size))
        assert np.all(dist.edt(ones) == np.inf)


def test_inputs_of_every_kind(dist):
    import torch

    shape = (3, 130, 67)
    a = K.sites(shape, "sparse")
    want = K.statement(shape, "sparse", 0, K.UNIT)
    for vol in (a, a.astype(bool), a * 200, a.astype(np.int32) * -7, a.astype(np.float32) * 0.5):
        got = dist.nearest(vol)
        assert isinstance(got[0], np.ndarray) and isinstance(got[1], np.ndarray)
        _same(got, want)
    for vol in (torch.from_numpy(a), torch.from_numpy(a).cuda(), torch.from_numpy(a.astype(bool)).cuda(),
                torch.from_numpy(a.astype(np.int32) * 5).cuda()):
        d2, index = dist.nearest(vol, False, None)
        assert d2.is_cuda and index.is_cuda and d2.dtype == torch.float64 and index.dtype == torch.int32
        _same((_np(d2), _np(index)), want)
    with pytest.raises(ValueError, match="3-D"):
        dist.nearest(a[0])
    with pytest.raises(ValueError, match="spacing"):
        dist.nearest(a, False, (1.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="invert"):
        dist.nearest(a, 2)


def test_twice_gives_identical_bytes(dist):
    for shape, density, spacing in (((70, 5, 129), "half", K.UNIT), ((3, 130, 67), "sparse", (0.8, 1.1, 1.0)),
                                    ((40, 40, 40), "corner", (4.5, 1.0, 1.0))):
        a = K.sites(shape, density)
        first, second = dist.nearest(a, 0, spacing), dist.nearest(a, 0, spacing)
        assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()


# ---- raw calls ---------------------------------------------------------------------------------------------------------------
GUARD = 4096


class _Guarded:
    """`nbytes` device bytes that start `offset` bytes past a 256-byte boundary, inside a buffer filled with 0xA5."""

    def __init__(self, nbytes, offset=0, content=None):
        import torch

        self.buf = torch.full((nbytes + 2 * GUARD + 512,), 0xA5, dtype=torch.uint8, device="cuda")
        self.at = GUARD + (offset - self.buf.data_ptr() - GUARD) % 256
        self.ptr, self.nbytes = self.buf.data_ptr() + self.at, nbytes
        assert self.ptr % 256 == offset
        if content is not None:
            raw = np.ascontiguousarray(content).view(np.uint8).ravel()
            assert raw.size == nbytes
            self.buf[self.at:self.at + nbytes] = torch.from_numpy(raw.copy()).cuda()

    def bytes(self):
        """The content, after checking that nothing was written before or after it."""
        host = self.buf.cpu().numpy()
        assert np.all(host[:self.at] == 0xA5) and np.all(host[self.at + self.nbytes:] == 0xA5)
        return host[self.at:self.at + self.nbytes].copy()


@pytest.mark.parametrize("shape,density", [((3, 130, 67), "sparse"), ((2, 3, 600), "half"), ((5, 7, 9), "corner")],
                         ids=["rows-shared", "row-longer-than-a-workgroup", "tiny"])
def test_raw_calls_with_caller_owned_buffers(dist, shape, density):
    import torch

    from fetal_t2mapping_amd._lib import load

    lib = load()
    a = K.sites(shape, density)
    n = a.size
    spacing = (1.25, 0.5, 0.5)
    s = (C.c_double * 3)(*spacing)
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)
    need = C.c_size_t(0)
    assert lib.t2fit_edt_workspace_bytes(*shape, C.byref(need)) == _abi.OK
    with torch.cuda.stream(stream):
        vol = _Guarded(n, 3, a)  # a uint8 volume needs no alignment
        for invert in (0, 1):
            want_d2, want_index = K.statement(shape, density, 0, spacing) if not invert else _edt.nearest(a, 1, spacing)
            for which in ("both", "d2", "index"):  # a NULL output is not written and the other is what it was
                d2, index, ws = _Guarded(8 * n, 8), _Guarded(4 * n, 4), _Guarded(need.value)  # the workspace exactly as asked for
                assert lib.t2fit_edt_dev(vol.ptr, invert, *shape, s, d2.ptr if which != "index" else None,
                                         index.ptr if which != "d2" else None, ws.ptr, ws.nbytes, st) == _abi.OK
                stream.synchronize()
                ws.bytes()
                if which != "index":
                    assert np.array_equal(d2.bytes(), _bits(want_d2).ravel()), (invert, which)
                else:
                    assert np.all(d2.bytes() == 0xA5)
                if which != "d2":
                    assert np.array_equal(index.bytes().view(np.int32), want_index.ravel()), (invert, which)
                else:
                    assert np.all(index.bytes() == 0xA5)
        assert np.array_equal(vol.bytes(), a.ravel())  # the input is as it was
        # NULL spacing is 1
        d2, index, ws = _Guarded(8 * n, 8), _Guarded(4 * n, 4), _Guarded(need.value)
        assert lib.t2fit_edt_dev(vol.ptr, 0, *shape, None, d2.ptr, index.ptr, ws.ptr, ws.nbytes, st) == _abi.OK
        stream.synchronize()
        unit = K.statement(shape, density, 0, K.UNIT)
        assert np.array_equal(d2.bytes(), _bits(unit[0]).ravel()) and np.array_equal(index.bytes().view(np.int32), unit[1].ravel())
        # the fill
        rng = np.random.default_rng(5)
        labels = rng.integers(-3, 9, n).astype(np.int32)
        where = (rng.random(n) < 0.5).astype(np.uint8) * 3
        lab, wh, out = _Guarded(4 * n, 4, labels), _Guarded(n, 1, where), _Guarded(4 * n, 4)
        assert lib.t2fit_edt_fill_dev(lab.ptr, wh.ptr, index.ptr, n, out.ptr, st) == _abi.OK
        stream.synchronize()
        assert np.array_equal(out.bytes().view(np.int32), _edt.fill_nearest(labels, where, unit[1].ravel()))
        assert np.array_equal(lab.bytes().view(np.int32), labels)


# ---- what is built on it -------------------------------------------------------------------------------------------------------

def test_edt_is_scipys_convention(dist):
    import torch

    shape = (3, 130, 67)
    m = K.as_input(K.sites(shape, "sparse"), 1)  # a mask with 1 % zeros
    for spacing in (None, (4.5, 1.0, 1.0), (0.8, 1.1, 1.0)):
        want = K.statement(shape, "sparse", 1, K.UNIT if spacing is None else spacing)
        root = np.sqrt(want[0])
        got = dist.edt(m, spacing)
        assert got.dtype == np.float64 and np.all(np.abs(got - root) <= np.spacing(root))
        assert np.array_equal(dist.edt(m, spacing, squared=True), want[0])
        d, index = dist.edt(torch.from_numpy(m).cuda(), spacing, return_indices=True)
        assert d.is_cuda and np.array_equal(_np(index), want[1]) and np.all(np.abs(_np(d) - root) <= np.spacing(root))


def test_fill_nearest(dist):
    import torch

    rng = np.random.default_rng(8)
    shape = (3, 9, 70)
    labels = rng.integers(0, 5, shape)
    where = rng.random(shape) < 0.4
    _, index = _edt.nearest(labels, 0)
    index = index.copy()
    index[0, 0, :5] = -1
    want = _edt.fill_nearest(labels, where, index)
    got = dist.fill_nearest(labels, where, index)
    assert got.dtype == np.int32 and got.shape == shape and np.array_equal(got, want) and (want != labels).any()
    got = dist.fill_nearest(torch.from_numpy(labels.astype(np.int32)).cuda(), torch.from_numpy(where).cuda(), torch.from_numpy(index).cuda())
    assert got.is_cuda and got.dtype == torch.int32 and np.array_equal(_np(got), want)


@pytest.mark.parametrize("r", (1, 2, 3))
def test_balls_in_millimetres(dist, r):
    from fetal_t2mapping_amd import t2map

    m = K.blobs()
    grown, shrunk = dist.dilate_mm(m, r + 0.5), dist.erode_mm(m, r + 0.5)
    assert grown.dtype == shrunk.dtype == np.uint8
    assert np.array_equal(grown, _edt.dilate_mm(m, r + 0.5)) and np.array_equal(shrunk, _edt.erode_mm(m, r + 0.5)) and shrunk.any()
    assert np.array_equal(grown, _np(t2map.binary_dilate(m, _morph.ball(r))))
    assert np.array_equal(shrunk, _np(t2map.binary_erode(m, _morph.ball(r), border_value=1)))
    for spacing in ((4.5, 1.0, 1.0), (0.8, 1.1, 1.0)):
        assert np.array_equal(dist.dilate_mm(m, 2.0 * r, spacing), _edt.dilate_mm(m, 2.0 * r, spacing))
        assert np.array_equal(dist.erode_mm(m, 1.0 * r, spacing), _edt.erode_mm(m, 1.0 * r, spacing))
    big = dist.dilate_mm(m, 40.0)  # beyond the run-list footprints' radius of 32
    assert big.all()


def test_surface_distances(dist):
    import torch

    shape = (15, 16, 24)
    a, b = K.ball_mask(shape, (7, 7, 8), 5), K.ball_mask(shape, (7, 7, 12), 5)
    assert np.array_equal(dist.surface(a), _edt.surface(a)) and np.array_equal(dist.surface(K.blobs()), _edt.surface(K.blobs()))
    for spacing in (None, (4.5, 1.0, 1.0), (1.25, 0.5, 0.5)):
        want = _edt.surface_distances(a, b, spacing)
        got = dist.surface_distances(a, b, spacing)
        assert got["n_a"] == want["n_a"] and got["n_b"] == want["n_b"]
        # every gathered value is a square root within one spacing of numpy's (test_edt_is_scipys_convention); the maximum
        # keeps that bound, the percentile's interpolation and the pairwise sum of n values add at most log2(n) roundings
        assert abs(got["hausdorff"] - want["hausdorff"]) <= np.spacing(want["hausdorff"])
        slack = (2 + np.log2(want["n_a"] + want["n_b"])) * 2.0 ** -52
        for key in ("hd95", "assd"):
            assert abs(got[key] - want[key]) <= slack * want[key], key
    got = dist.surface_distances(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    assert got["hausdorff"] == 4.0
    with pytest.raises(ValueError, match="empty"):
        dist.surface_distances(a, np.zeros(shape, np.uint8))


def test_reassign_small(dist):
    import torch

    from fetal_t2mapping_amd import t2map

    c, island = K.slab()
    for vol in (c, c.astype(np.int64), c.astype(np.uint8), torch.from_numpy(c).cuda()):
        for min_size in (island, island + 1, 10**6, 0):
            for kw in ({}, {"connectivity": 3, "spacing": (4.5, 1.0, 1.0)}):
                got, changed = t2map.components.reassign_small(vol, min_size, **kw)
                want, n_want = _edt.reassign_small(c, min_size, **kw)
                assert got.is_cuda and got.dtype == torch.int32 and changed == n_want and np.array_equal(_np(got), want)
    assert t2map.components.reassign_small(c, island + 1)[1] == 2 * island
    rng = np.random.default_rng(2)
    noisy = rng.integers(0, 4, (6, 20, 70)).astype(np.int32)  # many islands of many sizes
    got, changed = t2map.components.reassign_small(noisy, 4, 2)
    want, n_want = _edt.reassign_small(noisy, 4, 2)
    assert changed == n_want > 0 and np.array_equal(_np(got), want)
    with pytest.raises(ValueError, match="negative"):
        t2map.components.reassign_small(c, -1)


def test_segment_em_min_island(dist):
    import seg_cases as SC

    from fetal_t2mapping_amd import t2map

    y, mask, _, atlas = SC.phantom()
    cl = SC.PHANTOM_CLASSES
    prior = t2map.seg.priors_from_labels(atlas, cl)
    kw = dict(n_iter=3, beta=0.0)
    plain = t2map.seg.segment_em(y, mask, prior, cl, **kw)
    zero = t2map.seg.segment_em(y, mask, prior, cl, min_island=0, **kw)
    assert plain.n_reassigned == 0 and zero.n_reassigned == 0 and np.array_equal(plain.labels, zero.labels)
    assert _seg.SegResult._fields == ("labels", "model", "s0_trace", "n_iter", "posteriors", "n_reassigned")
    want, changed = _edt.reassign_small(plain.labels, 20)
    res = t2map.seg.segment_em(y, mask, prior, cl, min_island=20, **kw)
    assert changed > 0 and res.n_reassigned == changed and res.labels.dtype == np.int32 and np.array_equal(res.labels, want)
    assert np.array_equal(res.s0_trace, plain.s0_trace)


def test_atlas_labels_passes_min_island_on(dist):
    import atlas_cases as AC

    from fetal_t2mapping_amd import t2map

    subject, template, g, mask, atlases, _ = AC.atlas_case()
    classes = [int(v) for v in np.unique(atlases["ho"])[1:]]
    kw = dict(mask=mask, levels=(4,), max_iter=3)
    tissue = {"labels": atlases["ho"], "classes": classes, "channels": [subject, 0.7 * subject], "n_iter": 2, "beta": 0.0}
    plain = t2map.atlas.atlas_labels(subject, g, template, g, atlases, tissue=tissue, **kw)[3]
    out = t2map.atlas.atlas_labels(subject, g, template, g, atlases, tissue=dict(tissue, min_island=6), **kw)[3]
    want, changed = _edt.reassign_small(plain["labels"], 6)
    assert plain["n_reassigned"] == 0 and out["n_reassigned"] == changed and np.array_equal(out["labels"], want)
