"""Connected components on the device (csrc/t2fit_components.hip) against the numpy statement
(fetal_t2mapping_amd/_components.py), element for element: the labelling on every case and connectivity of
tests/components_cases.py, the statistics, the selection table, select / keep_largest / remove_small / seeds, raw calls
with caller-owned guarded buffers, repeatability, the mask keywords, and recon.py --phantom_find_seeds on a small
synthetic phantom.  Every call is one that must succeed."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import components_cases as K
from fetal_t2mapping_amd import _abi, _components, _register

pytestmark = pytest.mark.gpu

MASKS = K.mask_cases()
CLASSES = K.class_cases()


@pytest.fixture(scope="module")
def cc():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X")
    from fetal_t2mapping_amd import t2map

    return t2map.components


def _np(t):
    return t.cpu().numpy()


# ---- the labelling ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("connectivity", K.CONNECTIVITIES)
@pytest.mark.parametrize("index", range(len(MASKS)), ids=[name for name, _ in MASKS])
def test_masks(cc, index, connectivity):
    import torch

    a = MASKS[index][1]
    want, n_want = K.statement("mask", index, connectivity)
    got, n = cc.label(a, connectivity)
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == a.shape
    assert n == n_want and np.array_equal(_np(got), want)


@pytest.mark.parametrize("connectivity", K.CONNECTIVITIES)
@pytest.mark.parametrize("index", range(len(CLASSES)), ids=[name for name, _ in CLASSES])
def test_classes(cc, index, connectivity):
    a = CLASSES[index][1]
    want, n_want = K.statement("classes", index, connectivity)
    got, n = cc.label(a, connectivity)
    assert n == n_want and np.array_equal(_np(got), want)
    got64, n64 = cc.label(a.astype(np.int64) * 3 - (a != 0), connectivity)  # other values, another dtype: the same partition
    assert n64 == n_want and np.array_equal(_np(got64), want)


def test_inputs_of_every_kind(cc):
    import torch

    a = K.random_mask(K.MID, 0.31, seed=4)
    want, n_want = _components.label(a, 2)
    for vol in (a, a.astype(bool), a * 200, torch.from_numpy(a), torch.from_numpy(a).cuda(), torch.from_numpy(a.astype(bool)).cuda()):
        got, n = cc.label(vol, 2)
        assert n == n_want and np.array_equal(_np(got), want)
    # int32 ones are classes with a single class: the same components
    got, n = cc.label(torch.from_numpy(a.astype(np.int32)).cuda(), 2)
    assert n == n_want and np.array_equal(_np(got), want)
    with pytest.raises(ValueError, match="connectivity"):
        cc.label(a, 0)
    with pytest.raises(ValueError, match="3-D"):
        cc.label(a[0])
    with pytest.raises(ValueError, match="integer"):
        cc.label(a.astype(np.float32))


def test_twice_gives_identical_bytes(cc):
    for a, c in ((K.random_mask(K.BIG, 0.31, seed=1), 1), (K.random_mask(K.BIG, 0.2, seed=1), 3), (K.random_classes(K.BIG), 2),
                 (K.comb(K.BIG), 1)):
        first, n1 = cc.label(a, c)
        second, n2 = cc.label(a, c)
        assert n1 == n2 and np.array_equal(_np(first).view(np.uint8), _np(second).view(np.uint8))
        s1, s2 = cc.stats(first, n1), cc.stats(second, n2)
        for x, y in zip(s1, s2):
            assert np.array_equal(_np(x).view(np.uint8), _np(y).view(np.uint8))


# ---- statistics, tables, the operations built from them ------------------------------------------------------------------

ALL_CASES = [("mask", i) for i in range(len(MASKS))] + [("classes", i) for i in range(len(CLASSES))]
ALL_IDS = [name for name, _ in MASKS] + [name for name, _ in CLASSES]


@pytest.mark.parametrize("connectivity", K.CONNECTIVITIES)
@pytest.mark.parametrize("kind,index", ALL_CASES, ids=ALL_IDS)
def test_stats(cc, kind, index, connectivity):
    import torch

    lab, n = K.statement(kind, index, connectivity)
    want = _components.stats(lab, n)
    got = cc.stats(np.asarray(lab), n)
    assert [t.dtype for t in got] == [torch.int64, torch.int32, torch.int64]
    for g, w in zip(got, want):
        assert tuple(g.shape) == w.shape and np.array_equal(_np(g), w)


def test_stats_of_any_label_volume(cc):
    lab = np.array([[[0, 1, 5, -3], [1, 7, 3, 3]]], np.int32)
    for n in (3, 0, 9):
        for g, w in zip(cc.stats(lab, n), _components.stats(lab, n)):
            assert np.array_equal(_np(g), w)
    # a volume in which one wave sees many labels, and labels that come back after another one
    rng = np.random.default_rng(11)
    lab = rng.integers(-1, 70, (3, 9, 150)).astype(np.int32)
    lab[1] = 4
    lab[2, :, ::2] = 6
    for n in (69, 20):
        for g, w in zip(cc.stats(lab, n), _components.stats(lab, n)):
            assert np.array_equal(_np(g), w)
    for shape, top in (((7, 9, 5), 4), ((1, 1, 1), 1), ((2, 3, 64), 2), ((5, 1, 63), 40)):  # rows shorter than a wave, and as long
        lab = rng.integers(0, top + 1, shape).astype(np.int32)
        for g, w in zip(cc.stats(lab, top), _components.stats(lab, top)):
            assert np.array_equal(_np(g), w), shape
    big = np.full((8, 64, 130), 2, np.int64)  # int64 in, coordinate sums beyond 2^31 / 64
    for g, w in zip(cc.stats(big, 2), _components.stats(big, 2)):
        assert np.array_equal(_np(g), w)


@pytest.mark.parametrize("largest", [False, True])
@pytest.mark.parametrize("renumber", [False, True])
def test_lut(cc, largest, renumber):
    rng = np.random.default_rng(3)
    tables = [np.array([100, 5, 9, 9, 1, 30, 30, 2], np.int64), np.array([7], np.int64), np.array([0, 4], np.int64),
              np.array([3, 0, 6, 0, 6], np.int64), rng.integers(0, 50, 1025).astype(np.int64), rng.integers(0, 9, 3000).astype(np.int64)]
    for sizes in tables:
        for min_size, max_size in ((0, 0), (1, 0), (2, 9), (9, 9), (10, 29), (31, 0), (0, 5), (1000, 0)):
            want, kept_want = _components.lut(sizes, min_size, max_size, largest, renumber)
            got, kept = cc.lut(sizes, min_size=min_size, max_size=max_size, largest=largest, renumber=renumber)
            assert kept == kept_want and np.array_equal(_np(got), want), (sizes.size, min_size, max_size)
    with pytest.raises(ValueError, match="negative"):
        cc.lut(tables[0], min_size=-1)


SELECTIONS = ({}, {"min_size": 2}, {"min_size": 2, "max_size": 30, "renumber": True}, {"largest": True},
              {"largest": True, "renumber": True, "max_size": 24})


@pytest.mark.parametrize("connectivity", K.CONNECTIVITIES)
@pytest.mark.parametrize("kind,index", ALL_CASES, ids=ALL_IDS)
def test_select_keep_largest_remove_small_seeds(cc, kind, index, connectivity):
    """The statement's results are composed here from its cached labelling, as _components composes them."""
    import torch

    c = connectivity
    a = (MASKS if kind == "mask" else CLASSES)[index][1]
    lab, n = K.statement(kind, index, c)
    sizes = _components.stats(lab, n)[0]
    dev_lab = torch.from_numpy(np.asarray(lab)).cuda()
    for kw in SELECTIONS:
        table, kept = _components.lut(sizes, **kw)
        assert np.array_equal(_np(cc.select(dev_lab, n, **kw)), table[lab]), kw
        got_table, got_kept = cc.lut(sizes, **kw)
        assert got_kept == kept and np.array_equal(_np(got_table), table), kw
    got = cc.remove_small(a, 3, c)
    kept3 = _components.lut(sizes, 3)[0][lab] != 0
    if kind == "classes":
        assert got.dtype == torch.int32 and np.array_equal(_np(got), np.where(kept3, a, 0))
        return
    assert got.dtype == torch.uint8 and np.array_equal(_np(got), kept3.astype(np.uint8))
    for k in (1, 3):
        got = cc.keep_largest(a, k, c)
        assert got.dtype == torch.uint8 and np.array_equal(_np(got), (_components.largest_lut(sizes, k)[lab] != 0).astype(np.uint8))
    for lo, hi in ((1, 0), (2, 40)):
        picked = _components.select(lab, n, lo, hi, renumber=True)
        s2, _, sums2 = _components.stats(picked, int(picked.max(initial=0)))
        assert cc.seeds(a, c, lo, hi) == [[int(v) for v in row] for row in _components.centroids(s2, sums2)]


def test_the_composed_operations_of_the_statement(cc):
    """keep_largest, remove_small and seeds as _components itself computes them, on one volume per kind."""
    a, c = K.random_mask(K.MID, 0.31, seed=6), K.random_classes(K.MID)
    for conn in K.CONNECTIVITIES:
        for k in (1, 3):
            assert np.array_equal(_np(cc.keep_largest(a, k, conn)), _components.keep_largest(a, k, conn))
        assert np.array_equal(_np(cc.remove_small(a, 3, conn)), _components.remove_small(a, 3, conn))
        assert np.array_equal(_np(cc.remove_small(c, 3, conn)), _components.remove_small(c, 3, conn))
        assert cc.seeds(a, conn, 2, 40) == _components.seeds(a, conn, 2, 40) and cc.seeds(a, conn) == _components.seeds(a, conn)


def test_the_tie_and_the_classes(cc):
    import torch

    a = K.two_blobs()
    lab, n = cc.label(a)
    assert n == 4 and _np(cc.stats(lab, n)[0]).tolist() == [a.size - 61, 24, 12, 24, 1]
    assert np.array_equal(_np(cc.keep_largest(a)), (_np(lab) == 1).astype(np.uint8))  # 24 twice: the lower label
    assert np.array_equal(_np(cc.keep_largest(a, 2)), np.isin(_np(lab), (1, 3)).astype(np.uint8))
    assert cc.seeds(a, min_size=12) == _components.seeds(a, min_size=12) and len(cc.seeds(a, min_size=12)) == 3
    c = K.random_classes(K.BIG)
    got = cc.remove_small(c, 4, 2)
    want = _components.remove_small(c, 4, 2)
    assert got.dtype == torch.int32 and np.array_equal(_np(got), want) and (want != c).any() and (want != 0).any()
    assert cc.seeds(np.zeros((3, 4, 5), np.uint8)) == []


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


@pytest.mark.parametrize("kind", ["mask", "classes"])
def test_raw_calls_with_caller_owned_buffers(cc, kind):
    import torch

    from fetal_t2mapping_amd._lib import load

    lib = load()
    a = K.random_mask(K.BIG, 0.31, seed=2) if kind == "mask" else K.random_classes(K.BIG)
    shape, n_vox = a.shape, a.size
    conn = 2
    want, n_want = _components.label(a, conn)
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)
    need = C.c_size_t(0)
    assert lib.t2fit_components_workspace_bytes(*shape, C.byref(need)) == _abi.OK
    with torch.cuda.stream(stream):
        inp = _Guarded(a.nbytes, 1 if kind == "mask" else 4, a)
        lab, ws = _Guarded(4 * n_vox, 4), _Guarded(need.value)  # the workspace exactly as long as the call asks for
        in_type = _abi.MORPH_U8 if kind == "mask" else _abi.MORPH_I32
        n = C.c_int32(-1)
        # without n_out the call does not wait; the count is in the first word of the workspace
        assert lib.t2fit_components_label_dev(inp.ptr, in_type, *shape, conn, lab.ptr, None, ws.ptr, ws.nbytes, st) == _abi.OK
        stream.synchronize()
        assert np.array_equal(lab.bytes().view(np.int32).reshape(shape), want)
        assert int(ws.bytes()[:4].view(np.int32)[0]) == n_want
        assert lib.t2fit_components_label_dev(inp.ptr, in_type, *shape, conn, lab.ptr, C.byref(n), ws.ptr, ws.nbytes, st) == _abi.OK
        assert n.value == n_want  # the call has waited
        assert np.array_equal(lab.bytes().view(np.int32).reshape(shape), want)
        assert np.array_equal(inp.bytes(), a.view(np.uint8).ravel())  # the input is as it was
        # statistics: every subset of the outputs
        sizes_w, bbox_w, sums_w = _components.stats(want, n_want)
        rows = n_want + 1
        for mask in range(1, 8):
            sizes, bbox, sums = _Guarded(8 * rows, 8), _Guarded(24 * rows, 4), _Guarded(24 * rows, 8)
            assert lib.t2fit_components_stats_dev(lab.ptr, *shape, n_want, sizes.ptr if mask & 1 else None, bbox.ptr if mask & 2 else None,
                                                  sums.ptr if mask & 4 else None, st) == _abi.OK
            stream.synchronize()
            assert np.array_equal(sizes.bytes().view(np.int64), sizes_w) or not mask & 1
            assert np.array_equal(bbox.bytes().view(np.int32).reshape(rows, 6), bbox_w) or not mask & 2
            assert np.array_equal(sums.bytes().view(np.int64).reshape(rows, 3), sums_w) or not mask & 4
            for buf, used in ((sizes, mask & 1), (bbox, mask & 2), (sums, mask & 4)):
                assert used or np.all(buf.bytes() == 0xA5)
        # the table, applied by t2fit_relabel_dev in place
        sizes = _Guarded(8 * rows, 8, sizes_w)
        table = _Guarded(4 * rows, 4)
        kept = C.c_int32(-1)
        assert lib.t2fit_components_lut_dev(sizes.ptr, n_want, 3, 0, 0, 1, table.ptr, C.byref(kept), st) == _abi.OK
        table_w, kept_w = _components.lut(sizes_w, 3, 0, False, True)
        assert kept.value == kept_w and 0 < kept_w < n_want and np.array_equal(table.bytes().view(np.int32), table_w)
        assert lib.t2fit_components_lut_dev(sizes.ptr, n_want, 0, 0, 1, 0, table.ptr, None, st) == _abi.OK
        stream.synchronize()
        assert np.array_equal(table.bytes().view(np.int32), _components.lut(sizes_w, largest=True)[0])
        assert lib.t2fit_relabel_dev(lab.ptr, n_vox, table.ptr, rows, lab.ptr, st) == _abi.OK
        stream.synchronize()
        assert np.array_equal(lab.bytes().view(np.int32).reshape(shape), _components.select(want, n_want, largest=True))


# ---- the mask keywords -----------------------------------------------------------------------------------------------------

def test_build_mask_and_phantom_mask_keywords(cc):
    from fetal_t2mapping_amd import t2map

    vol, _ = K.phantom()
    plain = _np(t2map.build_mask(vol))
    assert np.array_equal(plain, _register.build_mask(vol))
    assert np.array_equal(_np(t2map.build_mask(vol, keep_largest=0, min_size=0, connectivity=2)), plain)  # the defaults: today's bytes
    for kw in ({"keep_largest": 1}, {"keep_largest": 2, "connectivity": 3}, {"min_size": 20}, {"min_size": 20, "keep_largest": 3}):
        got = _np(t2map.build_mask(vol, **kw))
        assert np.array_equal(got, _register.build_mask(vol, **kw)), kw
        assert 0 < got.sum() < plain.sum()
    assert np.array_equal(_np(t2map.build_mask(vol, keep_largest=1)), _components.keep_largest(plain))
    small = vol[:, :24, :40]
    pm = _np(t2map.phantom_mask(small, 100, 3, 2))
    assert np.array_equal(_np(t2map.phantom_mask(small, 100, 3, 2, keep_largest=1)), _components.keep_largest(pm))
    assert np.array_equal(_np(t2map.phantom_mask(small, 100, 3, 2, min_size=30, connectivity=3)), _components.remove_small(pm, 30, 3))
    with pytest.raises(ValueError, match="negative"):
        t2map.build_mask(vol, keep_largest=-1)


# ---- recon.py --phantom_find_seeds, on files -------------------------------------------------------------------------------

def test_recon_phantom_find_seeds(cc, tmp_path, monkeypatch):
    import pandas as pd

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import fake_sitk

    monkeypatch.setitem(sys.modules, "SimpleITK", fake_sitk.install())
    from fetal_t2mapping_amd import _morph, cli, recon

    bids = str(tmp_path / "projects") + "/"
    vol, centres = K.phantom()
    rows = []
    for i, te in enumerate((114, 202)):
        acq = {"prj": "prj-901", "sub": "sub-001", "ses": "ses-01", "run": f"run-{i + 1:02d}", "EchoTime": te / 1000.0,
               "CoilString": "HeadNeck", "ImageOrientationPatientSTR": "ax"}
        rows.append(acq)
        np.save(cli.get_img_path(bids, acq, cli.recon_dirname).replace(" ", "") + ".npy", (vol * (1.0 if i == 0 else 0.1)).astype(np.float32))
    md = pd.DataFrame(rows)
    out = str(tmp_path / "seeds.json")
    args = recon.parse_arguments(["--path", str(tmp_path), "--csv", "x.csv", "--in_vitro", "--lf", "--phantom_masks", "--phantom_find_seeds", out,
                                  "--phantom_vial_window", "500,2000", "--phantom_vial_size", "10,0"])
    assert recon.process_find_seeds(md, bids, args.phantom_find_seeds, fixed=args.fixed, device=args.device, **args.find_seeds) == [out]
    seeds = recon.load_seeds(out)
    assert sorted(seeds) == sorted(centres)  # the known centres of the vials
    assert seeds == _components.seeds(_morph.erode(vol >= 500, _morph.ball(2)), 1, 10, 0) == json.load(open(out))
    # the labels painted at the proposal are the ones painted at the centres, up to the order of the vials
    from fetal_t2mapping_amd import t2map

    a = _np(t2map.phantom_labels(vol.shape, seeds, 3)) != 0
    b = _np(t2map.phantom_labels(vol.shape, centres, 3)) != 0
    assert np.array_equal(a, b) and a.any()
