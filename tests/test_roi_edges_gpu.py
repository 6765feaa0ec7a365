"""The ROI kernels of csrc/t2fit_roi.hip on the device, at the edges tests/test_roi_stats_gpu.py does not reach.  The
statistics are held to the numpy statement of tests/roi_cases.py bit for bit (no tolerance: the statement fixes the
segment order and the sum tree, and tests/test_roi_edges_host.py holds it to an exact reference): ragged volume sizes, the
257-unit volume whose scan is ragged, medians whose two ranks part in every pass, infinities, denormals and signed zeros,
labels outside 1..n_labels, raw calls on offset pointers into sentinel-guarded buffers on two streams, and the scratch
cache growing under queued kernels.  The erosion goes through its raw entry point against scipy's binary_erosion per label:
misaligned buffers at a vector-eligible width, 3 and 8 iterations, small and tile-edge shapes, 256 labels, and raw label
values that a narrowing to 16 bits would alias."""
import ctypes as C

import numpy as np
import pytest

import roi_cases as K

pytestmark = pytest.mark.gpu

SENTINEL = 0x5EA7C0DE
GUARD = 64  # sentinel words on each side of a payload

GROUPS = {"sizes": ("size-",), "parting": ("parting-",), "values": ("tree-", "non-finite", "edge-values"), "labels": ("labels-",)}


@pytest.fixture(scope="module")
def t2():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X")
    import fetal_t2mapping_amd as t2

    return t2


def _cases(group):
    found = [c for c in K.all_cases() if c.name.startswith(GROUPS[group])]  # the shared instances and their statements
    assert found and all(sum(c.name.startswith(p) for p in GROUPS.values()) == 1 for c in K.all_cases())  # no case is left out
    return found


def _lib():
    from fetal_t2mapping_amd._lib import load

    return load()


def _guarded(words, n_words=None, lead=1):
    """An int32 device buffer [lead words | GUARD sentinels | payload | GUARD sentinels], all sentinel but the payload
    when one is given.  The payload starts 4 * lead bytes past a 256-byte boundary: lead = 1 for 32-bit data, 2 for
    64-bit data, 0 for an aligned buffer.  Returns ``(buffer, payload pointer, payload slice)``."""
    import torch

    n = len(words) if words is not None else n_words
    buf = torch.full((lead + GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 256 == 0
    where = slice(lead + GUARD, lead + GUARD + n)
    if words is not None:
        buf[where] = torch.from_numpy(np.ascontiguousarray(words).view(np.int32).ravel()).cuda()
    ptr = buf.data_ptr() + 4 * (lead + GUARD)
    assert ptr % 256 == 4 * lead
    return buf, ptr, where


def _guarded64(n):
    """An output of n 64-bit elements 8 bytes past a 256-byte boundary between sentinel words."""
    return _guarded(None, 2 * n, lead=2)


def _payload(buf, where):
    """The payload of a guarded buffer after a call; everything around it must still be the sentinel."""
    host = buf.cpu().numpy()
    assert np.all(host[:where.start] == SENTINEL) and np.all(host[where.stop:] == SENTINEL), "written outside the payload"
    return host[where]


def _assert_equal(got, want, what, median=True):
    assert np.array_equal(got.count, want.count) and np.array_equal(got.valid, want.valid), what
    assert K.bits_equal(got.mean, want.mean), (what, "mean", got.mean, want.mean)
    assert K.bits_equal(got.std, want.std), (what, "std", got.std, want.std)
    if median:
        assert K.bits_equal(got.median, want.median), (what, "median", got.median, want.median)
    else:
        assert got.median is None


# ---- statistics -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_python_api_equals_the_statement(t2, group):
    """mean / std / median bit for bit in float64 (a NaN equals a NaN), count / valid exact: numpy arrays, CUDA tensors
    with an int32 and with an int64 roi, and once without the median."""
    import torch

    for c in _cases(group):
        want = K.expected(c)
        m, roi = c.map.reshape(c.shape), c.roi.reshape(c.shape)
        _assert_equal(t2.roi_stats(m, roi, c.n_labels), want, (c.name, "numpy"))
        md, rd = torch.from_numpy(m).cuda(), torch.from_numpy(roi).cuda()
        _assert_equal(t2.roi_stats(md, rd, c.n_labels), want, (c.name, "cuda int32"))
        _assert_equal(t2.roi_stats(md, rd.to(torch.int64), c.n_labels), want, (c.name, "cuda int64"))
        _assert_equal(t2.roi_stats(md, rd, c.n_labels, median=False), want, (c.name, "no median"), median=False)
        assert np.array_equal(md.cpu().numpy().view(np.uint32), m.view(np.uint32)) and np.array_equal(rd.cpu().numpy(), roi)


class _RawStats:
    """One call of t2fit_roi_stats_dev on guarded buffers: launched by the constructor, read (after a synchronise) by
    `read`, which also checks every guard and that the inputs are unchanged."""

    def __init__(self, lib, c, stream):
        self.c = c
        self.mbuf, mptr, self.mw = _guarded(c.map)
        self.rbuf, rptr, self.rw = _guarded(c.roi)
        self.outs = [_guarded64(c.n_labels) for _ in range(5)]
        self.lib, self.args = lib, (mptr, rptr, len(c.map), c.n_labels, *[ptr for _, ptr, _ in self.outs])
        self.stream = stream

    def launch(self):
        assert self.lib.t2fit_roi_stats_dev(*self.args, self.stream) == 0, self.lib.t2fit_last_error().decode()
        return self

    def read(self):
        assert np.array_equal(_payload(self.mbuf, self.mw), self.c.map.view(np.int32)), "map changed"
        assert np.array_equal(_payload(self.rbuf, self.rw), self.c.roi), "roi changed"
        mean, std, med, cnt, val = (np.ascontiguousarray(_payload(buf, where)) for buf, _, where in self.outs)
        return K.Stats(mean.view(np.float64), std.view(np.float64), med.view(np.float64), cnt.view(np.int64), val.view(np.int64), [])

    def reset(self):
        for buf, _, _ in self.outs:
            buf.fill_(SENTINEL)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_raw_calls_on_offset_pointers_and_two_streams(t2, group):
    """map and roi 4 bytes past a 256-byte boundary, the five outputs 8 bytes past one and between sentinels; on a stream
    of the caller's and on the current stream, twice each: the bits of the statement, nothing written outside, the inputs
    unchanged."""
    import torch

    lib = _lib()
    side = torch.cuda.Stream()
    for c in _cases(group):
        call = _RawStats(lib, c, None)
        for name, stream in (("side", side), ("current", torch.cuda.current_stream())):
            call.stream = C.c_void_p(stream.cuda_stream)
            for turn in range(2):
                call.reset()
                torch.cuda.synchronize()  # the buffers were filled on the current stream
                call.launch()
                torch.cuda.synchronize()
                _assert_equal(call.read(), K.expected(c), (c.name, name, turn))


def test_scratch_grows_under_queued_kernels_and_is_reused_with_stale_contents(t2):
    """Small, big, small on one stream without a synchronise in between (the second call replaces the stream's scratch
    while the first is queued; the third runs in a buffer full of the second's tables and segments), then the same on a
    second stream: every result is its statement."""
    import torch

    lib = _lib()
    small, big = K.case("size-65"), K.case(f"size-{257 * K.SPAN - 5}")
    for stream in (torch.cuda.Stream(), torch.cuda.Stream()):
        calls = [_RawStats(lib, c, C.c_void_p(stream.cuda_stream)) for c in (small, big, small)]
        torch.cuda.synchronize()
        for call in calls:
            call.launch()
        torch.cuda.synchronize()
        for i, call in enumerate(calls):
            _assert_equal(call.read(), K.expected(call.c), (call.c.name, i))


# ---- erosion ------------------------------------------------------------------------------------------------------------
def _blocky(rng, shape, block, lo, hi):
    """Random integers in [lo, hi) constant on blocks of `block` voxels per axis, cropped to `shape`."""
    small = tuple(-(-s // b) for s, b in zip(shape, block))
    a = rng.integers(lo, hi, small)
    for ax, b in enumerate(block):
        a = a.repeat(b, ax)
    return np.ascontiguousarray(a[: shape[0], : shape[1], : shape[2]]).astype(np.int32)


def _scipy(lab, tis, tv, n_labels, connectivity, iterations):
    """binary_erosion of (tissue == tv) & (label == L) per label L of 1..n_labels that occurs, as one class volume."""
    from scipy.ndimage import binary_erosion, generate_binary_structure

    out = np.zeros(lab.shape, np.int32)
    st = generate_binary_structure(3, connectivity)
    for L in np.unique(lab):
        if 1 <= L <= n_labels:
            mask = (lab == L) if tis is None else ((tis == tv) & (lab == L))
            out[binary_erosion(mask, structure=st, iterations=iterations)] = L
    return out


def _raw_erode(lab, tis, tv, n_labels, connectivity, iterations, leads=(0, 0, 0)):
    """t2fit_roi_erode_dev with label / tissue / roi_out placed 4 * lead bytes past a 256-byte boundary; the output (and
    the inputs) between sentinels, the inputs unchanged afterwards."""
    import torch

    lib = _lib()
    lbuf, lptr, lw = _guarded(lab.ravel(), lead=leads[0])
    tbuf, tptr, tw = _guarded(tis.ravel(), lead=leads[1]) if tis is not None else (None, None, None)
    obuf, optr, ow = _guarded(None, lab.size, lead=leads[2])
    assert [p % 16 for p in (lptr, optr)] == [4 * leads[0], 4 * leads[2]]
    rc = lib.t2fit_roi_erode_dev(lptr, tptr, tv if tis is not None else 0, *lab.shape, n_labels, connectivity, iterations, optr,
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.t2fit_last_error().decode()
    torch.cuda.synchronize()
    assert np.array_equal(_payload(lbuf, lw), lab.ravel())
    if tis is not None:
        assert np.array_equal(_payload(tbuf, tw), tis.ravel())
    return _payload(obuf, ow).reshape(lab.shape)


def test_erosion_scalar_path_at_a_vector_width(t2):
    """nx % 4 == 0 and one of label / tissue / roi_out 4 bytes past a 16-byte boundary: the scalar path, at a width that
    would take the vector one.  The bits of the aligned call and of scipy."""
    rng = np.random.default_rng(61)
    shape = (9, 17, 68)
    lab = _blocky(rng, shape, (3, 5, 7), 0, 5)
    lab[...] = np.where(rng.random(shape) < 0.7, 1, lab)
    tis = _blocky(rng, shape, (5, 9, 40), 2, 4)
    for connectivity, iterations in ((1, 1), (3, 1), (1, 2)):
        want = _scipy(lab, tis, 3, 4, connectivity, iterations)
        assert np.count_nonzero(want) > 20
        aligned = _raw_erode(lab, tis, 3, 4, connectivity, iterations)
        assert np.array_equal(aligned, want), (connectivity, iterations)
        for leads in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
            got = _raw_erode(lab, tis, 3, 4, connectivity, iterations, leads)
            assert got.tobytes() == aligned.tobytes(), (connectivity, iterations, leads)
    got = _raw_erode(lab, None, 0, 4, 3, 1, (1, 0, 0))  # without a tissue volume
    assert np.array_equal(got, _scipy(lab, None, 0, 4, 3, 1)) and got.any()


@pytest.mark.parametrize("shape", [(24, 40, 72), (23, 39, 71)])
def test_erosion_three_and_eight_iterations(t2, shape):
    """The ping-pong between roi_out and the scratch volume beyond two passes, up to the documented maximum, on the
    vector path (nx = 72) and the scalar one (nx = 71); a block of label 1 thick enough to outlast 8 passes."""
    rng = np.random.default_rng(62)
    lab = _blocky(rng, shape, (6, 8, 8), 2, 6)
    lab[2: shape[0] - 2, 3: shape[1] - 3, 4: shape[2] - 4] = 1
    tis = np.full(shape, 7, np.int32)
    tis[:, :, shape[2] - 6:] = 8  # cuts the block: tissue applies in the first pass only
    for connectivity in (1, 3):
        for iterations in (3, 8):
            want = _scipy(lab, tis, 7, 5, connectivity, iterations)
            assert np.count_nonzero(want == 1) > 100, "the reference keeps voxels"
            assert np.array_equal(_raw_erode(lab, tis, 7, 5, connectivity, iterations), want), (connectivity, iterations)
    assert np.array_equal(_raw_erode(lab, None, 0, 5, 2, 8, (1, 0, 1)), _scipy(lab, None, 0, 5, 2, 8))


@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 5, 1), (3, 3, 4), (8, 16, 64), (9, 17, 65), (16, 32, 128)])
def test_erosion_on_small_and_tile_edge_shapes(t2, shape):
    """Every voxel is labelled, so a region touches every face (out of volume is background)."""
    rng = np.random.default_rng(63)
    lab = _blocky(rng, shape, (4, 8, 16), 1, 5)
    tis = _blocky(rng, shape, (8, 16, 48), 2, 4)
    assert lab.min() >= 1
    for connectivity in (1, 2, 3):
        for iterations in (1, 2):
            for t, tv in ((None, 0), (tis, 3)):
                want = _scipy(lab, t, tv, 4, connectivity, iterations)
                got = _raw_erode(lab, t, tv, 4, connectivity, iterations)
                assert np.array_equal(got, want), (shape, connectivity, iterations, tv)
    if min(shape) < 3:
        assert not _raw_erode(lab, None, 0, 4, 1, 1).any()  # every voxel lies on a face
    if min(shape) >= 8:
        assert _scipy(lab, None, 0, 4, 3, 1).any()


def test_erosion_with_256_labels_and_labels_255_256_0_adjacent(t2):
    shape = (6, 8, 24)
    lab = np.zeros(shape, np.int32)
    lab[:, :, :8], lab[:, :, 8:16] = 255, 256
    for connectivity in (1, 2, 3):
        want = _scipy(lab, None, 0, 256, connectivity, 1)
        assert np.count_nonzero(want == 255) == 4 * 6 * 6 and np.count_nonzero(want == 256) == 4 * 6 * 6
        got = _raw_erode(lab, None, 0, 256, connectivity, 1)
        assert np.array_equal(got, want), connectivity
    # with 255 labels, 256 is background, for itself and for its neighbours
    got = _raw_erode(lab, None, 0, 255, 3, 1)
    assert np.array_equal(got, _scipy(np.where(lab == 256, 0, lab), None, 0, 255, 3, 1)) and set(np.unique(got)) == {0, 255}
    assert np.array_equal(t2.roi_erode(lab, labels=range(1, 257), connectivity=1).cpu().numpy(), _scipy(lab, None, 0, 256, 1, 1))


@pytest.mark.parametrize("n_labels", [1, 256])
def test_erosion_counts_out_of_range_label_values_as_background(t2, n_labels):
    """65537 (label 1 after a narrowing to 16 bits), 65536 + n_labels, -1, INT32_MIN, INT32_MAX and n_labels + 1 inside
    regions of label 1 (and of label n_labels): the neighbours erode exactly as scipy erodes with those voxels cleared."""
    shape = (8, 12, 16)
    lab = np.ones(shape, np.int32)
    if n_labels > 1:
        lab[:, :, 8:] = n_labels
    alien = [65537, 65536 + n_labels, -1, K.INT32_MIN, K.INT32_MAX, n_labels + 1]
    spots = [(2, 2, 2), (2, 9, 5), (5, 3, 3), (5, 9, 2), (3, 6, 6), (6, 6, 3)]
    for v, (z, y, x) in zip(alien, spots):
        lab[z, y, x] = v
        lab[z, y, x + 8] = v
    cleared = np.where((lab >= 1) & (lab <= n_labels), lab, 0).astype(np.int32)
    for connectivity in (1, 3):
        for iterations in (0, 1):
            want = _scipy(cleared, None, 0, n_labels, connectivity, iterations) if iterations else cleared
            got = _raw_erode(lab, None, 0, n_labels, connectivity, iterations)
            assert np.array_equal(got, want), (connectivity, iterations)
            assert iterations == 0 or (0 < np.count_nonzero(want) < np.count_nonzero(cleared) - 8 * len(alien))
    tis = np.where(lab == 1, 5, 6).astype(np.int32)  # the scalar path and the tissue test see the same values
    assert np.array_equal(_raw_erode(lab, tis, 5, n_labels, 3, 1, (1, 1, 1)), _scipy(cleared, tis, 5, n_labels, 3, 1))
