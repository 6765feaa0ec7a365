"""The non-rigid alignment's device half (csrc/t2fit_ffd.hip: t2fit_ffd_joint_hist_dev, t2fit_ffd_gradient_dev,
t2fit_ffd_warp_dev, t2fit_ffd_jacobian_dev) against its numpy statement (fetal_t2mapping_amd/_ffd.py): histogram integer
for integer, gradient, warp and Jacobian bit for bit, on shapes chosen against the kernels' tile (64 lanes along x, four
rows, one plane), shapes with more tiles than the histogram's launch has workgroups, the register tests' cases, every
lattice side and four bin pairs; masks that empty tiles or everything; lattices that push the volume outside; the zero
lattice against the existing device calls; raw calls on a second stream with a guarded workspace and offset outputs;
tensors as input; the whole registration, the atlas stage and recon.py.  tests/test_ffd_host.py covers what needs no
device."""
import ctypes as C
import sys

import numpy as np
import pytest

import atlas_cases as AC
import ffd_cases as FC
import register_cases as K
from fetal_t2mapping_amd import _atlas
from fetal_t2mapping_amd import _ffd as F
from fetal_t2mapping_amd import _register as G
from fetal_t2mapping_amd import _resample as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def t2():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X")
    import fetal_t2mapping_amd as t2

    return t2


def _assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64, (what, got.shape, want.shape)
    diff = np.flatnonzero(K.bits(got) != K.bits(want))
    assert diff.size == 0, (what, diff[:8], got.ravel()[diff[:8]], want.ravel()[diff[:8]])


def _check_metric(t2, what, bins, moving, a, fmask, mmask, phi, n_f, n_m, lo_m, scale_m, table=None):
    """Histogram and gradient of one case against the statement, each call made twice."""
    kw = dict(fixed_mask=fmask, moving_mask=mmask)
    got = t2.register.ffd_joint_histogram(bins, moving, a, phi, n_f, n_m, lo_m, scale_m, **kw)
    want = F.joint_histogram(bins, moving, a, phi, n_f, n_m, lo_m, scale_m, fmask, mmask)
    assert got.dtype == np.uint64 and got.shape == (n_f, n_m)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, bad[:8], got[got != want][:8], want[got != want][:8])
    assert got.tobytes() == t2.register.ffd_joint_histogram(bins, moving, a, phi, n_f, n_m, lo_m, scale_m, **kw).tobytes()
    table = FC.normal_table(n_f, n_m) if table is None else table
    grad = t2.register.ffd_gradient(bins, table, moving, a, phi, n_m, lo_m, scale_m, **kw)
    _assert_bits(grad, F.gradient(bins, table, moving, a, phi, n_m, lo_m, scale_m, fmask, mmask), what)
    assert grad.tobytes() == t2.register.ffd_gradient(bins, table, moving, a, phi, n_m, lo_m, scale_m, **kw).tobytes()
    return got, grad


def _check_warp_and_jacobian(t2, what, moving, a, fmask, phi, shape):
    w = t2.register.ffd_warp(moving, a, phi, shape, default=-7.5)
    assert w.dtype == np.float32 and w.tobytes() == F.warp(moving, a, phi, shape, default=-7.5).tobytes(), what
    assert w.tobytes() == t2.register.ffd_warp(moving, a, phi, shape, default=-7.5).tobytes()
    lab = (np.arange(moving.size, dtype=np.int64).reshape(moving.shape) % 251 - 100).astype(np.int32)
    n = t2.register.ffd_warp(lab, a, phi, shape, interp="nearest", default=-2)
    assert n.dtype == np.int32 and np.array_equal(n, F.warp(lab, a, phi, shape, interp="nearest", default=-2)), what
    assert np.array_equal(n, t2.register.ffd_warp(lab, a, phi, shape, interp="nearest", default=-2))
    got, want = t2.register.ffd_min_jacobian(phi, fmask), F.min_jacobian(phi, fmask)
    assert K.bits(got[0]) == K.bits(want[0]) and got[1] == want[1] and isinstance(got[1], int), (what, got, want)
    assert got == t2.register.ffd_min_jacobian(phi, fmask)


# ---- 1. shapes against the tile, every side ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FC.TILE_SHAPES + (FC.MANY_ROWS,))
def test_tile_edges_at_every_side(t2, shape):
    bins, moving, a, fmask, mmask = FC.shaped(shape)
    lo_m, scale_m = G.moving_bin_range(moving, mmask, 32)
    for i, side in enumerate(FC.SIDES):
        phi = FC.lattice(side, i, 1.2)
        n_f, n_m = FC.BIN_PAIRS[i % len(FC.BIN_PAIRS)]
        lo, sc = (lo_m, scale_m) if n_m == 32 else G.moving_bin_range(moving, mmask, n_m)
        hist, _ = _check_metric(t2, f"{shape} side {side}", bins, moving, a, fmask, mmask, phi, n_f, n_m, lo, sc)
        assert hist.any()
        _check_warp_and_jacobian(t2, f"{shape} side {side}", moving, a, fmask, phi, shape)


@pytest.mark.parametrize("shape", FC.CAPPED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_histogram_of_more_tiles_than_workgroups(t2, shape):
    """2210, 8840 and 2100 tiles under the 2048 workgroups of the histogram's launch: a workgroup stages T1 of another
    plane and T2 of another row on its second (up to fifth) trip, and its table gathers them all before its one flush."""
    bins, moving, a, fmask, mmask = FC.shaped(shape, cover=True)
    for i, side in enumerate((4, 19)):
        # (the statement alone: the tiles past the first trip hold voxels that count)
        assert FC.check_capped(shape, side) == {(130, 65, 5): 130 * 17, (520, 65, 5): 520 * 17, (2100, 1, 3): 2100}[shape]
        n_f, n_m = FC.BIN_PAIRS[i]
        lo_m, scale_m = G.moving_bin_range(moving, mmask, n_m)
        hist, _ = _check_metric(t2, f"{shape} side {side}", bins, moving, a, fmask, mmask, FC.lattice(side, 0, 1.2), n_f, n_m, lo_m, scale_m)
        assert hist.any()
    if shape == (130, 65, 5):  # the zero lattice: the affine histogram's kernel, capped the same way over its bricks
        kw = dict(fixed_mask=fmask, moving_mask=mmask)
        want = t2.register.joint_histogram(bins, moving, a, n_f, n_m, lo_m, scale_m, **kw)
        got = t2.register.ffd_joint_histogram(bins, moving, a, np.zeros((3, 4, 4, 4)), n_f, n_m, lo_m, scale_m, **kw)
        assert got.tobytes() == want.tobytes() and want.any()
        assert np.array_equal(want, G.joint_histogram(bins, moving, a, n_f, n_m, lo_m, scale_m, fmask, mmask))


# ---- 2. the register tests' cases, four bin pairs, the metric's own table ------------------------------------------------------
@pytest.mark.parametrize("name", FC.NAMED)
def test_named_cases_and_bin_pairs(t2, name):
    for i, (n_f, n_m) in enumerate(FC.BIN_PAIRS):
        bins, moving, a, fmask, mmask, lo_m, scale_m = FC.named(name, n_f, n_m)
        side = (7, 5, 11, 4)[i]
        phi = FC.lattice(side, i, 3.0 if name == "outside" else 1.0)  # 'outside': the lattice pushes more of the volume out
        hist, grad = _check_metric(t2, f"{name} {n_f} x {n_m}", bins, moving, a, fmask, mmask, phi, n_f, n_m, lo_m, scale_m)
        assert hist.any() == (name != "nothing")
        if name == "nothing":  # a transform that leaves nothing: zeros
            assert grad.tobytes() == np.zeros((3, side, side, side)).tobytes()
        elif n_f == 32:  # the table the loop uses
            table = G.mattes_metric(hist, n_f, n_m, scale_m)[1]
            _check_metric(t2, f"{name} metric table", bins, moving, a, fmask, mmask, phi, n_f, n_m, lo_m, scale_m, table)
        if i == 0:
            _check_warp_and_jacobian(t2, name, moving, a, fmask, phi, bins.shape)
    if name == "outside":
        inside = F.warp(np.ones_like(moving), a, phi, bins.shape, default=0.0)
        assert 0 < np.count_nonzero(inside) < inside.size


def test_masks_that_empty_tiles_and_an_empty_mask(t2):
    bins, moving, a, fmask, mmask, lo_m, scale_m = FC.named("prime", 32, 32)
    phi = FC.lattice(7, 9)
    holes = fmask.copy()
    holes[3:9], holes[:, 4:12], holes[12:, :, 20:] = 0, 0, 0  # whole planes, whole groups of four rows, the ends of rows
    _check_metric(t2, "holes", bins, moving, a, holes, mmask, phi, 32, 32, lo_m, scale_m)
    none = np.zeros_like(fmask)
    hist, grad = _check_metric(t2, "empty", bins, moving, a, none, mmask, phi, 32, 32, lo_m, scale_m)
    assert not hist.any() and grad.tobytes() == np.zeros((3, 7, 7, 7)).tobytes()
    assert t2.register.ffd_min_jacobian(phi, none) == (float("inf"), 0)
    fixed, moving, g, fmask, mmask, _, _ = FC.phantom()
    with pytest.raises(ValueError, match="empty"):
        t2.register.register_ffd(fixed, moving, g, g, affine=np.eye(4), fixed_mask=np.zeros_like(fmask), moving_mask=mmask)
    with pytest.raises(ValueError, match="no voxel"):  # masks that do not meet under the transform
        far = np.eye(4)
        far[0, 3] = 500.0
        t2.register.register_ffd(fixed, moving, g, g, affine=far, fixed_mask=fmask, moving_mask=mmask)


def test_non_finite_nodes_and_the_folding_lattice(t2):
    _, moving, a, fmask, _ = K.case("integer")  # Inf and NaN in the moving volume, whole-voxel shifts
    shape = fmask.shape
    for phi in (np.zeros((3, 4, 4, 4)), FC.lattice(5, 2, 0.6)):
        w = t2.register.ffd_warp(moving, a, phi, shape)
        assert w.tobytes() == F.warp(moving, a, phi, shape).tobytes()
    assert not np.all(np.isfinite(w))
    phi, mask = FC.folding_lattice(), np.ones((6, 6, 6), np.uint8)
    mask[0, :2, :3] = 0
    got = t2.register.ffd_min_jacobian(phi, mask)
    assert got == F.min_jacobian(phi, mask) and got[0] < 0.0 and got[1] == 210


# ---- 3. the zero lattice against the existing device calls -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["prime", "outside"])
def test_zero_lattice_equals_the_affine_calls_byte_for_byte(t2, name):
    bins, moving, a, fmask, mmask, lo_m, scale_m = FC.named(name, 32, 32)
    want = t2.register.joint_histogram(bins, moving, a, 32, 32, lo_m, scale_m, fixed_mask=fmask, moving_mask=mmask)
    for phi in (None, np.zeros((3, 4, 4, 4)), np.zeros((3, 19, 19, 19))):
        got = t2.register.ffd_joint_histogram(bins, moving, a, phi, 32, 32, lo_m, scale_m, fixed_mask=fmask, moving_mask=mmask)
        assert got.tobytes() == want.tobytes()
        assert t2.register.ffd_min_jacobian(phi, fmask) == (1.0, int(0))
    fg, mg = R.Geometry(bins.shape[::-1]), R.Geometry(moving.shape[::-1])  # unit grids: the index affine is the transform
    t = np.eye(4)
    t[:3] = np.asarray(a, np.float64).reshape(3, 4)
    assert np.array_equal(R.index_affine(fg, mg, t), np.asarray(a, np.float64).reshape(3, 4))
    lab = (moving > 400).astype(np.int32) * 9
    for phi in (None, np.zeros((3, 7, 7, 7))):
        assert t2.register.ffd_warp(moving, a, phi, bins.shape).tobytes() == t2.resample_volume(moving, mg, like=fg, transform=t)[0].tobytes()
        assert (t2.register.ffd_warp(lab, a, phi, bins.shape, interp="nearest", default=-1).tobytes()
                == t2.resample_volume(lab, mg, like=fg, transform=t, interp="nearest", default=-1)[0].tobytes())


# ---- 4. raw calls: a second stream, a workspace of 0xFF, offset outputs, guard words ---------------------------------------------
def _shifted(arr, offset, fill):
    import torch

    raw = np.ascontiguousarray(arr).view(np.uint8).ravel()
    buf = torch.full((raw.size + offset + 16,), fill, dtype=torch.uint8, device="cuda")
    buf[offset:offset + raw.size] = torch.from_numpy(raw).cuda()
    return buf, buf.data_ptr() + offset


def _guarded(nbytes, offset, fill=0x5A, guard=512):
    """A buffer of ``nbytes`` that starts ``offset`` bytes past a 256-byte boundary, with guard bytes on both sides:
    ``(tensor, pointer, index of the first byte)``."""
    import torch

    buf = torch.full((guard + 256 + offset + nbytes + guard,), fill, dtype=torch.uint8, device="cuda")
    at = (buf.data_ptr() + guard + 255) // 256 * 256 + offset - buf.data_ptr()
    return buf, buf.data_ptr() + at, at


def test_raw_calls_on_a_second_stream_keep_to_their_outputs(t2):
    import torch

    from fetal_t2mapping_amd import _gpu_ffd
    from fetal_t2mapping_amd._lib import load

    lib = load()
    name, n_f, n_m, side = "fixed_9x6x65", 7, 9, 5
    bins, moving, a, fmask, mmask, lo_m, scale_m = FC.named(name, n_f, n_m)
    shape, phi, table = bins.shape, FC.lattice(side, 6), FC.normal_table(n_f, n_m)
    need = C.c_size_t(0)
    assert lib.t2fit_ffd_workspace_bytes(*shape, side, C.byref(need)) == 0 and need.value == _gpu_ffd.workspace_bytes(shape, side)
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)
    A = (C.c_double * 12)(*np.asarray(a).ravel())
    n_out = int(np.prod(shape))
    with torch.cuda.stream(stream):
        (_, m_ptr), (_, b_ptr), (_, fm_ptr), (_, mm_ptr) = keep = (_shifted(moving, 4, 0xFF), _shifted(bins, 1, 0xFF),
                                                                   _shifted(fmask, 3, 0xFF), _shifted(mmask, 5, 0xFF))
        lat, tab = torch.from_numpy(phi).cuda(), torch.from_numpy(table.ravel()).cuda()
        ws, ws_ptr, ws_at = _guarded(need.value, 0, fill=0xFF)
        hist, h_ptr, h_at = _guarded(8 * n_f * n_m, 8)   # garbage: the call zeroes it
        grad, g_ptr, g_at = _guarded(8 * 3 * side ** 3, 8)
        out, o_ptr, o_at = _guarded(4 * n_out, 4)
        jac, j_ptr, j_at = _guarded(16, 8)
        geo = (fm_ptr, *shape, m_ptr, mm_ptr, *moving.shape)
        for _ in range(2):  # a second call into the same buffers: the same bytes
            assert lib.t2fit_ffd_joint_hist_dev(b_ptr, *geo, A, lat.data_ptr(), side, n_f, n_m, lo_m, scale_m, h_ptr, ws_ptr, need.value, st) == 0
        assert lib.t2fit_ffd_gradient_dev(b_ptr, tab.data_ptr(), n_f, n_m, lo_m, scale_m, *geo, A, lat.data_ptr(), side, g_ptr, ws_ptr,
                                          need.value, st) == 0
        assert lib.t2fit_ffd_warp_dev(m_ptr, 0, *moving.shape, A, lat.data_ptr(), side, o_ptr, *shape, 0, -1.0, ws_ptr, need.value, st) == 0
        assert lib.t2fit_ffd_jacobian_dev(lat.data_ptr(), side, fm_ptr, *shape, j_ptr, j_ptr + 8, ws_ptr, need.value, st) == 0
    stream.synchronize()
    del keep

    def payload(buf, at, nbytes, fill=0x5A):
        host = buf.cpu().numpy()
        assert np.all(host[:at] == fill) and np.all(host[at + nbytes:] == fill)  # the guard words
        return host[at:at + nbytes]

    assert np.array_equal(payload(hist, h_at, 8 * n_f * n_m).view(np.uint64).reshape(n_f, n_m),
                          F.joint_histogram(bins, moving, a, phi, n_f, n_m, lo_m, scale_m, fmask, mmask))
    _assert_bits(payload(grad, g_at, 8 * 3 * side ** 3).view(np.float64).reshape(3, side, side, side),
                 F.gradient(bins, table, moving, a, phi, n_m, lo_m, scale_m, fmask, mmask), "raw gradient")
    assert payload(out, o_at, 4 * n_out).tobytes() == F.warp(moving, a, phi, shape, default=-1.0).tobytes()
    got = payload(jac, j_at, 16)
    want = F.min_jacobian(phi, fmask)
    assert K.bits(got.view(np.float64)[0]) == K.bits(want[0]) and int(got.view(np.int64)[1]) == want[1]
    payload(ws, ws_at, need.value, fill=0xFF)

    # every refusal comes before a launch: the outputs keep their bytes
    buffers = (hist, grad, out, jac, ws)
    before = [t.clone() for t in buffers]
    FC.check_refusals(lib, b_ptr, tab.data_ptr(), fm_ptr, m_ptr, mm_ptr, lat.data_ptr(), h_ptr, g_ptr, m_ptr, o_ptr, j_ptr, ws_ptr, shape,
                      moving.shape, a, side, n_f, n_m, st)
    torch.cuda.synchronize()
    for t, was in zip(buffers, before):
        assert t.cpu().numpy().tobytes() == was.cpu().numpy().tobytes()


def test_tensors_as_input(t2):
    import torch

    bins, moving, a, fmask, mmask, lo_m, scale_m = FC.named("prime", 32, 32)
    phi, table = FC.lattice(7, 8), FC.normal_table(32, 32)
    d = [torch.from_numpy(v).cuda() for v in (bins, moving, fmask, mmask)]
    hist = t2.register.ffd_joint_histogram(d[0], d[1], a, phi, 32, 32, lo_m, scale_m, fixed_mask=d[2], moving_mask=d[3])
    assert np.array_equal(hist, F.joint_histogram(bins, moving, a, phi, 32, 32, lo_m, scale_m, fmask, mmask))
    grad = t2.register.ffd_gradient(d[0], table, d[1], a, phi, 32, lo_m, scale_m, fixed_mask=d[2], moving_mask=d[3])
    _assert_bits(grad, F.gradient(bins, table, moving, a, phi, 32, lo_m, scale_m, fmask, mmask), "tensors")
    w = t2.register.ffd_warp(d[1], a, phi, bins.shape)
    assert torch.is_tensor(w) and w.is_cuda and w.cpu().numpy().tobytes() == F.warp(moving, a, phi, bins.shape).tobytes()
    assert t2.register.ffd_min_jacobian(phi, d[2]) == F.min_jacobian(phi, fmask)


# ---- 5. the whole registration, the atlas stage, recon.py -----------------------------------------------------------------------
def test_register_ffd_equals_the_statement(t2):
    fixed, moving, g, fmask, mmask, _, _ = FC.phantom()
    want = FC.phantom_ffd()
    got = t2.register.register_ffd(fixed, moving, g, g, affine=FC.phantom_affine(), fixed_mask=fmask, moving_mask=mmask)
    assert got.lattice.tobytes() == want.lattice.tobytes() and got.iterations == want.iterations and got.stops == want.stops
    assert K.bits(got.cost) == K.bits(want.cost) and K.bits(got.min_jacobian) == K.bits(want.min_jacobian)
    assert got.n_folded == want.n_folded == 0 and got.affine is FC.phantom_affine()


def test_atlas_labels_nonrigid_equal_the_statement(t2):
    subject, template, g, mask, atlases, _ = AC.atlas_case()
    opts = {"max_iter": 5}
    want = _atlas.atlas_labels(subject, g, template, g, atlases, mask=mask, nonrigid=opts)
    warped, labels, found = t2.atlas.atlas_labels(subject, g, template, g, atlases, mask=mask, nonrigid=opts)
    assert type(found) is F.FFDRegistration and found.lattice.tobytes() == want[2].lattice.tobytes()
    assert found.parameters.tobytes() == want[2].parameters.tobytes() and found.iterations == want[2].iterations == (5, 5, 5)
    assert warped.dtype == np.float32 and warped.tobytes() == want[0].tobytes()
    for name in ("ho", "jhu"):
        assert labels[name].dtype == np.int32 and np.array_equal(labels[name], want[1][name])
    plain = t2.atlas.atlas_labels(subject, g, template, g, atlases, mask=mask)  # without the keyword: the affine stage alone
    assert type(plain[2]) is G.Registration and plain[0].tobytes() == AC.atlas_statement()[0].tobytes() != warped.tobytes()


def test_recon_atlas_nonrigid_on_the_device(t2, tmp_path, monkeypatch):
    import fake_sitk

    fake = fake_sitk.install()
    monkeypatch.setitem(sys.modules, "SimpleITK", fake)
    from fetal_t2mapping_amd import cli, recon

    bids, md, template_path, specs = AC.write_atlas_subject(tmp_path)
    written = recon.process_atlas_labels(md, bids, template_path, specs, nonrigid={"max_iter": 3}, write_warp=True)
    assert len(written) == 6
    t = AC.check_atlas_files(fake, bids, md, cli)
    warp = np.load([p for p in written if p.endswith(".npz")][0])
    assert np.array_equal(warp["transform"], t) and warp["lattice"].shape == (3, 7, 7, 7) and np.abs(warp["lattice"]).max() > 0.0
    assert int(warp["n_folded"]) == 0 and 0.0 < float(warp["min_jacobian"]) < 1.0
