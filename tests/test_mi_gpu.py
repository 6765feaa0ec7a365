"""Mattes mutual information's device half (csrc/t2fit_register.hip: t2fit_register_joint_hist_dev,
t2fit_register_mi_gradient_dev) against its numpy statement (fetal_t2mapping_amd/_register.py): the joint histogram integer
for integer and the 12 gradient sums bit for bit on the named cases of the 43 sums at four bin pairs, histograms in which
every voxel hits the same entries, volumes with more bricks than the histogram's launch has workgroups, raw calls through
unaligned-but-legal pointers with a guarded workspace, the whole registration with 6 and 12 degrees of freedom, and every
refusal of the ABI.  tests/test_mi_host.py covers what needs no device."""
import ctypes as C

import numpy as np
import pytest

import atlas_cases as AC
import mi_cases as MC
import register_cases as K
from fetal_t2mapping_amd import _register as G

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
    assert diff.size == 0, (what, diff, got[diff], want[diff])


def _hist(t2, name, n_f, n_m):
    bins, moving, a, fmask, mmask = MC.inputs(name, n_f)
    lo_m, scale_m = MC.moving_range(name, n_m)
    return t2.register.joint_histogram(bins, moving, a, n_f, n_m, lo_m, scale_m, fixed_mask=fmask, moving_mask=mmask)


def _gradient(t2, name, n_f, n_m, kind):
    bins, moving, a, fmask, mmask = MC.inputs(name, n_f)
    lo_m, scale_m = MC.moving_range(name, n_m)
    return t2.register.mi_gradient_sums(bins, MC.table(name, n_f, n_m, kind), moving, a, n_m, lo_m, scale_m, fixed_mask=fmask,
                                        moving_mask=mmask)


# ---- 10. the histogram ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MC.GPU_CASES)
def test_joint_histogram_equals_the_statement_integer_for_integer(t2, name):
    for n_f, n_m in MC.BIN_PAIRS:
        got, want = _hist(t2, name, n_f, n_m), MC.statement_hist(name, n_f, n_m)
        assert got.dtype == np.uint64 and got.shape == (n_f, n_m)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (name, n_f, n_m, bad[:8], got[got != want][:8], want[got != want][:8])
        assert got.tobytes() == _hist(t2, name, n_f, n_m).tobytes()  # the same from call to call
        assert got.any() == (name != "nothing")
    if name == "tail257":
        assert G.pass_sizes(int(np.prod(G.brick_counts(MC.inputs(name, 1)[0].shape)))) == [257, 2]


@pytest.mark.parametrize("name", MC.CONTENTION)
def test_histograms_in_which_the_lanes_of_a_wave_meet(t2, name):
    """'constant': every voxel adds to the same four entries of its row; 'lanes': the 64 lanes of a wave hold 64 fixed
    bins; 'brick': a workgroup's voxels all hold one fixed bin."""
    for n_f, n_m in ((64, 64), (32, 32), (1, 5)) if name == "constant" else ((64, 64), (64, 9)):
        got, want = _hist(t2, name, n_f, n_m), MC.statement_hist(name, n_f, n_m)
        assert np.array_equal(got, want), (name, n_f, n_m)
        n = K.statement_sums("bricks")[0]
        assert abs(int(got.sum(dtype=np.uint64)) - int(n) * MC.ONE) <= 2 * int(n)
        if name == "constant":
            assert np.count_nonzero(got.sum(axis=0)) <= 4 and got.max() > 1000 * MC.ONE // 6
        else:
            assert np.count_nonzero(got.sum(axis=1)) > 32


@pytest.mark.parametrize("name", tuple(MC.CAPPED) + ("capped2_constant",))
def test_histogram_of_more_bricks_than_workgroups(t2, name):
    """2322 and 8514 bricks under the 2048 workgroups of the launch: a workgroup's table gathers two (up to five) bricks
    before its one flush.  'capped2_constant': every brick of a workgroup adds to the same four columns."""
    of = "capped2" if name == "capped2_constant" else name
    assert MC.check_capped(of) == {"capped2": 2322, "capped5": 8514}[of]  # (the statement alone: the late bricks count)
    n = MC.counted(name)
    for n_f, n_m in MC.BIN_PAIRS:
        got, want = _hist(t2, name, n_f, n_m), MC.statement_hist(name, n_f, n_m)
        assert got.dtype == np.uint64 and got.shape == (n_f, n_m)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (name, n_f, n_m, bad[:8], got[got != want][:8], want[got != want][:8])
        assert got.tobytes() == _hist(t2, name, n_f, n_m).tobytes()  # the same from call to call
        assert abs(int(got.sum(dtype=np.uint64)) - n * MC.ONE) <= 2 * n
        if name == "capped2_constant":
            assert np.count_nonzero(got.sum(axis=0)) <= 4 and got.max() > 1000 * MC.ONE // 6


# ---- 11. the gradient sums -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MC.GPU_CASES + ("tail774",))
def test_gradient_sums_are_bit_equal_to_the_statement(t2, name):
    for (n_f, n_m), kind in (((32, 32), "normal"), ((7, 9), "normal"), ((64, 64), "normal"), ((1, 5), "normal"), ((32, 32), "metric")):
        if name == "nothing" and kind == "metric":
            continue  # (no histogram, no table)
        got = _gradient(t2, name, n_f, n_m, kind)
        _assert_bits(got, MC.statement_gradient(name, n_f, n_m, kind), f"{name} {n_f} x {n_m} {kind}")
        assert got.tobytes() == _gradient(t2, name, n_f, n_m, kind).tobytes()
        if name == "nothing":
            assert got.tobytes() == np.zeros(12).tobytes()
    if name == "tail774":
        assert G.pass_sizes(int(np.prod(G.brick_counts(MC.inputs(name, 1)[0].shape)))) == [774, 4]


# ---- 12. raw calls: zeroing, garbage, unaligned-but-legal pointers, the guarded workspace ---------------------------------------
def _shifted(arr, offset, fill):
    """A device copy of ``arr`` that starts ``offset`` bytes into its buffer; returns ``(buffer, pointer)``."""
    import torch

    raw = np.ascontiguousarray(arr).view(np.uint8).ravel()
    buf = torch.full((raw.size + offset + 16,), fill, dtype=torch.uint8, device="cuda")
    buf[offset:offset + raw.size] = torch.from_numpy(raw).cuda()
    return buf, buf.data_ptr() + offset


def test_raw_calls_zero_the_histogram_take_unaligned_volumes_and_keep_to_the_workspace(t2):
    import torch

    from fetal_t2mapping_amd._lib import load

    lib = load()
    name, n_f, n_m = "fixed_9x6x65", 7, 9
    bins, moving, a, fmask, mmask = MC.inputs(name, n_f)
    lo_m, scale_m = MC.moving_range(name, n_m)
    want_h, table = MC.statement_hist(name, n_f, n_m), MC.table(name, n_f, n_m, "normal")
    need = C.c_size_t(0)
    assert lib.t2fit_register_mi_workspace_bytes(*bins.shape, C.byref(need)) == 0
    assert need.value == sum((12 * 8 * n + 255) // 256 * 256 for n in G.pass_sizes(int(np.prod(G.brick_counts(bins.shape)))))
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)
    A = (C.c_double * 12)(*np.asarray(a).ravel())
    guard = 4096
    with torch.cuda.stream(stream):
        # the float32 volume 4 bytes into its allocation, the byte volumes at odd offsets
        (_, m_ptr), (_, b_ptr), (_, fm_ptr), (_, mm_ptr) = keep = (_shifted(moving, 4, 0xFF), _shifted(bins, 1, 0xFF),
                                                                   _shifted(fmask, 3, 0xFF), _shifted(mmask, 5, 0xFF))
        hist = torch.full((n_f * n_m,), -0x0123456789ABCDEF, dtype=torch.int64, device="cuda")  # garbage: the call zeroes it
        tab = torch.from_numpy(table.ravel()).cuda()
        sums = torch.full((12,), np.nan, dtype=torch.float64, device="cuda")
        ws = torch.full((need.value + 256 + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        ws_ptr = (ws.data_ptr() + 255) // 256 * 256
        geo = (fm_ptr, *bins.shape, m_ptr, mm_ptr, *moving.shape)
        assert lib.t2fit_register_joint_hist_dev(b_ptr, *geo, A, n_f, n_m, lo_m, scale_m, hist.data_ptr(), st) == 0
        first = hist.clone()
        assert lib.t2fit_register_joint_hist_dev(b_ptr, *geo, A, n_f, n_m, lo_m, scale_m, hist.data_ptr(), st) == 0
        assert lib.t2fit_register_mi_gradient_dev(b_ptr, tab.data_ptr(), n_f, n_m, lo_m, scale_m, *geo, A, sums.data_ptr(), ws_ptr,
                                                  need.value, st) == 0
    stream.synchronize()
    del keep
    assert np.array_equal(first.cpu().numpy().view(np.uint64).reshape(n_f, n_m), want_h)
    assert first.cpu().numpy().tobytes() == hist.cpu().numpy().tobytes()  # a second call into the same buffer: the same bytes
    _assert_bits(sums.cpu().numpy(), MC.statement_gradient(name, n_f, n_m, "normal"), "raw gradient sums")
    at = ws_ptr - ws.data_ptr()
    host = ws.cpu().numpy()
    assert np.all(host[:at] == 0xA5) and np.all(host[at + need.value:] == 0xA5)  # nothing before or after the workspace
    assert np.any(host[at:at + need.value] != 0xA5)

    # ---- 14. every refusal comes before a launch: the outputs keep their bytes
    before = (hist.clone(), sums.clone(), ws.clone())
    MC.check_refusals(lib, b_ptr, tab.data_ptr(), fm_ptr, m_ptr, mm_ptr, hist.data_ptr(), sums.data_ptr(), ws_ptr, bins.shape, moving.shape,
                      a, n_f, n_m, st)
    torch.cuda.synchronize()
    for t, was in zip((hist, sums, ws), before):
        assert t.cpu().numpy().tobytes() == was.cpu().numpy().tobytes()


# ---- 13. the registration --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dof", [6, 12])
def test_register_affine_mattes_equals_the_statement(t2, dof):
    fixed, moving, g, fmask, mmask = AC.recovery_pair()
    want = MC.recovered(dof)
    got = t2.register.register_affine(fixed, moving, g, g, metric="mattes", dof=dof, fixed_mask=fmask, moving_mask=mmask)
    print(got, f"TRE {AC.tre(got.transform):.4f} mm")
    assert got.parameters.tobytes() == want.parameters.tobytes() and got.transform.tobytes() == want.transform.tobytes()
    assert got.iterations == want.iterations and got.stops == want.stops and got.metric == want.metric
    if dof == 12:
        assert AC.tre(got.transform) < AC.START_TRE / 4


def test_register_rigid_mattes_and_the_atlas_stage_equal_their_statements(t2):
    from fetal_t2mapping_amd import _atlas

    fixed, moving, g, fmask, mmask = MC.rigid_pair()
    kw = dict(fixed_mask=fmask, moving_mask=mmask, levels=(4, 2), max_iter=5, metric="mattes", bins=16, moving_bins=24)
    want, got = G.register_rigid(fixed, moving, g, g, **kw), t2.register.register_rigid(fixed, moving, g, g, **kw)
    assert got.parameters.shape == (6,) and got.parameters.tobytes() == want.parameters.tobytes() and got.iterations == want.iterations == (5, 5)
    assert got.transform.tobytes() == want.transform.tobytes()
    subject, template, ag, mask, atlases, _ = AC.atlas_case()
    akw = dict(mask=mask, metric="mattes", levels=(4,), max_iter=3)
    w_warped, w_labels, w_found = _atlas.atlas_labels(subject, ag, template, ag, atlases, **akw)
    warped, labels, found = t2.atlas.atlas_labels(subject, ag, template, ag, atlases, **akw)
    assert found.parameters.tobytes() == w_found.parameters.tobytes() and np.array_equal(warped.view(np.uint32), w_warped.view(np.uint32))
    assert all(np.array_equal(labels[n], w_labels[n]) for n in w_labels)
