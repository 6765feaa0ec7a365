"""The correlation ratio's device half (csrc/t2fit_register.hip: t2fit_register_bin_dev, t2fit_register_binned_sums_dev,
t2fit_register_sums_lut_dev) against its numpy statement (fetal_t2mapping_amd/_register.py), bit for bit: the named
cases of the 43 sums at 1, 7 and 64 bins, bricks of one bin and waves of 64 bins, the binning rule at its edges, the
whole affine registration, raw calls on a caller's stream and every refusal of the ABI, and the atlas-label stage.
tests/test_atlas_host.py covers what needs no device."""
import ctypes as C

import numpy as np
import pytest

import atlas_cases as AC
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


def _check_case(t2, bins, moving, a, fmask, mmask, n_bins, want, what):
    w_binned, w_lut, w_sums = want
    binned, lut = t2.register.binned_sums(bins, moving, a, n_bins, fixed_mask=fmask, moving_mask=mmask, return_lut=True)
    again, lut2 = t2.register.binned_sums(bins, moving, a, n_bins, fixed_mask=fmask, moving_mask=mmask, return_lut=True)
    _assert_bits(binned, w_binned, what + " binned")
    _assert_bits(lut, w_lut, what + " lut")
    assert binned.tobytes() == again.tobytes() and lut.tobytes() == lut2.tobytes()
    sums = t2.register.registration_sums_lut(bins, lut, moving, a, fixed_mask=fmask, moving_mask=mmask)
    _assert_bits(sums, w_sums, what + " sums")
    assert sums.tobytes() == t2.register.registration_sums_lut(bins, lut, moving, a, fixed_mask=fmask, moving_mask=mmask).tobytes()
    return binned


@pytest.mark.parametrize("name", AC.SUMS_CASES)
@pytest.mark.parametrize("n_bins", AC.N_BINS)
def test_binned_sums_lut_and_sums_are_bit_equal_to_the_statement_and_repeat(t2, name, n_bins):
    _, moving, a, fmask, mmask = K.case(name)
    binned = _check_case(t2, AC.bins_of(name, n_bins), moving, a, fmask, mmask, n_bins, AC.statement(name, n_bins), f"{name} B={n_bins}")
    if name == "nothing":
        assert binned.tobytes() == np.zeros(2 * n_bins).tobytes()
    if name == "tail257":
        assert G.pass_sizes(int(np.prod(G.brick_counts(K.case(name)[0].shape)))) == [257, 2]
    if n_bins == 64 and binned[:64].sum() > 1000:  # the top bit of the presence word is in use
        assert binned[0] > 0 and binned[63] > 0


@pytest.mark.parametrize("kind", ["brick", "lanes"])
def test_bricks_of_one_bin_and_waves_of_64_bins(t2, kind):
    bins, moving, a, fmask, mmask = AC.layout_case(kind)
    if kind == "brick":
        per_brick = bins[:8, :4, :64]
        assert np.all(per_brick == per_brick[0, 0, 0]) and np.unique(bins).size > 32
    else:
        assert np.array_equal(bins[3, 5, :64], np.arange(64))
    binned = _check_case(t2, bins, moving, a, fmask, mmask, 64, AC.statement(kind, 64), kind)
    assert np.count_nonzero(binned[:64]) > 32 and binned[:64].sum() == K.statement_sums("bricks")[0]


def test_binning_is_bit_equal_to_the_statement(t2):
    rng = np.random.default_rng(61)
    v = rng.normal(400, 120, (7, 11, 13)).astype(np.float32)  # 1001 voxels: not a multiple of the workgroup
    v[0, 0, :4] = (np.nan, np.inf, -np.inf, -0.0)
    finite = v[np.isfinite(v)]
    lo, hi = float(finite.min()), float(finite.max())
    for n_bins in (1, 7, 32, 64):
        scale = n_bins / (hi - lo)
        got = t2.register.bin_volume(v, lo, scale, n_bins).cpu().numpy()
        assert got.dtype == np.uint8 and np.array_equal(got, G.bin_volume(v, lo, scale, n_bins))
        assert got.ravel()[np.argmax(np.where(np.isfinite(v), v, -np.inf))] == n_bins - 1  # f == hi clamps to B - 1
        assert got[0, 0, 0] == 0 and got[0, 0, 1] == n_bins - 1 and got[0, 0, 2] == 0 and got.max() == n_bins - 1
    assert not t2.register.bin_volume(v, 7.0, 0.0, 8).cpu().numpy().any()  # lo == hi: scale 0, all zeros
    # an unaligned length and pointer: a view 4 bytes into the buffer, raw call
    import torch

    from fetal_t2mapping_amd._lib import load

    flat = torch.from_numpy(v.ravel()).cuda()
    out = torch.full((flat.numel(),), 9, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert load().t2fit_register_bin_dev(flat.data_ptr() + 4, 999, lo, 32 / (hi - lo), 32, out.data_ptr() + 1, st) == 0
    got = out.cpu().numpy()
    assert np.array_equal(got[1:1000], G.bin_volume(v.ravel()[1:1000].reshape(1, 1, -1), lo, 32 / (hi - lo), 32).ravel())
    assert got[0] == 9 and got[1000] == 9


def test_register_affine_equals_the_statement_on_the_recovery_case(t2):
    fixed, moving, g, fmask, mmask = AC.recovery_pair()
    want = AC.recovered("cr", 12)
    got = t2.register.register_affine(fixed, moving, g, g, fixed_mask=fmask, moving_mask=mmask)
    print(got, f"TRE {AC.tre(got.transform):.4f} mm")
    assert got.parameters.tobytes() == want.parameters.tobytes() and got.transform.tobytes() == want.transform.tobytes()
    assert got.iterations == want.iterations and got.stops == want.stops and got.metric == want.metric
    assert AC.tre(got.transform) == AC.tre(want.transform) < AC.START_TRE / 4


def test_register_affine_ncc_and_fewer_degrees_equal_the_statement(t2):
    fixed, moving, g, fmask, mmask = AC.recovery_pair()
    for kw in (dict(metric="ncc", dof=12), dict(metric="cr", dof=7, bins=8), dict(metric="cr", dof=9, init="centroids")):
        kw.update(fixed_mask=fmask, moving_mask=mmask, levels=(4, 2), max_iter=6)
        want, got = G.register_affine(fixed, moving, g, g, **kw), t2.register.register_affine(fixed, moving, g, g, **kw)
        assert got.parameters.tobytes() == want.parameters.tobytes() and got.iterations == want.iterations == (6, 6)


def _ws(n_bytes):
    import torch

    ws = torch.full((n_bytes + 256,), 0xFF, dtype=torch.uint8, device="cuda")  # NaN bytes: an unwritten value shows
    return ws, (ws.data_ptr() + 255) // 256 * 256


def test_raw_calls_on_another_stream_and_every_refusal(t2):
    import torch

    from fetal_t2mapping_amd._lib import load

    lib = load()
    name, n_bins = "fixed_9x6x65", 7
    fixed, moving, a, fmask, mmask = K.case(name)
    w_binned, w_lut, w_sums = AC.statement(name, n_bins)
    need, need43 = C.c_size_t(0), C.c_size_t(0)
    assert lib.t2fit_register_binned_workspace_bytes(*fixed.shape, n_bins, C.byref(need)) == 0
    slabs = int(np.prod(G.brick_counts(fixed.shape)))
    assert need.value == sum((2 * n_bins * 8 * n + 255) // 256 * 256 for n in G.pass_sizes(slabs))
    assert lib.t2fit_register_workspace_bytes(*fixed.shape, C.byref(need43)) == 0
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)
    A = (C.c_double * 12)(*np.asarray(a).ravel())
    with torch.cuda.stream(stream):
        f, fm = torch.from_numpy(fixed).cuda(), torch.from_numpy(fmask).cuda()
        m, mm = torch.from_numpy(moving).cuda(), torch.from_numpy(mmask).cuda()
        bins = torch.empty(fixed.shape, dtype=torch.uint8, device="cuda")
        (ws, ws_ptr), (ws43, ws43_ptr) = _ws(need.value), _ws(need43.value)
        binned = torch.full((2 * n_bins,), np.nan, dtype=torch.float64, device="cuda")
        lut = torch.full((n_bins,), np.nan, dtype=torch.float64, device="cuda")
        sums = torch.full((43,), np.nan, dtype=torch.float64, device="cuda")
        geo = (fm.data_ptr(), *fixed.shape, m.data_ptr(), mm.data_ptr(), *moving.shape)
        assert lib.t2fit_register_bin_dev(f.data_ptr(), f.numel(), 220.0, n_bins / 360.0, n_bins, bins.data_ptr(), st) == 0
        assert lib.t2fit_register_binned_sums_dev(bins.data_ptr(), *geo, A, n_bins, binned.data_ptr(), lut.data_ptr(), ws_ptr, need.value, st) == 0
        assert lib.t2fit_register_sums_lut_dev(bins.data_ptr(), lut.data_ptr(), n_bins, *geo, A, sums.data_ptr(), ws43_ptr, need43.value, st) == 0
        # without a table: binned alone
        alone = torch.full((2 * n_bins,), np.nan, dtype=torch.float64, device="cuda")
        assert lib.t2fit_register_binned_sums_dev(bins.data_ptr(), *geo, A, n_bins, alone.data_ptr(), None, ws_ptr, need.value, st) == 0
    stream.synchronize()
    assert np.array_equal(bins.cpu().numpy(), AC.bins_of(name, n_bins))
    _assert_bits(binned.cpu().numpy(), w_binned, "binned")
    _assert_bits(alone.cpu().numpy(), w_binned, "binned, no table")
    _assert_bits(lut.cpu().numpy(), w_lut, "lut")
    _assert_bits(sums.cpu().numpy(), w_sums, "sums")

    # every refusal comes before a launch: the outputs keep their bytes
    before = (binned.clone(), lut.clone(), sums.clone(), bins.clone())
    AC.check_refusals(lib, f.data_ptr(), bins.data_ptr(), lut.data_ptr(), fm.data_ptr(), m.data_ptr(), mm.data_ptr(), binned.data_ptr(),
                      sums.data_ptr(), ws_ptr, ws43_ptr, fixed.shape, moving.shape, a, n_bins, st)
    torch.cuda.synchronize()
    for t, was in zip((binned, lut, sums, bins), before):
        assert t.cpu().numpy().tobytes() == was.cpu().numpy().tobytes()


def test_atlas_labels_equal_the_statement(t2):
    import torch

    subject, template, g, mask, atlases, truth = AC.atlas_case()
    w_warped, w_labels, w_found = AC.atlas_statement()
    warped, labels, found = t2.atlas.atlas_labels(subject, g, template, g, atlases, mask=mask)
    assert found.parameters.tobytes() == w_found.parameters.tobytes() and found.iterations == w_found.iterations
    assert warped.dtype == np.float32 and np.array_equal(warped.view(np.uint32), w_warped.view(np.uint32))
    for name in ("ho", "jhu"):
        assert labels[name].dtype == np.int32 and np.array_equal(labels[name], w_labels[name])
        for value in np.unique(truth[name])[1:]:
            assert AC.dice(labels[name], truth[name], value) >= 0.9
    brain = t2.atlas.extract_brain(torch.from_numpy(subject).cuda(), torch.from_numpy(mask).cuda())
    assert brain.is_cuda and np.array_equal(brain.cpu().numpy(), t2.atlas.extract_brain(subject, mask))
    assert np.array_equal(t2.atlas.extract_brain(subject, mask), np.where(mask != 0, subject, 0))


def test_recon_atlas_labels_on_the_device(t2, tmp_path, monkeypatch):
    import sys

    import fake_sitk

    fake = fake_sitk.install()
    monkeypatch.setitem(sys.modules, "SimpleITK", fake)
    from fetal_t2mapping_amd import cli, recon

    bids, md, template_path, specs = AC.write_atlas_subject(tmp_path)
    written = recon.process_atlas_labels(md, bids, template_path, specs)
    assert len(written) == 5
    AC.check_atlas_files(fake, bids, md, cli)
