"""The N4 bias-field correction's device half (csrc/t2fit_n4.hip) against its numpy statement
(fetal_t2mapping_amd/_bias.py): every step bit for bit where no transcendental is involved (mask, min/max, histogram,
omega, delta, lattice, field, the new u), within 1 float32 ulp through log and exp, the convergence sums within the
documented error of expm1; every step against a second call; min/max and histogram of more voxels than their grid grows
for; raw calls on a caller's stream with a NaN workspace and buffers 4 bytes past a 256-byte boundary; whole calls; the
recovery of a known field; recon.py --n4.  tests/test_bias_host.py covers what needs no device."""
import ctypes as C
import functools
import sys

import numpy as np
import pytest

import bias_cases as K
from fetal_t2mapping_amd import _abi, _bias

pytestmark = pytest.mark.gpu

SUMS_BOUND = 8 * 2.2e-16  # times sum |terms|: the error the two libraries document for expm1 (a few ulp each)


@pytest.fixture(scope="module")
def t2():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X")
    import fetal_t2mapping_amd as t2

    return t2


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    diff = np.flatnonzero(_bits(got).ravel() != _bits(want).ravel())
    assert diff.size == 0, (what, diff[:8], got.ravel()[diff[:8]], want.ravel()[diff[:8]])


def _ulps32(got, want):
    """The largest distance in float32 steps (both finite, same sign or zero)."""
    g, w = (np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64) for a in (got, want))
    return int(np.max(np.abs(g - w))) if g.size else 0


def _host(t):
    return t.cpu().numpy()


def _steps(t2, shape, side, kind):
    """One pass through every step on the device, each compared with the statement and with a second call."""
    B = t2.bias
    vol, mask = (np.array(a) for a in K.case(shape, kind))  # (the shared case is read-only)
    # 1. log image: the mask is exact, the log within 1 ulp; everything after runs on the device's own log image
    u0_t, m_t = B.log_image(vol, mask)
    u0, m = _host(u0_t), _host(m_t)
    w_u0, w_m = _bias.log_image(vol, mask)
    _same(m, w_m, "mask")
    assert _ulps32(u0, w_u0) <= 1 and np.all(u0[m == 0] == 0)
    _same(_host(B.log_image(vol, mask)[0]), u0, "log, second call")
    _same(_host(B.log_image(vol)[1]), (vol > 0).astype(np.uint8), "mask of None")
    # min / max
    lo, hi = B.minmax(u0_t, m_t)
    _same(np.array([lo, hi]), np.array(_bias.minmax(u0, m)), "min / max")
    # 2. histogram and table (one voxel: no range, the fit takes u itself)
    table, slope = None, 1.0
    if hi > lo:
        slope = _bias.slope_of(lo, hi)
        hist = B.histogram(u0_t, m_t, float(lo), slope)
        _same(hist, _bias.histogram(u0, m, float(lo), slope), "histogram")
        _same(B.histogram(u0_t, m_t, float(lo), slope), hist, "histogram, second call")
        assert int(hist.sum()) == int(m.sum()) << 24
        table = _bias.sharpen_table(hist, lo, slope, 0.15)
    # 3. omega, delta, lattice
    omega = B.fit_weights(m_t, side)
    _same(omega, _bias.fit_weights(m, side), "omega")
    _same(B.fit_weights(m_t, side), omega, "omega, second call")
    lat0 = K.lattice_of(side)
    for tab in ((table, None) if table is not None else (None,)):
        delta, lat = B.fit(u0_t, m_t, lat0, omega, tab, float(lo) if tab is not None else 0.0, slope)
        w_delta = _bias.fit_delta(u0, m, side, tab, float(lo), slope)
        _same(delta, w_delta, "delta")
        _same(lat, _bias.lattice_update(lat0, w_delta, omega), "lattice")
        again = B.fit(u0_t, m_t, lat0, omega, tab, float(lo) if tab is not None else 0.0, slope)
        _same(again[0], delta, "delta, second call"), _same(again[1], lat, "lattice, second call")
    # 4, 5. field, the new u, its range, the sums
    old = K.old_field(shape)
    field_t, u_t, sums, rng = B.field_step(lat, u0_t, m_t, old)
    w_field = _bias.field_eval(lat, shape)
    _same(_host(field_t), w_field, "field")
    w_u = _bias.next_u(u0, w_field, m)
    _same(_host(u_t), w_u, "new u")
    _same(np.array(rng, np.float32), np.array(_bias.minmax(w_u, m), np.float32), "range of the new u")
    d = _bias.convergence_terms(w_field, old, m)
    w_sums = _bias.convergence_sums(w_field, old, m)
    mags = (float(np.abs(d).sum()), float((d * d).sum()))
    ratios = [abs(g - w) / mag if mag else abs(g - w) for g, w, mag in zip(sums, w_sums, mags)]
    assert max(ratios) <= SUMS_BOUND, (ratios, sums, w_sums)
    second = B.field_step(lat, u0_t, m_t, old)
    _same(_host(second[0]), w_field, "field, second call"), _same(_host(second[1]), w_u, "new u, second call")
    assert second[2] == sums and second[3] == rng
    # 7. output
    out = B.apply_field(vol, w_field, 0.25)
    assert _ulps32(out, _bias.apply_field(vol, w_field, 0.25)) <= 1 and out.dtype == np.float32
    _same(B.apply_field(vol, w_field, 0.25), out, "output, second call")
    return max(ratios)


@pytest.mark.parametrize("side", K.SIDES)
@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_step_equals_the_statement_and_repeats(t2, shape, side):
    """Measured on the MI355X: the convergence sums' largest ratio over these cases is printed (pytest -s); the bound is
    8 x 2.2e-16.  The largest seen on the MI355X: 4.16e-16."""
    worst = max(_steps(t2, shape, side, kind) for kind in ("rows", "one"))
    print(f"{shape} side {side}: convergence sums, |device - statement| / sum |terms| = {worst:.3e}")


def test_minmax_and_histogram_past_the_grid_cap(t2):
    """1024 x 2048 + 2049 voxels: the grid stays at its 1024 workgroups, every thread makes more than eight trips, and the
    extremes (and the last voxel) are read on the ninth alone; the final kernel reads all 1024 partials."""
    B = t2.bias
    u, m = (np.array(a) for a in K.capped_case())  # (the shared case is read-only)
    w_lo, w_hi, slope = K.check_capped()           # (numpy alone: the extremes are unique and lie in the tail)
    want = _bias.histogram(u, m, float(w_lo), slope)
    for call in ("first", "second"):
        lo, hi = B.minmax(u, m)
        _same(np.array([lo, hi]), np.array([w_lo, w_hi]), f"min / max, {call} call")
        hist = B.histogram(u, m, float(lo), slope)
        _same(hist, want, f"histogram, {call} call")
        assert int(hist.sum()) == int(m.sum()) << 24


def _offset(t, elements):
    """A copy of tensor `t` that starts `elements` elements into a fresh buffer."""
    import torch

    buf = torch.empty(t.numel() + elements + 64, dtype=t.dtype, device="cuda")
    view = buf[elements:elements + t.numel()]
    view.copy_(t.reshape(-1))
    return buf, view


def test_raw_calls_on_another_stream_nan_workspace_and_offset_buffers(t2):
    """ctypes calls on a caller's stream: the workspace is all NaN before every call, and every float32 / uint8 buffer
    starts 4 bytes past a 256-byte boundary (float64 ones 8 bytes past one)."""
    import torch

    from fetal_t2mapping_amd._lib import load

    lib = load()
    shape, side = (19, 23, 37), 7
    vol, mask = (np.array(a) for a in K.case(shape))
    n = int(np.prod(shape))
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)
    need = C.c_size_t(0)
    assert lib.t2fit_n4_workspace_bytes(*shape, side, C.byref(need)) == _abi.OK
    ws = torch.empty(need.value + 256, dtype=torch.uint8, device="cuda")
    ptr = (ws.data_ptr() + 255) // 256 * 256

    def poison():
        ws.fill_(0xFF)  # every float and double of it is a NaN

    def at4(t):  # 65 floats = 260 bytes; 260 bytes of a uint8 buffer
        buf, view = _offset(t, 65 if t.dtype == torch.float32 else 260)
        assert view.data_ptr() % 256 == 4
        return buf, view

    def at8(t):
        buf, view = _offset(t, 33)
        assert view.data_ptr() % 256 == 8
        return buf, view

    keep = []

    def dev(a, where):
        buf, view = where(torch.from_numpy(np.ascontiguousarray(a)).cuda())
        keep.append(buf)
        return view

    vol_d, mask_d = dev(vol, at4), dev(mask, at4)
    u0_d, m_d = dev(np.zeros(n, np.float32), at4), dev(np.zeros(n, np.uint8), at4)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        poison()
        assert lib.t2fit_n4_log_dev(vol_d.data_ptr(), mask_d.data_ptr(), n, u0_d.data_ptr(), m_d.data_ptr(), st) == _abi.OK
        rng_d = dev(np.zeros(2, np.float32), at4)
        assert lib.t2fit_n4_minmax_dev(u0_d.data_ptr(), m_d.data_ptr(), n, rng_d.data_ptr(), ptr, need.value, st) == _abi.OK
        stream.synchronize()
        u0, m = _host(u0_d).reshape(shape), _host(m_d).reshape(shape)
        lo, hi = _host(rng_d)
        _same(np.array([lo, hi]), np.array(_bias.minmax(u0, m)), "min / max")
        slope = _bias.slope_of(lo, hi)
        hist_d = dev(np.zeros(200, np.int64), at8)
        poison()
        assert lib.t2fit_n4_histogram_dev(u0_d.data_ptr(), m_d.data_ptr(), n, float(lo), slope, 200, hist_d.data_ptr(), st) == _abi.OK
        stream.synchronize()
        hist = _host(hist_d).view(np.uint64)
        _same(hist, _bias.histogram(u0, m, float(lo), slope), "histogram")
        table = _bias.sharpen_table(hist, lo, slope, 0.15)
        omega_d, delta_d = dev(np.zeros(side ** 3), at8), dev(np.zeros(side ** 3), at8)
        lat0 = K.lattice_of(side)
        lat_d, table_d = dev(lat0.ravel(), at8), dev(table, at8)
        poison()
        assert lib.t2fit_n4_weights_dev(m_d.data_ptr(), *shape, side, omega_d.data_ptr(), ptr, need.value, st) == _abi.OK
        poison()
        assert lib.t2fit_n4_fit_dev(u0_d.data_ptr(), m_d.data_ptr(), *shape, table_d.data_ptr(), float(lo), slope, 200, side,
                                    omega_d.data_ptr(), lat_d.data_ptr(), delta_d.data_ptr(), ptr, need.value, st) == _abi.OK
        stream.synchronize()
        omega = _host(omega_d).reshape((side,) * 3)
        _same(omega, _bias.fit_weights(m, side), "omega")
        w_delta = _bias.fit_delta(u0, m, side, table, float(lo), slope)
        _same(_host(delta_d).reshape((side,) * 3), w_delta, "delta")
        lat = _bias.lattice_update(lat0, w_delta, omega)
        _same(_host(lat_d).reshape((side,) * 3), lat, "lattice")
        old = K.old_field(shape)
        field_d, u_d = dev(old.ravel(), at4), dev(np.zeros(n, np.float32), at4)
        sums_d, rng2_d = dev(np.zeros(2), at8), dev(np.zeros(2, np.float32), at4)
        poison()
        assert lib.t2fit_n4_field_dev(lat_d.data_ptr(), side, u0_d.data_ptr(), m_d.data_ptr(), *shape, field_d.data_ptr(),
                                      u_d.data_ptr(), sums_d.data_ptr(), rng2_d.data_ptr(), ptr, need.value, st) == _abi.OK
        out_d = dev(np.zeros(n, np.float32), at4)
        assert lib.t2fit_n4_apply_dev(vol_d.data_ptr(), field_d.data_ptr(), n, 1.0, out_d.data_ptr(), st) == _abi.OK
        stream.synchronize()
    w_field = _bias.field_eval(lat, shape)
    _same(_host(field_d).reshape(shape), w_field, "field")
    w_u = _bias.next_u(u0, w_field, m)
    _same(_host(u_d).reshape(shape), w_u, "new u")
    _same(_host(rng2_d), np.array(_bias.minmax(w_u, m), np.float32), "range")
    d = _bias.convergence_terms(w_field, old, m)
    for got, want, mag in zip(_host(sums_d), _bias.convergence_sums(w_field, old, m), (np.abs(d).sum(), (d * d).sum())):
        assert abs(got - want) <= SUMS_BOUND * mag
    assert _ulps32(_host(out_d).reshape(shape), _bias.apply_field(vol, w_field)) <= 1
    # every refusal comes back before any launch, on this stream as on none
    for name, args, word in K.refusals():
        assert getattr(lib, name)(*args[:-1], st) == _abi.E_INVALID, (name, args)
        assert word in lib.t2fit_last_error().decode()
    torch.cuda.synchronize()  # nothing was launched with the made-up addresses: the device is still well


@functools.lru_cache(maxsize=None)
def _recovery(device_log=True):
    """The recovery phantom through the device at full defaults, and the statement on the device's own log image."""
    import fetal_t2mapping_amd as t2

    vol, mask, _, _ = K.recovery_phantom()
    found = t2.bias.n4_correct(vol, mask)
    u0, m = t2.bias.log_image(vol, mask)
    want = _bias.n4_correct(vol, mask, log=(_host(u0), _host(m)))
    return found, want


def test_whole_call_equals_the_statement_on_the_devices_log_image(t2):
    found, want = _recovery()
    # the case keeps every convergence figure at least 1e-6 away from the threshold (checked with the statement)
    assert min(abs(c - 1e-3) for level in want.convergence for c in level) >= 1e-6
    assert found.iterations == want.iterations
    _same(found.lattice, want.lattice, "lattice")
    _same(found.log_field, want.log_field, "field")
    assert _ulps32(found.corrected, want.corrected) <= 1
    for a, b in zip(found.convergence, want.convergence):
        assert np.allclose(a, b, rtol=1e-9, atol=0)
    # tensors in, tensors out; a scale; a short budget
    import torch

    vol, mask, _, _ = K.recovery_phantom()
    short = t2.bias.n4_correct(torch.from_numpy(vol).cuda(), torch.from_numpy(mask).cuda(), max_iter=(3, 2), scale=0.25)
    assert torch.is_tensor(short.corrected) and short.corrected.is_cuda and short.iterations == (3, 2)
    assert _ulps32(_host(short.corrected), _bias.apply_field(vol, _host(short.log_field), 0.25)) <= 1
    assert _ulps32(_host(t2.bias.apply_field(torch.from_numpy(vol).cuda(), short.log_field, 0.25)), _host(short.corrected)) == 0
    with pytest.raises(ValueError, match="flat"):
        t2.bias.n4_correct(np.full((4, 5, 6), 7.0, np.float32), np.ones((4, 5, 6), np.uint8))
    with pytest.raises(ValueError, match="finite"):
        t2.bias.n4_correct(np.full((4, 5, 6), np.nan, np.float32), np.ones((4, 5, 6), np.uint8))
    with pytest.raises(ValueError, match="max_iter"):
        t2.bias.n4_correct(vol, mask, max_iter=(1,) * 6)


def test_recovery_of_a_known_field_on_the_device(t2):
    """The host test's bars (bias_cases.check_recovery), on the device's result."""
    found, _ = _recovery()
    K.check_recovery(found.corrected, found.log_field)
    # mask None: build_mask on the device; the ball is found and the field recovered as well
    vol, mask, _, logf = K.recovery_phantom()
    auto = t2.bias.n4_correct(vol)
    assert 1.0 - K.field_correlation(auto.log_field, logf, mask) <= 10 * K.RECOVERY_ONE_MINUS_CORR


def test_recon_n4_lowers_the_class_cv_of_the_merged_volume(t2, tmp_path, monkeypatch):
    """recon.py --n4 on stacks that each carry a field of their own: the brightest class of the merged volume varies less
    than without the flag, at every echo; --write_n4 leaves the corrected stacks, whose echo ratios are the raw ones."""
    import glob
    import os

    monkeypatch.setitem(sys.modules, "SimpleITK", None)  # the package's NIfTI reader
    from fetal_t2mapping_amd import nifti, recon

    stacks, geoms, cls = K.recon_phantom()
    bids, md = K.write_recon_subject(tmp_path, stacks, geoms)
    plain = [K.recon_cv(nifti.ReadImage(p).arr, cls) for p in recon.process_recon(md, bids, denoise=False)]
    args = recon.parse_arguments(["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo", "--lf", "--n4", "--write_n4"])
    fixed = [K.recon_cv(nifti.ReadImage(p).arr, cls) for p in recon.process_recon(md, bids, denoise=False, n4=args.n4_args,
                                                                                   write_n4=args.write_n4)]
    print("class CV of the merged volume per echo: without --n4", plain, "with", fixed)
    assert len(plain) == len(fixed) == 3 and all(f < p for f, p in zip(fixed, plain))
    files = sorted(glob.glob(os.path.join(bids, "prj-900", "derivatives", recon.n4_dirname, "sub-001", "ses-01", "anat", "*_T2w_n4.nii.gz")))
    assert len(files) == 9
    first, second = (np.asarray(nifti.ReadImage(files[i]).arr, np.float64) for i in (0, 3))  # the ax stacks of two echoes
    inside = (stacks["ax"][0] > 0) & (stacks["ax"][1] > 0)
    want = stacks["ax"][0][inside].astype(np.float64) / stacks["ax"][1][inside]
    assert np.max(np.abs(first[inside] / second[inside] / want - 1.0)) <= 2.0 ** -23
