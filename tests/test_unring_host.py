"""The unringing without a GPU: the numpy statement (fetal_t2mapping_amd/_unring.py) against the independent float64
reference of tests/unring_cases.py within derived bounds, the taps and tables, the exact cases, the benefit on the
band-limited phantom, and the refusals through Python and through the C entry points that need no kernel.  The drivers
(recon.py, cli.py) are in test_unring_drivers_host.py; the device is held to the statement in test_unring_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

import unring_cases as K
from fetal_t2mapping_amd import _abi, _unring

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from fetal_t2mapping_amd import build
    from fetal_t2mapping_amd._lib import load

    build.build()
    return load()


# ---- against the reference ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ny,nx", K.NOISY_SIZES)
def test_split_against_the_reference(ny, nx):
    """Bound: unring_cases.split_bound, the first-order bound of the four float32 chains (lengths nx, 2ny, 2ny, 2nx) in the
    Frobenius norm of one slice; it bounds every element too.  I1 + I2 = X holds to one rounding."""
    x = np.stack([K.noisy_phantom(ny, nx), K.random_slices(1, ny, nx, 3)[0]])
    t = _unring.Tables(ny, nx, 20)
    i1, i2 = _unring.split(x, t)
    r1, r2 = K.ref_split(x)
    assert i1.dtype == np.float32 and i1.shape == x.shape and i2.shape == x.shape
    for s in range(2):
        bound = K.split_bound(x[s])
        err = float(np.linalg.norm(i1[s].astype(np.float64) - r1[s]))
        print(f"split {ny} x {nx} slice {s}: |I1 - ref|_F {err:.3g}, max {np.abs(i1[s] - r1[s]).max():.3g}, bound {bound:.3g}")
        assert err <= bound
        assert np.abs(i2[s] - r2[s]).max() <= bound + K.U32 * np.abs(x[s]).max()
    assert np.array_equal(i2, x - i1)
    assert np.abs(r1).max() > 10 and np.abs(r2).max() > 10  # both parts carry signal


@pytest.mark.parametrize("ny,nx", K.NOISY_SIZES)
@pytest.mark.parametrize("window", [(1, 3), (2, 5)])
def test_rows_against_the_reference(ny, nx, window):
    """The winning tv within unring_cases.tv_bound on every sample; the winning shift equal on at least 90 % of the samples; the
    value within unring_cases.value_bound where the shift agrees."""
    x = K.noisy_phantom(ny, nx)[None]
    t = _unring.Tables(ny, nx, 20)
    r1, r2 = K.ref_split(x)
    for rows, h in ((r1[0].astype(np.float32), t.hx), (r2[0].T.astype(np.float32), t.hy)):
        out, shift, tv = _unring.unring_rows(rows, h, t.ab, *window)
        ro, rs, rtv = K.ref_rows(rows, 20, *window)
        assert out.dtype == np.float32 and shift.dtype == np.int8 and tv.dtype == np.float32
        share = float(np.mean(shift == rs))
        print(f"rows {rows.shape} window {window}: shift agrees on {share:.4f}, tv err {np.abs(tv - rtv).max():.3g}, "
              f"value err {np.abs(out - ro)[shift == rs].max():.3g}")
        assert np.all(np.abs(tv - rtv) <= K.tv_bound(rows, *window, rtv))
        assert share >= 0.9
        same = shift == rs
        assert np.all((np.abs(out - ro) <= K.value_bound(rows, ro))[same])
        assert len(np.unique(shift)) > 10  # the shifts are in use


def test_shifted_rows_against_the_phase_ramp():
    rows = K.random_slices(1, 9, 33, 5)[0]
    for n, K_ in ((33, 3), (32, 20)):
        r = rows[:, :n].copy()
        y = _unring.shifted(r, _unring.taps(n, K_))
        ref = K.ref_shifted(r, K_)
        assert np.all(np.abs(y[1:] - ref[1:]) <= K.shifted_bound(r)[None, :, None])


# ---- taps and tables ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [8, 9, 32, 33, 65, 130])
def test_taps_sum_to_one_and_mirror(n):
    K_ = 7
    h = _unring.taps(n, K_).astype(np.float64)
    assert np.all(np.abs(h.sum(axis=1) - 1.0) <= (n + 1) * K.U32)
    # h_{K+j}[d] = h_j[-d]: shifting a mirrored row by -s mirrors the row shifted by s
    mirror = h[:, (-np.arange(n)) % n]
    assert np.all(np.abs(h[K_ + 1:] - mirror[1:K_ + 1]) <= 2 * K.U32)
    row = K.random_slices(1, 8, n, n)[0, :1]
    y = _unring.shifted(row, _unring.taps(n, K_))
    ym = _unring.shifted(row[:, ::-1].copy(), _unring.taps(n, K_))
    bound = 2 * K.shifted_bound(row)[0]
    for j in range(1, K_ + 1):
        assert np.all(np.abs(y[j, 0] - ym[K_ + j, 0][::-1]) <= bound)
    s = _unring.shifts(K_)
    assert s[0] == 0 and np.all(s[1:K_ + 1] > 0) and np.all(s[K_ + 1:] == -s[1:K_ + 1]) and abs(s[K_]) < 0.5
    ab = _unring.weights(K_)
    assert ab.dtype == np.float32 and ab[0, 0] == 1 and ab[1, 0] == 0 and np.all(np.abs(ab.sum(axis=0) - 1) <= 2 * K.U32)


@pytest.mark.parametrize("ny,nx,shifts", [(8, 8, 1), (33, 40, 20), (24, 65, 3), (32, 130, 32)])
def test_tables_of_the_library_against_python(lib, ny, nx, shifts):
    """t2fit_unring_tables_host (no GPU) against _unring.Tables: the same header and layout, every value within one float32
    step, and exactly equal where the value is 0, +-1 or +-0.5."""
    from fetal_t2mapping_amd import _gpu_unring

    blob = _gpu_unring.tables_host(ny, nx, shifts)
    t = _unring.Tables(ny, nx, shifts)
    mine = t.pack()
    assert blob.size == mine.size and np.array_equal(blob[:128], mine[:128])
    got = _unring.Tables.unpack(blob)
    for (name, a) in t.parts():
        b = getattr(got, name)
        assert a.shape == b.shape and a.dtype == b.dtype == np.float32, name
        step = np.spacing(np.maximum(np.abs(a), np.abs(b)))
        assert np.all(np.abs(a.astype(np.float64) - b) <= step), name
        exact = np.isin(a, np.array([0, 1, -1, 0.5, -0.5], np.float32))
        assert np.array_equal(a[exact], b[exact]), name
    assert np.any(t.cx == 1) and np.any(t.cx == -1) == (nx % 2 == 0) and t.hx[0, 0] == 1 and np.all(t.hx[0, 1:] == 0)
    # the filter: Gx + Gy = 1 (before the normalisation), 0.5 at the double Nyquist corner
    g = t.g.astype(np.float64) * nx * ny
    if nx == ny:
        assert np.all(np.abs(g + g.T - 1.0) <= 4 * K.U32)
    if nx % 2 == 0 and ny % 2 == 0:
        assert t.g[ny // 2, nx // 2] == np.float32(0.5 / (nx * ny))


# ---- exact cases --------------------------------------------------------------------------------------------------------

def test_constant_zero_and_nan_slices():
    t = _unring.Tables(33, 40, 20)
    x = K.random_slices(4, 33, 40, 9)
    x[0] = np.float32(7.3)
    x[1] = 0.0
    x[2, 5, 7] = np.nan
    out, skipped = _unring.unring(x, t)
    assert skipped == 1
    assert out[0].tobytes() == x[0].tobytes() and out[1].tobytes() == x[1].tobytes() and out[2].tobytes() == x[2].tobytes()
    alone, none = _unring.unring(x[3:], t)
    assert none == 0 and out[3].tobytes() == alone[0].tobytes() and not np.array_equal(out[3], x[3])
    # rows: a constant row keeps shift 0 with tv 0
    o, s, tv = _unring.unring_rows(np.full((2, 40), 5.5, np.float32), t.hx, t.ab)
    assert np.all(o == np.float32(5.5)) and np.all(s == 0) and np.all(tv == 0)


def test_circular_wrap():
    """A step at column 0 is treated like one in the middle: rolling the rows rolls the result, up to the chain's rounding
    (the summation starts at another sample), and exactly in the chosen shifts away from near ties."""
    n = 40
    t = _unring.Tables(33, n, 20)
    rows = np.zeros((1, n), np.float32)
    rows[0, : n // 2] = 100.0
    rows = K.band_limit(np.repeat(rows, 8, axis=1).astype(np.float64).repeat(8, axis=0), 1, n).astype(np.float32)  # a ringing step pair
    o, s, tv = _unring.unring_rows(rows, t.hx, t.ab)
    for roll in (1, 7, n // 2):
        o2, s2, tv2 = _unring.unring_rows(np.roll(rows, roll, axis=1), t.hx, t.ab)
        assert np.all(np.abs(np.roll(tv2, -roll, axis=1) - tv) <= K.tv_bound(rows, 1, 3, tv) * 2)
        agree = np.roll(s2, -roll, axis=1) == s
        assert agree.mean() >= 0.9
        assert np.all((np.abs(np.roll(o2, -roll, axis=1) - o) <= 2 * K.value_bound(rows, o))[agree])
    assert np.abs(o - rows).max() > 1.0  # the ringing is there and is changed


# ---- benefit ------------------------------------------------------------------------------------------------------------

def test_benefit_on_the_band_limited_phantom():
    img, truth, flat = K.phantom()
    assert img.shape == (48, 48) and flat.sum() > 500
    t = _unring.Tables(48, 48, 20)
    out, _ = _unring.unring(img[None].copy(), t)

    def figures(a):
        e = (a.astype(np.float64) - truth)[flat]
        return float(np.sqrt(np.mean(e * e))), float(np.abs(e).max())

    before, after = figures(img), figures(out[0])
    print(f"flat-region RMSE {before[0]:.3f} -> {after[0]:.3f} ({after[0] / before[0]:.3f} x), overshoot {before[1]:.2f} -> {after[1]:.2f}")
    assert after[0] <= 0.5 * before[0]
    assert after[1] < before[1]
    ref = K.ref_unring(img[None])[0]
    rb = figures(ref)
    assert rb[0] <= 0.5 * before[0]
    blob = K.blob()
    ob, _ = _unring.unring(blob[None].copy(), t)
    print(f"smooth blob changes by at most {np.abs(ob[0] - blob).max():.3f}")
    assert blob.max() > 99 and np.abs(ob[0] - blob).max() < 0.5


def test_the_near_tie_rows_bite():
    rows, t, shift32, differ = K.near_tie_case()
    assert differ >= 10 and rows.shape[1] == 40 and shift32.shape == rows.shape


# ---- refusals -------------------------------------------------------------------------------------------------------------

BAD = [dict(ny=7, nx=40), dict(ny=33, nx=7), dict(ny=513, nx=40), dict(ny=33, nx=513), dict(K=0), dict(K=33), dict(min_w=0),
       dict(max_w=9), dict(min_w=3, max_w=2), dict(ny=8, nx=40, max_w=4)]


@pytest.mark.parametrize("bad", BAD)
def test_refusals_in_python(bad):
    args = dict(ny=33, nx=40, K=20, min_w=1, max_w=3)
    args.update(bad)
    with pytest.raises(ValueError, match="unring"):
        _unring.check_params(**args)
    assert _unring.check_params(33, 40) == (33, 40, 20, 1, 3)
    assert _unring.check_params(9, 9, 1, 1, 3) == (9, 9, 1, 1, 3)


@pytest.mark.parametrize("bad", BAD)
def test_refusals_of_the_library_before_hip(lib, bad):
    args = dict(ny=33, nx=40, K=20, min_w=1, max_w=3)
    args.update(bad)
    p = _abi.T2FitUnringParams()
    assert lib.t2fit_unring_params_default(C.byref(p)) == _abi.OK and (p.K, p.min_w, p.max_w, p.flags) == (20, 1, 3, 0)
    p.K, p.min_w, p.max_w = args["K"], args["min_w"], args["max_w"]
    need = C.c_size_t(0)
    ptr = C.c_void_p(4096)  # never dereferenced: the refusal comes first
    assert lib.t2fit_unring_workspace_bytes(C.byref(p), 3, args["ny"], args["nx"], C.byref(need)) == _abi.E_INVALID
    assert b"t2fit_unring_workspace_bytes" in lib.t2fit_last_error()
    axis = 1 if args["ny"] != 33 else 0  # the rows are held to the limits along their own axis only
    assert lib.t2fit_unring_rows_dev(C.byref(p), ptr, ptr, 3, args["ny"], args["nx"], axis, C.c_void_p(8192), None, None, None) == _abi.E_INVALID
    assert b"t2fit_unring_rows_dev" in lib.t2fit_last_error()
    assert lib.t2fit_unring_dev(C.byref(p), ptr, ptr, 3, args["ny"], args["nx"], C.c_void_p(8192), None, None, None, ptr, 1 << 30,
                                None) == _abi.E_INVALID
    if "K" in bad or "ny" in bad and "max_w" not in bad:
        assert lib.t2fit_unring_tables_bytes(args["ny"], args["nx"], args["K"], C.byref(need)) == _abi.E_INVALID
        assert lib.t2fit_unring_tables_host(args["ny"], args["nx"], args["K"], ptr, 1 << 30) == _abi.E_INVALID


def test_null_pointers_and_small_buffers_are_refused_before_hip(lib):
    p = _abi.T2FitUnringParams()
    lib.t2fit_unring_params_default(C.byref(p))
    need = C.c_size_t(0)
    ptr, other, third = C.c_void_p(4096), C.c_void_p(8192), C.c_void_p(12288)
    ws = C.c_void_p(1 << 20)
    assert lib.t2fit_unring_params_default(None) == _abi.E_INVALID
    assert lib.t2fit_unring_tables_bytes(33, 40, 20, None) == _abi.E_INVALID
    assert lib.t2fit_unring_tables_bytes(33, 40, 20, C.byref(need)) == _abi.OK and need.value == _unring.Tables(33, 40, 20).pack().size
    buf = np.zeros(need.value, np.uint8)
    assert lib.t2fit_unring_tables_host(33, 40, 20, None, need.value) == _abi.E_INVALID
    assert lib.t2fit_unring_tables_host(33, 40, 20, buf.ctypes.data, need.value - 1) == _abi.E_INVALID
    assert b"bytes" in lib.t2fit_last_error()
    assert lib.t2fit_unring_workspace_bytes(None, 3, 33, 40, C.byref(need)) == _abi.E_INVALID
    assert lib.t2fit_unring_workspace_bytes(C.byref(p), 3, 33, 40, None) == _abi.E_INVALID
    assert lib.t2fit_unring_workspace_bytes(C.byref(p), -1, 33, 40, C.byref(need)) == _abi.E_INVALID
    assert lib.t2fit_unring_workspace_bytes(C.byref(p), 3, 33, 40, C.byref(need)) == _abi.OK and need.value >= 6 * 3 * 33 * 40 * 4
    big = need.value
    # the workspace does not depend on K or on the window
    for k, lo, hi in ((1, 1, 1), (32, 1, 3), (20, 2, 8)):
        p.K, p.min_w, p.max_w = k, lo, hi
        assert lib.t2fit_unring_workspace_bytes(C.byref(p), 3, 33, 40, C.byref(need)) == _abi.OK and need.value == big
    lib.t2fit_unring_params_default(C.byref(p))
    # split
    for args in ((None, ptr, other, third), (ptr, None, other, third), (ptr, ptr, None, third), (ptr, ptr, other, None)):
        assert lib.t2fit_unring_split_dev(args[0], args[1], 3, 33, 40, args[2], args[3], ws, big, None) == _abi.E_INVALID
    assert lib.t2fit_unring_split_dev(ptr, other, 3, 33, 40, other, third, ws, big, None) == _abi.E_INVALID      # I1 is the input
    assert lib.t2fit_unring_split_dev(ptr, other, 3, 33, 40, third, third, ws, big, None) == _abi.E_INVALID      # I1 is I2
    assert lib.t2fit_unring_split_dev(ptr, other, 3, 33, 40, third, ws, None, big, None) == _abi.E_INVALID       # no workspace
    assert lib.t2fit_unring_split_dev(ptr, other, 3, 33, 40, third, ws, C.c_void_p(4100), big, None) == _abi.E_INVALID
    assert lib.t2fit_unring_split_dev(ptr, other, 3, 33, 40, third, ws, C.c_void_p(1 << 21), big - 1, None) == _abi.E_INVALID
    assert b"workspace" in lib.t2fit_last_error()
    assert lib.t2fit_unring_split_dev(ptr, C.c_void_p(8194), 3, 33, 40, third, ws, C.c_void_p(1 << 21), big, None) == _abi.E_INVALID
    assert b"aligned" in lib.t2fit_last_error()
    assert lib.t2fit_unring_split_dev(C.c_void_p(4100), other, 3, 33, 40, third, ws, C.c_void_p(1 << 21), big, None) == _abi.E_INVALID
    assert lib.t2fit_unring_split_dev(ptr, other, -1, 33, 40, third, ws, C.c_void_p(1 << 21), big, None) == _abi.E_INVALID
    # rows
    assert lib.t2fit_unring_rows_dev(None, ptr, other, 3, 33, 40, 0, third, None, None, None) == _abi.E_INVALID
    assert lib.t2fit_unring_rows_dev(C.byref(p), None, other, 3, 33, 40, 0, third, None, None, None) == _abi.E_INVALID
    assert lib.t2fit_unring_rows_dev(C.byref(p), ptr, None, 3, 33, 40, 0, third, None, None, None) == _abi.E_INVALID
    assert lib.t2fit_unring_rows_dev(C.byref(p), ptr, other, 3, 33, 40, 0, None, None, None, None) == _abi.E_INVALID
    assert lib.t2fit_unring_rows_dev(C.byref(p), ptr, other, 3, 33, 40, 2, third, None, None, None) == _abi.E_INVALID
    assert b"axis" in lib.t2fit_last_error()
    assert lib.t2fit_unring_rows_dev(C.byref(p), ptr, other, 3, 33, 40, 0, other, None, None, None) == _abi.E_INVALID
    assert lib.t2fit_unring_rows_dev(C.byref(p), ptr, other, 3, 0, 40, 0, third, None, None, None) == _abi.E_INVALID    # no rows
    assert lib.t2fit_unring_rows_dev(C.byref(p), ptr, other, 3, 513, 40, 0, third, None, None, None) == _abi.E_INVALID
    assert b"across" in lib.t2fit_last_error()
    # the whole stage
    assert lib.t2fit_unring_dev(None, ptr, other, 3, 33, 40, third, None, None, None, ws, big, None) == _abi.E_INVALID
    assert lib.t2fit_unring_dev(C.byref(p), None, other, 3, 33, 40, third, None, None, None, ws, big, None) == _abi.E_INVALID
    assert lib.t2fit_unring_dev(C.byref(p), ptr, None, 3, 33, 40, third, None, None, None, ws, big, None) == _abi.E_INVALID
    assert lib.t2fit_unring_dev(C.byref(p), ptr, other, 3, 33, 40, None, None, None, None, ws, big, None) == _abi.E_INVALID
    assert lib.t2fit_unring_dev(C.byref(p), ptr, other, 3, 33, 40, other, None, None, None, ws, big, None) == _abi.E_INVALID
    assert lib.t2fit_unring_dev(C.byref(p), ptr, other, 3, 33, 40, third, None, None, None, None, big, None) == _abi.E_INVALID
    assert lib.t2fit_unring_dev(C.byref(p), ptr, other, 3, 33, 40, third, None, None, None, ws, big - 1, None) == _abi.E_INVALID
    p.flags = 1
    assert lib.t2fit_unring_dev(C.byref(p), ptr, other, 3, 33, 40, third, None, None, None, ws, big, None) == _abi.E_INVALID


def test_wrong_dtype_and_shape_are_refused_by_the_binding():
    """The marshalling refuses before the library is asked (no GPU needed: the checks come before the device is picked up,
    or the call fails for want of a device, which is not what is matched here)."""
    from fetal_t2mapping_amd import _gpu_unring, t2map

    assert t2map.unring is _gpu_unring
    for name in ("unring_volume", "unring_split", "unring_rows", "unring_tables", "unring_slices"):
        assert callable(getattr(t2map.unring, name))
    with pytest.raises(ValueError, match="float32"):
        _gpu_unring.unring_volume(np.zeros((3, 33, 40), np.float64))
    with pytest.raises(ValueError, match="float32"):
        _gpu_unring.unring_volume(np.zeros((3, 33, 40), np.int16))
    with pytest.raises(ValueError, match="slice_axis"):
        _gpu_unring.unring_volume(np.zeros((3, 33, 40), np.float32), slice_axis=3)
    with pytest.raises(ValueError, match=r"\(\.\.\., Z, Y, X\)"):
        _gpu_unring.unring_volume(np.zeros((33, 40), np.float32))
    with pytest.raises(ValueError, match="axis must be"):
        _gpu_unring.unring_rows(np.zeros((3, 33, 40), np.float32), axis="z")
    t = _gpu_unring.unring_tables(33, 40, 20)
    assert t is _gpu_unring.unring_tables(33, 40, 20) and isinstance(t, _unring.Tables) and t.hx.shape == (41, 40)
    with pytest.raises(ValueError, match="unring"):
        _gpu_unring.unring_tables(7, 40, 20)


def test_abi_mirror_and_build_list():
    from fetal_t2mapping_amd import build

    header = open(os.path.join(REPO, "include", "t2fit.h")).read()
    names = [s[0] for s in _abi.SYMBOLS]
    assert len(_abi.UNRING_SYMBOLS) == 7
    for sym in _abi.UNRING_SYMBOLS:
        assert sym in names and sym + "(" in header and sym in _abi.LOOKED_UP
    assert (_abi.UNRING_MIN_N, _abi.UNRING_MAX_N, _abi.UNRING_MAX_SHIFTS, _abi.UNRING_MAX_WINDOW) == (8, 512, 32, 8)
    assert (_unring.MIN_N, _unring.MAX_N, _unring.MAX_K, _unring.MAX_W) == (8, 512, 32, 8)
    for macro, value in (("T2FIT_UNRING_MIN_N", 8), ("T2FIT_UNRING_MAX_N", 512), ("T2FIT_UNRING_MAX_SHIFTS", 32), ("T2FIT_UNRING_MAX_WINDOW", 8)):
        assert f"#define {macro} {value}" in header
    assert C.sizeof(_abi.T2FitUnringParams) == 16
    assert "t2fit_unring.hip" in [os.path.basename(s) for s in build.SOURCES]
