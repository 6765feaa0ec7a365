"""The unringing on the device (csrc/t2fit_unring.hip: unring_product_kernel, unring_rows_kernel) against its numpy
statement (fetal_t2mapping_amd/_unring.py): bit for bit, and equal from call to call.  Rows along x and along y over row
lengths below, at and above one and several 32-position tiles (odd and even, odd contracted lengths), row counts that
leave ragged workgroups, shift counts, windows and the largest row; the split over sizes that pad the chains and leave
ragged tiles; the whole stage with NaN and constant slices; raw calls at odd offsets on another stream between guard
words; NULL optional outputs; the workspace size; unring_volume; the near-tie rows of tests/unring_cases.py, which a
kernel with another summation order fails.  tests/test_unring_host.py holds the statement to an independent reference."""
import ctypes as C

import numpy as np
import pytest

import unring_cases as K
from fetal_t2mapping_amd import _abi, _unring

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def t2():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X")
    import fetal_t2mapping_amd as t2

    return t2


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a


def _same(got, want, what):
    got = _bits(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    g, w = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    view = np.uint32 if g.dtype == np.float32 else np.uint8
    bad = np.flatnonzero(g.view(view) != w.view(view))
    assert bad.size == 0, (what, bad.size, bad[:5], g[bad[:5]], w[bad[:5]])


def _want_rows(x, axis, tables, K_, window):
    """The statement of unring_rows on slices (S, ny, nx) along an axis."""
    s, ny, nx = x.shape
    if axis == "x":
        return tuple(a.reshape(s, ny, nx) for a in _unring.unring_rows(x.reshape(-1, nx), tables.hx, tables.ab, *window))
    res = _unring.unring_rows(x.transpose(0, 2, 1).reshape(-1, ny), tables.hy, tables.ab, *window)
    return tuple(np.ascontiguousarray(a.reshape(s, nx, ny).transpose(0, 2, 1)) for a in res)


def _check_rows(t2, x, axis, K_, window, what):
    s, ny, nx = x.shape
    n = nx if axis == "x" else ny
    tables = _unring.Tables(ny, nx, K_) if min(ny, nx) >= 8 else _unring.Tables(n, n, K_)
    want = _want_rows(x, axis, tables, K_, window)
    for again in ("", " (again)"):
        got = t2.unring.unring_rows(x, axis, K_, *window, tables=tables)
        for g, w, name in zip(got, want, ("out", "shift", "tv")):
            _same(g, w, f"{what} {name}{again}")
    return want


@pytest.mark.parametrize("n", [8, 9, 31, 32, 33, 40, 65, 130])
def test_rows_over_row_lengths_along_x_and_y(t2, n):
    window = (1, 3) if n >= 9 else (1, 2)
    x = K.random_slices(2, 9, n, 100 + n)
    want = _check_rows(t2, x, "x", 20, window, f"x n {n}")
    assert len(np.unique(want[1])) > 5 and np.any(want[1] > 20)
    y = np.ascontiguousarray(K.random_slices(2, 9, n, 200 + n).transpose(0, 2, 1))  # (2, n, 9): the columns have length n
    want = _check_rows(t2, y, "y", 20, window, f"y n {n}")
    assert len(np.unique(want[1])) > 5


@pytest.mark.parametrize("rows", [1, 31, 33, 65])
def test_rows_over_row_counts(t2, rows):
    x = K.random_slices(1, rows, 40, 300 + rows)
    _check_rows(t2, x, "x", 20, (1, 3), f"{rows} rows along x")
    _check_rows(t2, np.ascontiguousarray(x.transpose(0, 2, 1)), "y", 20, (1, 3), f"{rows} rows along y")
    if rows == 65:  # the same lines split over slices: a workgroup's 32 lines straddle slices
        x5 = K.random_slices(5, 13, 40, 365)
        _check_rows(t2, x5, "x", 20, (1, 3), "5 x 13 rows along x")
        _check_rows(t2, np.ascontiguousarray(x5.transpose(0, 2, 1)), "y", 20, (1, 3), "5 x 13 rows along y")


@pytest.mark.parametrize("shifts", [1, 3, 20, 32])
def test_rows_over_shift_counts(t2, shifts):
    x = K.random_slices(1, 20, 40, 400 + shifts)
    want = _check_rows(t2, x, "x", shifts, (1, 3), f"K {shifts}")
    assert want[1].max() <= 2 * shifts and want[1].min() == 0
    _check_rows(t2, x, "y", shifts, (1, 3), f"K {shifts} along y")


@pytest.mark.parametrize("window", [(1, 1), (1, 3), (2, 8)])
def test_rows_over_windows(t2, window):
    x = K.random_slices(1, 20, 40, 500 + window[1])
    _check_rows(t2, x, "x", 20, window, f"window {window}")
    _check_rows(t2, x, "y", 20, window, f"window {window} along y")


def test_rows_of_the_largest_length(t2):
    """n = 512, 8 rows, K = 32: 64 lines of samples per lane and the largest images in LDS."""
    x = K.random_slices(1, 8, 512, 600)
    want = _check_rows(t2, x, "x", 32, (1, 3), "n 512")
    assert np.any(want[1] > 32)


def test_rows_on_the_near_ties(t2):
    rows, tables, shift32, differ = K.near_tie_case()
    assert differ >= 10
    x = rows.reshape(1, -1, 40).copy()
    got = t2.unring.unring_rows(x, "x", 20, 1, 3, tables=_unring.Tables(40, 40, 20))
    want = _unring.unring_rows(rows, tables.hx, tables.ab, 1, 3)
    assert np.array_equal(want[1], shift32)
    for g, w, name in zip(got, want, ("out", "shift", "tv")):
        _same(g, w.reshape(x.shape), f"near ties {name}")


@pytest.mark.parametrize("ny,nx", [(8, 8), (9, 31), (33, 40), (24, 65), (32, 32)])
def test_split(t2, ny, nx):
    x = K.random_slices(3, ny, nx, 700 + nx)
    tables = _unring.Tables(ny, nx, 3)
    want = _unring.split(x, tables)
    for again in ("", " (again)"):
        got = t2.unring.unring_split(x, tables)
        _same(got[0], want[0], f"I1 {ny} x {nx}{again}")
        _same(got[1], want[1], f"I2 {ny} x {nx}{again}")


@pytest.mark.parametrize("s", [1, 3, 5])
def test_whole_stage_with_nan_and_constant_slices(t2, s):
    x = K.random_slices(s, 33, 40, 800 + s)
    if s >= 3:
        x[1, 17, 3] = np.nan
    if s == 5:
        x[3] = np.float32(41.7)
    tables = _unring.Tables(33, 40, 20)
    with np.errstate(invalid="ignore"):
        want, skipped, shift, tv = _unring.unring(x, tables, details=True)
    assert skipped == (1 if s >= 3 else 0)
    keep = [i for i in range(s) if not (s >= 3 and i == 1)]  # the slice with the NaN: its shift and tv are not defined bit for bit
    for again in ("", " (again)"):
        got = t2.unring.unring_slices(x, 20, 1, 3, tables=tables, details=True)
        assert got[1] == skipped
        _same(got[0], want, f"S {s} out{again}")
        _same(got[2][:, keep], np.ascontiguousarray(shift[:, keep]), f"S {s} shift{again}")
        _same(got[3][:, keep], np.ascontiguousarray(tv[:, keep]), f"S {s} tv{again}")
    out = _bits(got[0])
    if s >= 3:
        assert out[1].tobytes() == x[1].tobytes()
        alone = _unring.unring(x[:1], tables)[0]
        assert out[0].tobytes() == alone[0].tobytes()  # the neighbours are untouched
    if s == 5:
        assert out[3].tobytes() == x[3].tobytes()
    assert not np.array_equal(out[0], x[0])
    plain, count = t2.unring.unring_slices(x, 20, 1, 3, tables=tables)  # NULL optional outputs
    _same(plain, want, f"S {s} out without the optional outputs")
    assert count == skipped


def test_more_slices_than_a_chunk(t2):
    """70 slices of 9 x 12: the stage and the split work through them 64 at a time."""
    x = K.random_slices(70, 9, 12, 900)
    tables = _unring.Tables(9, 12, 2)
    want, _ = _unring.unring(x, tables, 1, 3)
    got, skipped = t2.unring.unring_slices(x, 2, 1, 3, tables=tables)
    _same(got, want, "70 slices")
    i1 = t2.unring.unring_split(x, tables)[0]
    _same(i1, _unring.split(x, tables)[0], "70 slices, I1")
    assert skipped == 0


def test_raw_calls_at_odd_offsets_on_another_stream_between_guards(t2):
    """Every buffer starts at an odd element offset inside a larger one filled with a guard word; the calls run on a
    non-default stream; the guards around every output and around the workspace survive."""
    import torch

    from fetal_t2mapping_amd._lib import load

    lib = load()
    dev = torch.device("cuda", 0)
    s, ny, nx, k = 3, 33, 40, 20
    n = s * ny * nx
    x = K.random_slices(s, ny, nx, 1000)
    tables = _unring.Tables(ny, nx, k)
    blob = torch.from_numpy(tables.pack()).to(dev)
    p = _abi.T2FitUnringParams()
    lib.t2fit_unring_params_default(C.byref(p))
    need = C.c_size_t(0)
    assert lib.t2fit_unring_workspace_bytes(C.byref(p), s, ny, nx, C.byref(need)) == _abi.OK
    guard = np.float32(-7777.25)

    def guarded(count, offset, dtype=torch.float32, fill=float(guard)):
        return torch.full((count + 2 * offset + 64,), fill, dtype=dtype, device=dev), offset

    src, so = guarded(n, 3)
    src[so:so + n] = torch.from_numpy(x.reshape(-1)).to(dev)
    outs = {name: guarded(cnt, off) for name, cnt, off in (("i1", n, 1), ("i2", n, 5), ("rows", n, 7), ("tv", n, 9), ("out", n, 11),
                                                           ("tv2", 2 * n, 13))}
    shift, sho = guarded(n, 5, torch.int8, 99)
    shift2, sh2o = guarded(2 * n, 3, torch.int8, 99)
    ws = torch.full((need.value // 4 + 256,), float(guard), dtype=torch.float32, device=dev)
    ws_off = (-(ws.data_ptr()) % 256) // 4 + 64  # 256-byte aligned, with guard words on both sides
    ptr = lambda name: outs[name][0].data_ptr() + 4 * outs[name][1]
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    skipped = C.c_int64(-1)
    with torch.cuda.stream(stream):
        st = C.c_void_p(stream.cuda_stream)
        wptr = ws.data_ptr() + 4 * ws_off
        assert wptr % 256 == 0
        rc = lib.t2fit_unring_split_dev(blob.data_ptr(), src.data_ptr() + 4 * so, s, ny, nx, ptr("i1"), ptr("i2"), wptr, need.value, st)
        assert rc == _abi.OK, lib.t2fit_last_error()
        rc = lib.t2fit_unring_rows_dev(C.byref(p), blob.data_ptr(), src.data_ptr() + 4 * so, s, ny, nx, 1, ptr("rows"), shift.data_ptr() + sho,
                                       ptr("tv"), st)
        assert rc == _abi.OK, lib.t2fit_last_error()
        rc = lib.t2fit_unring_dev(C.byref(p), blob.data_ptr(), src.data_ptr() + 4 * so, s, ny, nx, ptr("out"), shift2.data_ptr() + sh2o,
                                  ptr("tv2"), C.byref(skipped), wptr, need.value, st)
        assert rc == _abi.OK, lib.t2fit_last_error()
    stream.synchronize()
    assert skipped.value == 0
    i1, i2 = _unring.split(x, tables)
    ro, rs, rtv = _want_rows(x, "y", tables, k, (1, 3))
    wo, _, wshift, wtv = _unring.unring(x, tables, details=True)
    want = {"i1": i1, "i2": i2, "rows": ro, "tv": rtv, "out": wo, "tv2": wtv}
    for name, (buf, off) in outs.items():
        host = buf.cpu().numpy()
        w = want[name].reshape(-1)
        _same(host[off:off + w.size], w, f"raw {name}")
        assert np.all(host[:off] == guard) and np.all(host[off + w.size:] == guard), name
    for buf, off, w in ((shift, sho, rs), (shift2, sh2o, wshift)):
        host = buf.cpu().numpy()
        _same(host[off:off + w.size], w.reshape(-1), "raw shift")
        assert np.all(host[:off] == 99) and np.all(host[off + w.size:] == 99)
    host = ws.cpu().numpy()
    assert np.all(host[:ws_off] == guard) and np.all(host[ws_off + need.value // 4:] == guard)
    assert np.all(src.cpu().numpy()[so:so + n] == x.reshape(-1))  # the input is not written


def test_workspace_does_not_depend_on_the_shift_count(t2):
    from fetal_t2mapping_amd._lib import load

    lib = load()
    p = _abi.T2FitUnringParams()
    lib.t2fit_unring_params_default(C.byref(p))
    sizes = []
    for k in (1, 32):
        p.K = k
        need = C.c_size_t(0)
        assert lib.t2fit_unring_workspace_bytes(C.byref(p), 57, 256, 256, C.byref(need)) == _abi.OK
        sizes.append(need.value)
    assert sizes[0] == sizes[1] and sizes[0] < 7 * 57 * 256 * 256 * 4


def test_refusals_on_the_device(t2):
    import torch

    x = torch.zeros((2, 33, 40), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="float32"):
        t2.unring.unring_slices(x.double())
    with pytest.raises(ValueError, match="K"):
        t2.unring.unring_slices(x, K=33)
    with pytest.raises(ValueError, match="the tables were built for"):
        t2.unring.unring_slices(x, K=20, tables=_unring.Tables(33, 40, 3))
    with pytest.raises(ValueError, match="the tables were built for"):
        t2.unring.unring_split(x, _unring.Tables(40, 33, 3))
    with pytest.raises(ValueError, match="out must be a contiguous float32 tensor"):
        t2.unring.unring_slices(x, out=torch.zeros((2, 33, 41), dtype=torch.float32, device="cuda"))


@pytest.mark.parametrize("slice_axis", [0, 1])
def test_unring_volume(t2, slice_axis):
    import torch

    block = np.ascontiguousarray(K.random_slices(10, 24, 33, 1100).reshape(2, 5, 24, 33))
    if slice_axis == 0:   # the slices are the (Y, X) planes
        slices = block.reshape(-1, 24, 33)
        want = _unring.unring(slices, _unring.Tables(24, 33, 20))[0].reshape(block.shape)
    else:                 # the slices are the (Z, X) planes, which must meet the size limit: a block with Z = 9
        block = np.ascontiguousarray(K.random_slices(2 * 9, 5, 33, 1101).reshape(2, 9, 5, 33))
        slices = np.ascontiguousarray(block.transpose(0, 2, 1, 3)).reshape(-1, 9, 33)
        want = _unring.unring(slices, _unring.Tables(9, 33, 20))[0].reshape(2, 5, 9, 33).transpose(0, 2, 1, 3)
    info = {}
    got = t2.unring.unring_volume(block, slice_axis=slice_axis, info=info)
    assert isinstance(got, np.ndarray) and info == {"skipped": 0}
    _same(got, np.ascontiguousarray(want), f"unring_volume axis {slice_axis}")
    dev = t2.unring.unring_volume(torch.from_numpy(block).cuda(), slice_axis=slice_axis)
    assert torch.is_tensor(dev) and dev.is_cuda
    _same(dev, np.ascontiguousarray(want), f"unring_volume axis {slice_axis}, tensor")
    out = np.zeros_like(block)
    assert t2.unring.unring_volume(block, slice_axis=slice_axis, out=out) is out
    _same(out, np.ascontiguousarray(want), "out=")
    if slice_axis == 1:
        with pytest.raises(ValueError, match="unring"):
            t2.unring.unring_volume(np.zeros((2, 5, 24, 33), np.float32), slice_axis=1)  # a 5 x 33 plane is below the limits


def test_recon_unrings_the_raw_stacks_and_writes_them(t2, tmp_path, monkeypatch):
    """recon.py --unring on a tiny synthetic tree: the files under derivatives/unring hold, bit for bit, what the Python call
    gives on the raw stacks; recon_1mm is the reconstruction of those; cli.py's --reconstruct --recon_unring reconstructs the
    same volumes in memory; and without the flag recon_1mm is what it was."""
    import glob
    import os
    import sys

    import pandas as pd

    monkeypatch.setitem(sys.modules, "SimpleITK", None)  # the package's NIfTI reader; an earlier test may have faked one
    from fetal_t2mapping_amd import _resample as R
    from fetal_t2mapping_amd import cli, nifti, recon

    directions = {"ax": np.eye(3), "cor": np.array([[1, 0, 0], [0, 0, 1], [0, 1, 0.0]]), "sag": np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0.0]])}
    size, spacing = (26, 22, 6), (1.0, 1.0, 4.5)
    geoms = {}
    for o, d in directions.items():
        extent = d @ (np.array(spacing) * (np.array(size) - 1) / 2.0)
        geoms[o] = R.Geometry(size, spacing, np.array([2.0, -3.0, 5.0]) - extent, d.ravel())
    te_ms = [114, 202]
    stacks = {o: K.random_slices(2 * 6, 22, 26, 1200 + i).reshape(2, 6, 22, 26) for i, o in enumerate(geoms)}
    bids = str(tmp_path / "projects") + "/"
    rows, run = [], 0
    for i, te in enumerate(te_ms):
        for o in ("ax", "cor", "sag"):
            run += 1
            acq = {"prj": "prj-900", "sub": "sub-001", "ses": "ses-01", "run": f"run-{run:02d}", "EchoTime": te / 1000.0,
                   "CoilString": "HeadNeck", "ImageOrientationPatientSTR": o}
            rows.append(acq)
            g = geoms[o]
            nifti.WriteImage(nifti.Image(stacks[o][i], g.GetSpacing(), g.GetOrigin(), g.GetDirection()), cli.get_img_path(bids, acq, "anat"))
    md = pd.DataFrame(rows)

    plain = recon.process_recon(md, bids, denoise=False)
    want_plain, _ = R.reconstruct(stacks, geoms)
    for i, path in enumerate(plain):
        assert np.asarray(nifti.ReadImage(path).arr, np.float32).tobytes() == want_plain[i].tobytes()
    assert not os.path.exists(os.path.join(bids, "prj-900", "derivatives", "unring"))

    args = recon.parse_arguments(["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo", "--lf", "--unring", "--unring_shifts", "5",
                                  "--unring_window", "1,2", "--write_unring"])
    written = recon.process_recon(md, bids, denoise=False, unring=args.unring_args, write_unring=args.write_unring)
    unrung = {o: t2.unring.unring_volume(stacks[o], slice_axis=0, K=5, min_w=1, max_w=2) for o in geoms}
    files = sorted(glob.glob(os.path.join(bids, "prj-900", "derivatives", "unring", "sub-001", "ses-01", "anat", "*.nii.gz")))
    assert [os.path.basename(f) for f in files] == [f"sub-001_ses-01_run-{r:02d}_T2w_unring.nii.gz" for r in range(1, 7)]
    for acq, f in zip(rows, files):
        o, i = acq["ImageOrientationPatientSTR"], te_ms.index(int(round(acq["EchoTime"] * 1000)))
        img = nifti.ReadImage(f)
        assert img.arr.dtype == np.float32 and img.arr.tobytes() == unrung[o][i].tobytes(), f
        assert np.allclose(img.GetSpacing(), spacing) and np.allclose(img.GetOrigin(), geoms[o].GetOrigin(), atol=1e-4)
        assert not np.array_equal(img.arr, stacks[o][i])
    want, _ = R.reconstruct(unrung, geoms)
    for i, path in enumerate(written):
        assert np.asarray(nifti.ReadImage(path).arr, np.float32).tobytes() == want[i].tobytes()
    assert want[0].tobytes() != want_plain[0].tobytes()
    a = cli.parse_arguments(["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo", "--gaussian", "--lf", "--sim", "x", "--reconstruct",
                             "--recon_unring", "--recon_unring_shifts", "5", "--recon_unring_window", "1,2"])
    kw = {k: v for k, v in a.reconstruct_args.items()}
    volumes, _ = recon.reconstruct_subject(recon._sitk(), bids, md, "sub-001", "ses-01", **kw)
    for v, w in zip(volumes, want):
        assert np.asarray(v, np.float32).tobytes() == w.tobytes()
