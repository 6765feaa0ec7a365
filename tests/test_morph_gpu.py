"""The mask-building stage on the device (csrc/t2fit_morph.hip) against its numpy statement (fetal_t2mapping_amd/_morph.py)
and against scipy.ndimage, exactly: threshold, run-list dilation / erosion / closing / opening over shapes that exercise
the word tail, both borders, in place and out of place; hole filling in 3-D and per plane, with a channel that needs
several tile sweeps; seed labels and relabelling; the recipes against restatements of the reference's host functions;
repeatability; argument errors; recon.py --phantom_masks and cli.py --build_mask phantom on files.  With the cases of
tests/morph_cases.py: dilation and erosion where about half of the voxels change, every run offset against a response
pasted from the definition, the sweep counts of the hole filling against a model of its tiles, degenerate volumes, and
raw calls into guarded memory."""
import ctypes as C
import glob
import json
import os
import sys

import morph_cases as K
import numpy as np
import pandas as pd
import pytest
from scipy import ndimage as ndi

from fetal_t2mapping_amd import _abi
from fetal_t2mapping_amd import _morph as M

pytestmark = pytest.mark.gpu

SHAPES = [(24, 40, 48), (17, 33, 70), (5, 7, 130), (1, 9, 64)]


@pytest.fixture(scope="module")
def t2():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X")
    import fetal_t2mapping_amd as t2

    return t2


def _host(t):
    return t.cpu().numpy().astype(bool)


def _volume(shape, seed, p=0.03):
    rng = np.random.default_rng(seed)
    a = rng.random(shape) < p
    a[0, 0, 0] = a[-1, -1, -1] = a[0, -1, 0] = a[-1, 0, -1] = True  # something on every face
    return a


def _two_runs():
    fp = np.zeros((3, 5, 9), bool)
    fp[1, 2, 0:3] = fp[1, 2, 6:9] = True
    fp[0, 4, 8] = True
    fp[2, 1, 2:5] = True
    return fp


ELEMENTS = {"ball2": M.ball(2), "ball234": M.ball((2, 3, 4)), "cross1": M.cross(1), "two_runs": _two_runs(),
            "flat5x5": np.ones((1, 5, 5), bool), "wide": M.box((0, 1, 32))}


def _scipy(op, a, fp, iterations, border):
    """scipy's result for `iterations` >= 1 as that many single passes, which is its definition.  (Its one-call form
    with iterations > 1 overruns the heap when the structure is larger than the volume along an axis, as here on the
    single-slice and narrow shapes.)"""
    for _ in range(iterations):
        a = op(a, fp, border_value=border)
    return a


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("border", [0, 1])
def test_dilate_erode_equal_statement_and_scipy(t2, shape, border):
    import torch

    a = _volume(shape, 11)
    for name, fp in ELEMENTS.items():
        for it in (1, 2):
            d = _host(t2.binary_dilate(a, fp, iterations=it, border_value=border))
            e = _host(t2.binary_erode(torch.from_numpy(a).cuda(), fp, iterations=it, border_value=border))
            assert np.array_equal(d, M.dilate(a, fp, it, border)), (name, it)
            assert np.array_equal(e, M.erode(a, fp, it, border)), (name, it)
            assert np.array_equal(d, _scipy(ndi.binary_dilation, a, fp, it, border)), (name, it)
            assert np.array_equal(e, _scipy(ndi.binary_erosion, a, fp, it, border)), (name, it)


@pytest.mark.parametrize("shape", SHAPES)
def test_close_open_both_forms_in_place_and_threshold(t2, shape):
    import torch

    rng = np.random.default_rng(12)
    vol = rng.normal(50.0, 40.0, shape).astype(np.float32)
    vol[0, 0, 0] = np.nan
    m = t2.binary_threshold(vol, 100.0)
    assert m.dtype == torch.uint8 and m.is_cuda and np.array_equal(_host(m), np.nan_to_num(vol, nan=0.0) >= 100.0)
    ints = rng.integers(-5, 6, shape).astype(np.int32)
    assert np.array_equal(_host(t2.binary_threshold(torch.from_numpy(ints).cuda(), -1, 2)), (ints >= -1) & (ints <= 2))
    a = _volume(shape, 13, 0.08)
    fp = M.ball(2)
    for border in (0, 1):
        assert np.array_equal(_host(t2.binary_close(a, fp, border_value=border)), ndi.binary_closing(a, fp, border_value=border))
        assert np.array_equal(_host(t2.binary_open(a, fp, border_value=border)), ndi.binary_opening(a, fp, border_value=border))
    padded = np.pad(a, 4)
    want = _scipy(ndi.binary_erosion, _scipy(ndi.binary_dilation, padded, fp, 2, 0), fp, 2, 0)[4:-4, 4:-4, 4:-4]
    buf = torch.from_numpy(a.astype(np.uint8)).cuda()
    got = t2.binary_close(buf, fp, iterations=2, unbounded=True, out=buf)  # in place
    assert got.data_ptr() == buf.data_ptr()
    assert np.array_equal(_host(buf), want) and np.array_equal(want, M.close(a, fp, 2, unbounded=True))
    assert np.array_equal(_host(t2.binary_open(a, fp, unbounded=True)), M.open(a, fp, unbounded=True))


@pytest.mark.parametrize("radius", [10, 15])
def test_large_balls(t2, radius):
    a = _volume((40, 48, 70), 14, 0.0005)
    fp = M.ball(radius)
    assert np.array_equal(_host(t2.binary_dilate(a, fp)), ndi.binary_dilation(a, fp))
    b = ndi.binary_dilation(a, M.ball(radius + 2), border_value=1)
    for border in (0, 1):
        got = _host(t2.binary_erode(b, fp, border_value=border))
        assert np.array_equal(got, ndi.binary_erosion(b, fp, border_value=border))
        assert np.array_equal(got, M.erode(b, fp, 1, border))


def _shells(shape, seed=5, n=40):
    rng = np.random.default_rng(seed)
    pts = np.zeros(shape, bool)
    pts[tuple(rng.integers(0, s, n) for s in shape)] = True
    blob = ndi.binary_dilation(pts, ndi.generate_binary_structure(3, 1), iterations=min(4, max(1, min(shape) // 3)))
    return blob & ~ndi.binary_erosion(blob, ndi.generate_binary_structure(3, 1), border_value=1)


@pytest.mark.parametrize("shape", SHAPES + [(24, 40, 45)])
def test_fill_holes_3d_and_per_plane(t2, shape):
    a = _shells(shape)
    got = _host(t2.fill_holes(a))
    assert np.array_equal(got, ndi.binary_fill_holes(a)) and np.array_equal(got, M.fill_holes(a))
    if shape == (24, 40, 45):
        assert int(got.sum() - a.sum()) > 0
    for axis in (0, 1, 2):
        want = np.stack([ndi.binary_fill_holes(np.take(a, i, axis)) for i in range(a.shape[axis])], axis)
        got = _host(t2.fill_holes(a, slice_axis=axis))
        assert np.array_equal(got, want) and np.array_equal(got, M.fill_holes(a, axis)), axis


def test_fill_holes_serpentine_channel_needs_several_sweeps(t2):
    a = np.ones((6, 80, 300), bool)  # tiles are 8 x 8 rows by 256 voxels of x: the channel crosses them back and forth
    for k, y in enumerate(range(1, 79, 2)):
        a[2, y, 1:299] = False
        a[2, y + 1, 298 if k % 2 == 0 else 1] = False
    a[2, 0, 1] = False            # the channel's mouth, on the border
    a[4, 40:44, 30:34] = False    # a cavity nothing reaches
    got, sweeps = t2.fill_holes(a, return_sweeps=True)
    got = _host(got)
    want = ndi.binary_fill_holes(a)
    print(f"serpentine: {sweeps} sweeps")
    assert sweeps > 1
    assert np.array_equal(got, want)
    assert not got[2, 77, 150] and got[4, 41, 31]
    again, sweeps2 = t2.fill_holes(a, return_sweeps=True)
    assert sweeps2 == sweeps and np.array_equal(_host(again), got)


def test_seed_labels_and_relabel(t2):
    import torch

    shape = (20, 26, 70)
    seeds = [(10, 12, 9), (14, 12, 9), (0, 0, 0), (69, 25, 19), (66, 3, 5)]
    for dtype in ("uint8", "int32"):
        got = t2.seed_labels(shape, seeds, M.ball(3), dtype=dtype)
        want = M.seed_labels(shape, seeds, range(1, 6), M.ball(3), np.dtype(dtype))
        assert str(got.dtype) == "torch." + dtype and np.array_equal(got.cpu().numpy(), want)
    got = t2.phantom_labels(shape, seeds[:3], radius=6).cpu().numpy()
    want = np.zeros(shape, np.uint8)
    for i, (x, y, z) in enumerate(seeds[:3]):  # the reference: a seed voxel dilated by the ball, times its label, maximum
        one = np.zeros(shape, bool)
        one[z, y, x] = True
        want = np.maximum(want, ndi.binary_dilation(one, M.ball(6)).astype(np.uint8) * np.uint8(i + 1))
    assert np.array_equal(got, want)
    assert got[9, 12, 12] == 2 and got[9, 12, 5] == 1  # the overlap holds the larger label
    assert 0 < int((got == 3).sum()) < int(M.ball(6).sum())  # the corner seed is clipped
    custom = t2.seed_labels(shape, seeds[:2], M.cross(1), labels=[7, 3], dtype="int32").cpu().numpy()
    assert custom[9, 12, 10] == 7 and custom[9, 12, 14] == 3 and int((custom > 0).sum()) == 14
    ids = np.random.default_rng(3).integers(-3, 70, shape).astype(np.int32)
    assert np.array_equal(t2.synthseg_to_feta(ids).cpu().numpy(), M.relabel(ids, M.feta_lut()))
    assert np.array_equal(t2.relabel(torch.from_numpy(ids.astype(np.int64)).cuda(), [5, 6]).cpu().numpy(), M.relabel(ids, [5, 6]))
    assert np.array_equal(_host(t2.mask_from_labels(ids)), ids >= 1)


def _phantom_volume(shape, seed=21):
    """A bright cylinder along z with dark vials and noise, dim background."""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")
    cy, cx = shape[1] / 2.0, shape[2] / 2.0
    r = np.hypot(y - cy, x - cx)
    vol = np.where((r < min(shape[1:]) * 0.33) & (z > 2) & (z < shape[0] - 3), 400.0, 5.0)
    for k in range(5):
        vy, vx = cy + 6 * np.cos(k * 1.3), cx + 6 * np.sin(k * 1.3)
        vol[np.hypot(y - vy, x - vx) < 2.2] = 20.0
    return (vol + rng.normal(0.0, 3.0, shape)).astype(np.float32)


def _reference_phantom_mask(vol, close_radius, dilate_radius):
    m = ndi.binary_fill_holes(vol >= 100)
    p = np.pad(m, close_radius)
    c = ndi.binary_erosion(ndi.binary_dilation(p, M.ball(close_radius)), M.ball(close_radius))
    c = c[close_radius:-close_radius, close_radius:-close_radius, close_radius:-close_radius]
    return ndi.binary_dilation(c, M.ball(dilate_radius))


def _reference_build_mask(vol):
    out = np.zeros(vol.shape, np.uint8)
    for i in range(vol.shape[2]):
        bw = ndi.binary_fill_holes(vol[:, :, i] > 1.0)
        bw = ndi.binary_dilation(bw, structure=np.ones((5, 5)))
        out[:, :, i] = ndi.binary_erosion(bw, structure=np.ones((5, 5)))
    return out


@pytest.mark.parametrize("shape,radii", [((30, 44, 70), (3, 2)), ((32, 36, 40), (15, 10))])
def test_phantom_mask_equals_the_reference_recipe(t2, shape, radii):
    import torch

    vol = _phantom_volume(shape)
    want = _reference_phantom_mask(vol, *radii)
    got = t2.phantom_mask(vol, close_radius=radii[0], dilate_radius=radii[1])
    assert got.dtype == torch.uint8 and np.array_equal(_host(got), want)
    assert 0 < int(want.sum()) and int((vol >= 100).sum()) < int(want.sum())
    again = t2.phantom_mask(torch.from_numpy(vol).cuda(), close_radius=radii[0], dilate_radius=radii[1])
    assert torch.equal(got, again)  # bit-identical from call to call, numpy and tensor input


@pytest.mark.parametrize("shape", [(24, 40, 48), (17, 33, 70)])
def test_build_mask_equals_the_reference_recipe(t2, shape):
    rng = np.random.default_rng(22)
    vol = _phantom_volume(shape) * (rng.random(shape) > 0.2)
    vol[:, :3] = 0.5
    vol = vol.astype(np.float32)
    vol[3, 5, 7] = 1.0  # the threshold is strict
    want = _reference_build_mask(vol)
    got = t2.build_mask(vol).cpu().numpy()
    assert np.array_equal(got, want) and 0 < int(want.sum()) < want.size


def test_argument_errors_do_not_touch_the_device(t2):
    from fetal_t2mapping_amd._lib import load

    lib = load()
    need = C.c_size_t(0)
    assert lib.t2fit_morph_workspace_bytes(8, 8, 8, 0, C.byref(need)) == _abi.OK and need.value > 0
    p = C.c_void_p(1 << 20)  # never dereferenced: every call below fails its checks first
    runs = np.array([[0, 0, -1, 1]], np.int32)

    def morph(size, runs=runs, op=0, border=0, ws=p, ws_bytes=None, in_=p, out=p, flags=0, it=1):
        size = np.asarray(size, np.int32)
        return lib.t2fit_binary_morph_dev(op, in_, out, 8, 8, 8, size.ctypes.data, runs.ctypes.data, len(runs), it, border, flags,
                                          ws, need.value if ws_bytes is None else ws_bytes, None)

    cases = {
        "workspace has": morph((1, 1, 3), ws_bytes=need.value - 1),
        "radius exceeds 32": morph((1, 1, 67), runs=np.array([[0, 0, -33, 33]], np.int32)),
        "odd": morph((1, 1, 4)),
        "NULL": morph((1, 1, 3), in_=None),
        "workspace_dev is NULL": morph((1, 1, 3), ws=None),
        "unknown op": morph((1, 1, 3), op=4),
        "border_value": morph((1, 1, 3), border=2),
        "leaves the footprint": morph((1, 1, 1)),
        "iterations": morph((1, 1, 3), it=0),
        "UNBOUNDED": morph((1, 1, 3), flags=1),
    }
    for text, rc in cases.items():
        assert rc == _abi.E_INVALID, text
    assert morph((1, 1, 4)) == _abi.E_INVALID and b"odd" in lib.t2fit_last_error()
    assert morph((1, 1, 67), runs=np.array([[0, 0, -33, 33]], np.int32)) == _abi.E_INVALID and b"32" in lib.t2fit_last_error()
    assert lib.t2fit_fill_holes_dev(p, p, 8, 8, 8, 3, p, need.value, None, None) == _abi.E_INVALID
    assert b"slice_axis" in lib.t2fit_last_error()
    assert lib.t2fit_fill_holes_dev(None, p, 8, 8, 8, 0, p, need.value, None, None) == _abi.E_INVALID
    assert lib.t2fit_fill_holes_dev(p, p, 8, 0, 8, 0, p, need.value, None, None) == _abi.E_INVALID
    assert lib.t2fit_fill_holes_dev(p, p, 8, 8, 8, 0, p, 16, None, None) == _abi.E_INVALID
    assert lib.t2fit_binary_threshold_dev(None, 0, 8, 0.0, 1.0, p, None) == _abi.E_INVALID
    assert lib.t2fit_binary_threshold_dev(p, 2, 8, 0.0, 1.0, p, None) == _abi.E_INVALID
    assert lib.t2fit_relabel_dev(p, 8, None, 4, p, None) == _abi.E_INVALID
    seeds, labels, size = np.zeros((1, 3), np.int32), np.array([300], np.int32), np.array([1, 1, 3], np.int32)
    assert lib.t2fit_seed_labels_dev(seeds.ctypes.data, labels.ctypes.data, 1, size.ctypes.data, runs.ctypes.data, 1, 8, 8, 8, p,
                                     _abi.MORPH_U8, p, need.value, None) == _abi.E_INVALID
    assert b"label" in lib.t2fit_last_error()
    with pytest.raises(ValueError, match="odd"):
        t2.binary_dilate(np.zeros((4, 4, 4), bool), np.ones((2, 3, 3), bool))


# ---- the drivers, on files ----------------------------------------------------------------------------------------------
TE_MS = [114, 202, 299]
SEEDS = [[16, 12, 6], [24, 20, 10], [1, 1, 1]]


def _write_phantom_subject(tmp_path, fake):
    """Three echoes of a decaying phantom as recon_1mm volumes of the npy-backed SimpleITK stand-in."""
    from fetal_t2mapping_amd import cli

    bids = str(tmp_path / "projects") + "/"
    shape = (16, 32, 40)
    base = _phantom_volume(shape, seed=31)
    rows, vols = [], []
    for i, te in enumerate(TE_MS):
        acq = {"prj": "prj-901", "sub": "sub-001", "ses": "ses-01", "run": f"run-{i + 1:02d}", "EchoTime": te / 1000.0,
               "CoilString": "HeadNeck", "ImageOrientationPatientSTR": "ax"}
        rows.append(acq)
        vol = (base * np.exp(-te / 180.0) * 2.0).astype(np.float32)
        vols.append(vol)
        np.save(cli.get_img_path(bids, acq, cli.recon_dirname).replace(" ", "") + ".npy", vol)
    return bids, pd.DataFrame(rows), vols


def test_recon_phantom_masks_and_cli_build_mask_phantom(t2, tmp_path, monkeypatch):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import fake_sitk

    fake = fake_sitk.install()
    monkeypatch.setitem(sys.modules, "SimpleITK", fake)
    from fetal_t2mapping_amd import cli, recon

    bids, md, vols = _write_phantom_subject(tmp_path, fake)
    seeds_file = tmp_path / "seeds.json"
    seeds_file.write_text(json.dumps(SEEDS))
    radii = {"close_radius": 4, "dilate_radius": 2}
    written = recon.process_phantom_masks(md, bids, seeds=recon.load_seeds(str(seeds_file)), label_radius=3, **radii)
    anat = os.path.join(bids, "prj-901", "derivatives", "{}", "sub-001", "ses-01", "anat")
    want_labels = M.seed_labels(vols[0].shape, SEEDS, [1, 2, 3], M.ball(3))
    assert len(written) == 6
    for i, te in enumerate(TE_MS):
        mask_path = os.path.join(anat.format("recon_1mm_mask"), f"sub-001_ses-01_te-{te}_recon_1mm_mask.nii.gz")
        label_path = os.path.join(anat.format("recon_1mm_label"), f"sub-001_ses-01_te-{te}_recon_1mm_label.nii.gz")
        assert mask_path in fake.written and label_path in fake.written, sorted(fake.written)
        mask, label = fake.written[mask_path].arr, fake.written[label_path].arr
        assert mask.dtype == np.uint8 and label.dtype == np.uint8
        assert np.array_equal(mask.astype(bool), _reference_phantom_mask(vols[i], 4, 2))
        assert np.array_equal(label, want_labels)
        np.save(mask_path + ".npy", mask), np.save(label_path + ".npy", label)  # the files a later run reads

    def run(sim, extra):
        args = cli.parse_arguments(["--path", str(tmp_path), "--csv", "x.csv", "--in_vitro", "--gaussian", "--lf", "--sim", sim] + extra)
        fit, fit_params = cli.t2map.set_fit_params(args)
        before = set(fake.written)
        cli.process_t2maps(md, bids, TE_MS, fit, fit_params, True, True, True, False, False, sim,
                           **({"build_mask": dict(args.build_mask_args, label_radius=3, **radii)} if args.build_mask_args else {}))
        new = sorted(set(fake.written) - before)
        maps = [fake.written[p].arr for p in new]
        csv = sorted(glob.glob(os.path.join(anat.format(cli.t2map_dirname), f"*sim-{sim}_*.csv")))
        assert len(maps) == 4 and len(csv) == 1, (new, csv)
        return maps, open(csv[0]).read()

    maps_files, csv_files = run("files", [])
    maps_built, csv_built = run("built", ["--build_mask", "phantom", "--phantom_seeds", str(seeds_file)])
    for a, b in zip(maps_files, maps_built):
        assert a.tobytes() == b.tobytes()
    assert csv_files == csv_built and np.count_nonzero(maps_files[0]) > 500
    with pytest.raises(SystemExit):
        cli.parse_arguments(["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo", "--gaussian", "--lf", "--sim", "x",
                             "--build_mask", "phantom", "--phantom_seeds", str(seeds_file)])


# ---- balanced inputs: about half of the voxels change (morph_cases.py) -----------------------------------------------------
def _tensor(a):
    import torch

    return torch.from_numpy(np.asarray(a).astype(np.uint8)).cuda()


@pytest.mark.parametrize("shape", K.GENERAL_SHAPES + K.FLAT_SHAPES)
def test_balanced_dilate_erode_equal_statement_and_scipy(t2, shape):
    import torch

    device = {"dilate": t2.binary_dilate, "erode": t2.binary_erode}
    in_place = set()
    for i, (name, n, border, op) in enumerate(K.cases(shape, K.ELEMENTS, (1, 2), general=shape in K.GENERAL_SHAPES)):
        a, fp = np.array(K.balanced(shape, name, n, op)), K.ELEMENTS[name]  # (a writable copy)
        got = device[op](a if i % 2 else _tensor(a), fp, iterations=n, border_value=border)  # numpy and tensor input in turn
        assert np.array_equal(_host(got), getattr(M, op)(a, fp, n, border)), (name, n, border, op)
        assert np.array_equal(_host(got), K.expected(shape, name, n, border, op)), (name, n, border, op)
        again = device[op](_tensor(a) if i % 2 else a, fp, iterations=n, border_value=border)
        assert torch.equal(got, again), (name, n, border, op)  # the same bytes from a second call
        if name == "two_runs" and n == 2 and border == 1 and op not in in_place:
            in_place.add(op)
            buf = _tensor(a)
            assert device[op](buf, fp, iterations=n, border_value=border, out=buf).data_ptr() == buf.data_ptr()
            assert torch.equal(buf, got), op
    assert in_place == {"dilate", "erode"}


@pytest.mark.parametrize("shape", K.GENERAL_SHAPES + K.FLAT_SHAPES)
def test_balanced_close_open_equal_statement_and_scipy(t2, shape):
    import torch

    device = {"close": t2.binary_close, "open": t2.binary_open}
    turn = 0
    todo = [(name, 1, False) for name in sorted(K.ELEMENTS)] + [("two_runs", 2, False), ("wide", 2, False)]
    for name, n, unbounded in todo + [("two_runs", 3, True), ("ball234", 1, True)]:  # two_runs three times: a reach of 12
        fp = K.ELEMENTS[name]
        for op, source in (("close", "dilate"), ("open", "erode")):
            a = np.array(K.balanced(shape, name, n, source))
            for border in ((0,) if unbounded else (0, 1)):
                turn += 1
                got = device[op](a if turn % 2 else _tensor(a), fp, iterations=n, border_value=border, unbounded=unbounded)
                what = (name, n, unbounded, op, border)
                assert np.array_equal(_host(got), getattr(M, op)(a, fp, n, border, unbounded)), what
                want = K.scipy_close_open(op, a, fp, n, border, unbounded)
                assert np.array_equal(_host(got), want), what
                assert K.is_thin(shape, name, n) or (want.any() and not want.all()), what
                again = device[op](_tensor(a) if turn % 2 else a, fp, iterations=n, border_value=border, unbounded=unbounded)
                assert torch.equal(got, again), what


# ---- every run offset, by impulse response -----------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["dilate", "dual", "erode0"])
@pytest.mark.parametrize("name", sorted(K.IMPULSES))
def test_every_run_offset_equals_the_pasted_response(t2, name, which):
    a = np.array(K.impulse_volume(name))
    element = M.footprint_runs(K.all_runs_footprint())
    assert len(element[0]) == 2145
    if which == "dilate":
        got, statement = t2.binary_dilate(a, element), M.dilate(a, element)
    else:
        border = 1 if which == "dual" else 0
        got, statement = t2.binary_erode(~a, element, border_value=border), M.erode(~a, element, 1, border)
    want = K.impulse_expected(name, which)
    got = _host(got)
    wrong = np.argwhere(got != want)
    assert len(wrong) == 0, (len(wrong), wrong[:5].tolist())
    assert np.array_equal(got, statement)
    assert want.any() and not want.all()


# ---- hole filling: sweep counts and degenerate volumes -----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.CHANNELS))
def test_fill_holes_channel_sweep_counts(t2, name):
    import torch

    a, axis, by_hand = K.CHANNELS[name]
    model, model_sweeps = K.sweep_model(a, axis)
    want = ndi.binary_fill_holes(a) if axis is None else K.fill_per_plane(a, axis)
    assert np.array_equal(model, want) and model_sweeps == by_hand
    got, sweeps = t2.fill_holes(a, slice_axis=axis, return_sweeps=True)
    print(f"{name}: {sweeps} sweeps on the device, {model_sweeps} in the model")
    assert np.array_equal(_host(got), want)
    assert sweeps == model_sweeps
    again, sweeps2 = t2.fill_holes(_tensor(a), slice_axis=axis, return_sweeps=True)
    assert sweeps2 == sweeps and torch.equal(again, got)


@pytest.mark.parametrize("name", sorted(K.DEGENERATE))
def test_fill_holes_degenerate_volumes(t2, name):
    a = K.DEGENERATE[name]
    for axis in (None, 0, 1, 2):
        want = ndi.binary_fill_holes(a) if axis is None else K.fill_per_plane(a, axis)
        got, sweeps = t2.fill_holes(a, slice_axis=axis, return_sweeps=True)
        assert np.array_equal(_host(got), want), axis
        assert np.array_equal(want, M.fill_holes(a, axis)), axis
        assert sweeps == K.sweep_model(a, axis)[1], axis


# ---- raw calls into guarded memory ---------------------------------------------------------------------------------------------
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
        return host[self.at:self.at + self.nbytes]


def test_raw_calls_keep_to_the_workspace_and_the_output_and_leave_the_input(t2):
    import torch

    from fetal_t2mapping_amd._lib import load

    lib = load()
    shape = (17, 33, 70)
    n = int(np.prod(shape))
    fp = K.two_runs()
    runs, size = M.footprint_runs(fp)
    size = np.asarray(size, np.int32)
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)

    def workspace(reach):
        need = C.c_size_t(0)
        assert lib.t2fit_morph_workspace_bytes(*shape, reach, C.byref(need)) == _abi.OK
        return _Guarded(need.value)  # exactly as long as the call asks for

    def check(ws, inp, a):
        assert np.any(ws.bytes() != 0xA5)  # used, and nothing written before or after it
        assert np.array_equal(inp.bytes(), a.astype(np.uint8).ravel())  # the input is as it was

    with torch.cuda.stream(stream):
        # erosion by the asymmetric element, border 1, twice
        a = K.balanced(shape, "two_runs", 2, "erode")
        inp, out, ws = _Guarded(n, 1, a.astype(np.uint8)), _Guarded(n, 3), workspace(0)
        assert inp.ptr % 2 == 1
        assert lib.t2fit_binary_morph_dev(_abi.MORPH_ERODE, inp.ptr, out.ptr, *shape, size.ctypes.data, runs.ctypes.data, len(runs),
                                          2, 1, 0, ws.ptr, ws.nbytes, st) == _abi.OK
        stream.synchronize()
        assert np.array_equal(out.bytes().reshape(shape), M.erode(a, fp, 2, 1))
        check(ws, inp, a)
        # the closing on the unbounded domain: the packed grid is larger than the volume by the reach on every side
        a = K.balanced(shape, "two_runs", 2, "dilate")
        inp, out, ws = _Guarded(n, 5, a.astype(np.uint8)), _Guarded(n, 7), workspace(4 * 2)
        assert lib.t2fit_binary_morph_dev(_abi.MORPH_CLOSE, inp.ptr, out.ptr, *shape, size.ctypes.data, runs.ctypes.data, len(runs),
                                          2, 0, _abi.MORPH_UNBOUNDED, ws.ptr, ws.nbytes, st) == _abi.OK
        stream.synchronize()
        assert np.array_equal(out.bytes().reshape(shape), M.close(a, fp, 2, unbounded=True))
        check(ws, inp, a)
        # hole filling
        a = _shells(shape)
        inp, out, ws = _Guarded(n, 9, a.astype(np.uint8)), _Guarded(n, 11), workspace(0)
        sweeps = C.c_int32(-1)
        assert lib.t2fit_fill_holes_dev(inp.ptr, out.ptr, *shape, -1, ws.ptr, ws.nbytes, C.byref(sweeps), st) == _abi.OK
        stream.synchronize()
        want = M.fill_holes(a)
        assert int(want.sum() - a.sum()) > 0 and np.array_equal(out.bytes().reshape(shape), want)
        assert sweeps.value == K.sweep_model(a)[1]
        check(ws, inp, a)
        # seed labels, both output types
        seeds = np.array([(10, 12, 9), (14, 12, 9), (0, 0, 0), (69, 32, 16), (66, 3, 5)], np.int32)
        labels = np.array([3, 250, 7, 1, 9], np.int32)
        ball, ball_size = M.footprint_runs(M.ball(3))
        ball_size = np.asarray(ball_size, np.int32)
        for out_type, dtype, offset in ((_abi.MORPH_U8, np.uint8, 13), (_abi.MORPH_I32, np.int32, 4)):
            out, ws = _Guarded(n * np.dtype(dtype).itemsize, offset), workspace(0)
            assert lib.t2fit_seed_labels_dev(seeds.ctypes.data, labels.ctypes.data, len(seeds), ball_size.ctypes.data, ball.ctypes.data,
                                             len(ball), *shape, out.ptr, out_type, ws.ptr, ws.nbytes, st) == _abi.OK
            stream.synchronize()
            assert np.array_equal(out.bytes().view(dtype).reshape(shape), M.seed_labels(shape, seeds, labels, M.ball(3), dtype))
            assert np.any(ws.bytes() != 0xA5)
    torch.cuda.synchronize()
