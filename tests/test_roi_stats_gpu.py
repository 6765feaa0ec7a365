"""In-vivo atlas ROI statistics on the device (t2fit_roi_erode_dev / t2fit_roi_stats_dev, t2map.roi_*, --roi_stats)
against the loops they replace (utils/ada_utils.py:130-216, :885-968), restated here with scipy.ndimage and numpy.
Boolean erosion and order statistics have no tolerance: erosion and medians are compared exactly."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def t2():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X")
    import fetal_t2mapping_amd as t2

    return t2


def _blocky(rng, shape, block, lo, hi):
    """Random integers in [lo, hi) constant on blocks of `block` voxels per axis, cropped to `shape`."""
    small = tuple(-(-s // b) for s, b in zip(shape, block))
    a = rng.integers(lo, hi, small)
    for ax, b in enumerate(block):
        a = a.repeat(b, ax)
    return np.ascontiguousarray(a[: shape[0], : shape[1], : shape[2]]).astype(np.int32)


def _scipy_erosion(mask, connectivity, iterations):
    from scipy.ndimage import binary_erosion, generate_binary_structure

    if iterations == 0:
        return mask
    return binary_erosion(mask, structure=generate_binary_structure(3, connectivity), iterations=iterations)


def _volume(rng):
    """(24, 40, 48): blocky labels 0..40 touching every face, a blocky tissue volume, a one-voxel-thick sheet, an
    isolated voxel, and label 37 absent."""
    shape = (24, 40, 48)
    lab = _blocky(rng, shape, (6, 8, 8), 0, 37)
    lab[2:20, 10:34, 20] = 38  # sheet, one voxel thick in x
    lab[12, 20, 40] = 39       # isolated voxel
    lab[8:16, 0:12, 0:10] = 40  # a big block on two faces
    lab[lab == 37] = 0
    tis = _blocky(rng, shape, (12, 20, 24), 1, 4)
    return lab, tis


@pytest.mark.parametrize("connectivity", [1, 2, 3])
@pytest.mark.parametrize("iterations", [0, 1, 2])
def test_erosion_equals_scipy_per_label(t2, connectivity, iterations):
    rng = np.random.default_rng(11)
    lab, tis = _volume(rng)
    n = 40
    for tissue, tv in ((tis, 2), (None, None)):
        roi = t2.roi_erode(lab, tissue, tv, labels=range(1, n + 1), connectivity=connectivity, iterations=iterations)
        assert roi.is_cuda and roi.dtype.is_floating_point is False and tuple(roi.shape) == lab.shape
        roi = roi.cpu().numpy()
        assert roi.dtype == np.int32 and roi.min() >= 0 and roi.max() <= n
        for L in range(1, n + 1):
            m = (lab == L) if tissue is None else ((tis == tv) & (lab == L))
            assert np.array_equal(roi == L, _scipy_erosion(m, connectivity, iterations)), (connectivity, iterations, L)
        assert not np.any(roi == 37)


@pytest.mark.parametrize("shape", [(7, 33, 65), (1, 5, 5), (9, 17, 130), (3, 3, 3)])
def test_erosion_on_sizes_off_the_tile_edges(t2, shape):
    rng = np.random.default_rng(12)
    lab = _blocky(rng, shape, (3, 5, 7), 0, 5)
    lab[...] = np.where(rng.random(shape) < 0.7, 1, lab)  # a large connected label so that something survives
    tis = _blocky(rng, shape, (4, 16, 32), 2, 4)
    for connectivity in (1, 3):
        for iterations in (1, 2):
            roi = t2.roi_erode(lab, tis, 3, connectivity=connectivity, iterations=iterations).cpu().numpy()
            for L in range(1, int(lab.max()) + 1):
                want = _scipy_erosion((tis == 3) & (lab == L), connectivity, iterations)
                assert np.array_equal(roi == L, want), (shape, connectivity, iterations, L)
            if shape[0] < 3:
                assert not roi.any()  # every voxel of a one-slice volume lies on a face


def test_erosion_with_sparse_label_ids_and_other_dtypes(t2):
    import torch

    rng = np.random.default_rng(13)
    lab, tis = _volume(rng)
    ids = [1003, 17, 2035, 4]  # FreeSurfer-like ids, in the caller's order
    sparse = np.zeros_like(lab, dtype=np.int64)
    for i, v in enumerate(ids):
        sparse[lab == i + 1] = v
    sparse[lab == 9] = 77  # an id nobody asked for
    want = t2.roi_erode(lab, tis, 2, labels=[1, 2, 3, 4]).cpu().numpy()
    got_np = t2.roi_erode(sparse, tis.astype(np.uint8), 2, labels=ids).cpu().numpy()
    got_t = t2.roi_erode(torch.from_numpy(sparse).cuda(), torch.from_numpy(tis.astype(np.int16)).cuda(), 2, labels=ids).cpu().numpy()
    assert np.array_equal(got_np, want) and np.array_equal(got_t, want) and want.any()
    with pytest.raises(ValueError):
        t2.roi_erode(lab, tis[:, :, :-1], 2)
    with pytest.raises(ValueError):
        t2.roi_erode(lab, tis)  # tissue without tissue_value
    with pytest.raises(ValueError):
        t2.roi_erode(lab, connectivity=4)


def _clustered_map(rng, shape):
    """float32 values with many exact ties (a grid of 0.25 ms), clusters sharing their top bytes, some negatives."""
    m = np.round(rng.normal(120.0, 25.0, shape) * 4.0) / 4.0
    m = np.where(rng.random(shape) < 0.05, -m, m)
    m = np.where(rng.random(shape) < 0.1, 100.0, m)
    return m.astype(np.float32)


def _check_stats(s, m, roi, n, nan=False):
    ulp = lambda v: np.spacing(np.abs(np.float32(v)))  # noqa: E731
    for i in range(n):
        sel = m[roi == i + 1]
        good = sel[~np.isnan(sel)]
        assert s.count[i] == len(sel) and s.valid[i] == len(good)
        if len(good) == 0:
            assert np.isnan(s.mean[i]) and np.isnan(s.std[i]) and np.isnan(s.median[i])
            continue
        assert np.float32(s.median[i]).tobytes() == np.float32(np.median(good)).tobytes(), (i, len(good))
        assert s.median[i] == np.median(good.astype(np.float64))  # exact in float64 as well
        g64 = good.astype(np.float64)
        assert abs(s.mean[i] - g64.mean()) <= 1e-12 * max(1.0, abs(g64.mean()))
        assert abs(s.std[i] - g64.std()) <= 1e-12 * max(1.0, g64.std())
        assert abs(s.mean[i] - np.mean(good)) <= 2 * ulp(np.mean(good))
        assert abs(s.std[i] - np.std(good)) <= 2 * ulp(max(np.std(good), 1e-30)) + 1e-6 * g64.std()
        if nan:
            assert np.float32(s.median[i]) == np.float32(np.nanmedian(sel))
            assert abs(s.mean[i] - np.nanmean(sel.astype(np.float64))) <= 1e-12 * abs(g64.mean()) + 1e-300


def test_stats_equal_numpy_on_eroded_regions(t2):
    rng = np.random.default_rng(21)
    lab, tis = _volume(rng)
    n = 40
    roi = t2.roi_erode(lab, None, None, labels=range(1, n + 1), connectivity=1)
    roi_h = roi.cpu().numpy()
    # regions of one voxel and of two voxels, an odd and an even count: planted into the ROI volume itself
    roi_h[roi_h == 38] = 0
    roi_h[0, 0, 0] = 38
    roi_h[roi_h == 39] = 0
    roi_h[23, 39, 46:48] = 39
    m = _clustered_map(rng, lab.shape)
    counts = np.bincount(roi_h.reshape(-1), minlength=n + 1)[1:]
    const = int(np.argmax(counts))
    m[roi_h == const + 1] = 87.5  # a constant region (the largest)
    assert (counts % 2 == 0).any() and (counts % 2 == 1).any() and counts[36] == 0 and counts[37] == 1 and counts[38] == 2
    s = t2.roi_stats(m, roi_h, n)
    _check_stats(s, m, roi_h, n)
    assert counts[const] > 100 and s.std[const] == 0.0 and s.mean[const] == 87.5 and s.median[const] == 87.5
    assert s.count[36] == 0 and np.isnan(s.mean[36]) and np.isnan(s.median[36])
    assert s.median[37] == float(m[0, 0, 0]) and s.median[38] == 0.5 * (float(m[23, 39, 46]) + float(m[23, 39, 47]))
    no_median = t2.roi_stats(m, roi_h, n, median=False)
    assert no_median.median is None and np.array_equal(no_median.mean, s.mean, equal_nan=True)
    with pytest.raises(ValueError):
        t2.roi_stats(m[:, :, :-1], roi_h, n)


def test_median_when_the_two_middle_values_part_in_every_byte(t2):
    """Even counts whose two middle values differ in the top byte (a negative and a positive half), in the second
    byte, and in the last one: the two ranks leave the shared histogram at different passes."""
    vals = [np.array([-3.0, -1.0, 2.0, 5.0], np.float32),
            np.array([1.0, 1.5, 300.0, 1000.0], np.float32),
            np.array([1.0, np.nextafter(np.float32(1.0), np.float32(2.0)), 0.5, 7.0], np.float32),
            np.array([-0.0, 0.0], np.float32),
            np.array([-2.5, -2.5, -7.0, -1.0, -2.25, -100.0], np.float32)]
    roi = np.zeros((1, 1, 64), np.int32)
    m = np.zeros((1, 1, 64), np.float32)
    at = 0
    for i, v in enumerate(vals):
        roi[0, 0, at:at + len(v)] = i + 1
        m[0, 0, at:at + len(v)] = v
        at += len(v) + 1
    s = t2.roi_stats(m, roi, len(vals))
    for i, v in enumerate(vals):
        assert s.median[i] == np.median(v.astype(np.float64)), (i, s.median[i])
        assert s.count[i] == len(v)


def test_nan_values_are_left_out_and_counted(t2):
    rng = np.random.default_rng(22)
    lab, _ = _volume(rng)
    n = 40
    m = _clustered_map(rng, lab.shape)
    for L in (3, 40):
        idx = np.flatnonzero(lab.reshape(-1) == L)
        m.reshape(-1)[idx[:: 5]] = np.nan
    m[lab == 7] = np.nan  # a region of NaNs only
    s = t2.roi_stats(m, lab, n)
    assert s.valid[2] < s.count[2] and s.valid[39] < s.count[39] and s.valid[6] == 0 and s.count[6] > 0
    assert np.array_equal(s.valid[[0, 1, 3]], s.count[[0, 1, 3]])
    _check_stats(s, m, lab, n, nan=True)


def test_results_are_a_function_of_the_data_alone(t2):
    import torch

    rng = np.random.default_rng(23)
    shape = (16, 64, 96)
    m = _clustered_map(rng, shape)
    lab256 = _blocky(rng, shape, (2, 4, 4), 0, 257)
    a = t2.roi_stats(m, lab256, 256)
    b = t2.roi_stats(m, lab256, 256)
    c = t2.roi_stats(torch.from_numpy(m).cuda(), torch.from_numpy(lab256).cuda(), 256)
    for f in ("mean", "std", "median", "count", "valid"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes() == getattr(c, f).tobytes(), f
    # 300 labels go through the library in two chunks: the first 256 rows are the one-call result on the same labels
    lab300 = lab256.copy()
    extra = _blocky(rng, shape, (2, 4, 4), 257, 301)
    lab300[:, :, 80:] = extra[:, :, 80:]
    d = t2.roi_stats(m, lab300, 300)
    e = t2.roi_stats(m, np.where(lab300 <= 256, lab300, 0).astype(np.int32), 256)
    for f in ("mean", "std", "median", "count", "valid"):
        assert getattr(d, f)[:256].tobytes() == getattr(e, f).tobytes(), f
    _check_stats(d, m, lab300, 300)
    # erosion through the chunked wrapper too
    wide = lab300.repeat(2, 0)  # blocks four voxels thick: something survives one pass
    for iterations in (0, 1):
        r300 = t2.roi_erode(wide, labels=range(1, 301), connectivity=1, iterations=iterations).cpu().numpy()
        for L in (1, 200, 256, 257, 300):
            assert np.array_equal(r300 == L, _scipy_erosion(wide == L, 1, iterations)), L
        assert r300.max() > 256
        again = t2.roi_erode(wide, labels=range(1, 301), connectivity=1, iterations=iterations).cpu().numpy()
        assert again.tobytes() == r300.tobytes()


def test_at_size_256x256x180_with_120_labels(t2):
    import torch

    shape = (180, 256, 256)
    g = torch.Generator(device="cuda").manual_seed(5)
    small = torch.randint(0, 121, (15, 16, 16), generator=g, device="cuda", dtype=torch.int32)
    lab = small.repeat_interleave(12, 0).repeat_interleave(16, 1).repeat_interleave(16, 2).contiguous()
    tis = torch.randint(2, 4, (3, 4, 4), generator=g, device="cuda", dtype=torch.int32)
    tis = tis.repeat_interleave(60, 0).repeat_interleave(64, 1).repeat_interleave(64, 2).contiguous()
    m = (torch.round(torch.randn(shape, generator=g, device="cuda") * 80.0) * 0.25 + 150.0).to(torch.float32)
    roi = t2.roi_erode(lab, tis, 3, labels=range(1, 121))
    s = t2.roi_stats(m, roi, 120)
    lab_h, tis_h, m_h, roi_h = lab.cpu().numpy(), tis.cpu().numpy(), m.cpu().numpy(), roi.cpu().numpy()
    assert s.count.sum() == np.count_nonzero(roi_h) and s.count.max() > 10000
    for L in (1, 17, 60, 61, 99, 120):
        want = _scipy_erosion((tis_h == 3) & (lab_h == L), 3, 1)
        assert np.array_equal(roi_h == L, want), L
        vals = m_h[want]
        assert s.count[L - 1] == vals.size
        assert np.float32(s.median[L - 1]).tobytes() == np.float32(np.median(vals)).tobytes(), L
        assert abs(s.mean[L - 1] - vals.astype(np.float64).mean()) <= 1e-12 * 150.0


def test_invalid_arguments_are_refused_before_any_device_work(t2):
    import torch

    from fetal_t2mapping_amd import _abi
    from fetal_t2mapping_amd._lib import load

    lib = load()
    lab = torch.ones((4, 4, 4), dtype=torch.int32, device="cuda")
    out = torch.full((4, 4, 4), -7, dtype=torch.int32, device="cuda")
    f = torch.ones(64, dtype=torch.float32, device="cuda")
    d = torch.full((3, 4), -7.0, dtype=torch.float64, device="cuda")
    c = torch.full((2, 4), -7, dtype=torch.int64, device="cuda")
    L, O, F = lab.data_ptr(), out.data_ptr(), f.data_ptr()

    def erode(label=L, tissue=None, nz=4, ny=4, nx=4, n=4, conn=3, it=1, roi=O):
        return lib.t2fit_roi_erode_dev(label, tissue, 0, nz, ny, nx, n, conn, it, roi, None)

    def stats(map_=F, roi=L, n_vox=64, n=4, mean=d[0].data_ptr(), std=d[1].data_ptr(), cnt=c[0].data_ptr()):
        return lib.t2fit_roi_stats_dev(map_, roi, n_vox, n, mean, std, d[2].data_ptr(), cnt, c[1].data_ptr(), None)

    bad = [erode(label=None), erode(roi=None), erode(nz=0), erode(ny=-1), erode(nx=0), erode(n=0), erode(n=257),
           erode(conn=0), erode(conn=4), erode(it=-1), erode(it=9), erode(nz=65536, ny=65536, nx=1),
           erode(nz=2048, ny=2048, nx=2048), erode(roi=L),
           stats(map_=None), stats(roi=None), stats(mean=None), stats(std=None), stats(cnt=None), stats(n_vox=0),
           stats(n_vox=-5), stats(n_vox=2**32), stats(n=0), stats(n=257)]
    assert bad == [_abi.E_INVALID] * len(bad)
    assert erode(n=0) == _abi.E_INVALID and b"n_labels" in lib.t2fit_last_error()
    assert stats(n_vox=2**32) == _abi.E_INVALID and b"2^32" in lib.t2fit_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((d == -7.0).all()) and bool((c == -7).all())  # nothing was launched
    assert erode() == _abi.OK and stats() == _abi.OK
    torch.cuda.synchronize()
    assert int(out[1:3, 1:3, 1:3].sum()) == 8 and int(out.sum()) == 8 and int(c[0, 0]) == 64 and float(d[2, 0]) == 1.0


def _roi_tree(tmp_path, with_labels=("ho", "jhu", "feta")):
    """A tiny BIDS tree: three echoes of a synthetic brain volume, masks, and the ho / jhu / feta label images."""
    import pandas as pd

    from fetal_t2mapping_amd import cli as R
    from fetal_t2mapping_amd import nifti, synth

    shape = (10, 24, 32)
    echoes, mask, te = synth.brain_volume(shape, 3, seed=synth.SEED_BASE, low_field=True)
    rng = np.random.default_rng(31)
    feta = _blocky(rng, shape, (5, 12, 16), 2, 4)
    vols = {"ho": _blocky(rng, shape, (5, 6, 8), 0, 7), "jhu": _blocky(rng, shape, (5, 8, 8), 0, 5), "feta": feta}
    root = str(tmp_path)
    bids = os.path.join(root, "projects") + "/"
    os.makedirs(os.path.join(bids, "prj-902"))
    os.makedirs(os.path.join(root, "dicom", "logs"))
    rows = []
    for i, t in enumerate(te):
        acq = {"prj": "prj-902", "sub": "sub-003", "ses": "ses-01", "run": f"run-{i + 1:02d}", "EchoTime": t / 1000.0,
               "CoilString": "HeadNeck"}
        rows.append(acq)
        for arr, dirname in ((echoes[i], R.recon_dirname), (mask, R.mask_dirname)):
            nifti.WriteImage(nifti.GetImageFromArray(arr), R.get_img_path(bids, acq, dirname).replace(" ", ""))
    # atlas images carry the last echo's name (as the phantom's label image), the FeTA image the first echo's
    # (utils/ada_utils.py:908): both are found
    for name in with_labels:
        acq = rows[0] if name == "feta" else rows[-1]
        arr = vols[name].astype(np.float32) if name == "jhu" else vols[name].astype(np.int16)  # FSL writes float atlases
        nifti.WriteImage(nifti.GetImageFromArray(arr), R.get_img_path(bids, acq, "recon_1mm_" + name).replace(" ", ""))
    pd.DataFrame(rows).to_csv(os.path.join(root, "dicom", "logs", "log.csv"), index=False)
    out_dir = os.path.join(bids, "prj-902", "derivatives", R.t2map_dirname, "sub-003", "ses-01", "anat")
    return root, out_dir, vols, [str(int(t)) for t in te]


def _reference_rows(maps, atlas, feta, tissue):
    """get_t2_per_roi (utils/ada_utils.py:160-189) restated: one dict per label 1..atlas.max()."""
    rows = []
    for L in range(1, int(atlas.max()) + 1):
        sel = (atlas == L) if tissue is None else ((feta == tissue) & (atlas == L))
        sel = _scipy_erosion(sel, 3, 1)
        row = {"index": L, "nvoxel": int(sel.sum())}
        for name, m in maps.items():
            v = m[sel]
            with np.errstate(all="ignore"):
                import warnings

                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    row.update({f"mean_{name}": np.mean(v), f"std_{name}": np.std(v), f"median_{name}": np.median(v)})
        rows.append(row)
    return rows


def test_cli_writes_the_roi_tables(t2, tmp_path, monkeypatch, capsys):
    import sys

    import pandas as pd

    from fetal_t2mapping_amd import cli as R
    from fetal_t2mapping_amd import nifti

    monkeypatch.setitem(sys.modules, "SimpleITK", None)
    base = ["--csv", "log.csv", "--in_vivo", "--gaussian", "--lf", "--sim", "r1"]
    stem = "sub-003_ses-01_recon_1mm_sim-r1_"
    map_files = sorted(stem + f"{m}map_ada-gaussian.nii.gz" for m in ("t2", "k", "sigma", "res"))

    # without the flags: the maps, nothing else
    root0, out0, _, tes = _roi_tree(tmp_path / "plain")
    base += ["--TEs"] + tes
    R.main(["--path", root0] + base)
    assert sorted(os.listdir(out0)) == map_files

    root, out_dir, vols, _ = _roi_tree(tmp_path / "roi")
    R.main(["--path", root] + base + ["--roi_stats", "ho:2", "--roi_stats", "jhu:3", "--roi_stats", "feta"])
    csvs = {name: stem + f"ROI_{name}_ada-gaussian.csv" for name in ("ho", "jhu", "feta")}
    assert sorted(os.listdir(out_dir)) == sorted(map_files + list(csvs.values()))
    maps = {m: nifti.ReadImage(os.path.join(out_dir, stem + f"{m}map_ada-gaussian.nii.gz")).arr for m in ("t2", "k", "sigma")}
    for m in ("t2", "k", "sigma", "res"):  # the maps do not depend on the flags
        a = nifti.ReadImage(os.path.join(out0, stem + f"{m}map_ada-gaussian.nii.gz")).arr
        assert np.array_equal(a, nifti.ReadImage(os.path.join(out_dir, stem + f"{m}map_ada-gaussian.nii.gz")).arr, equal_nan=True)
    some = 0
    for name, tissue in (("ho", 2), ("jhu", 3), ("feta", None)):
        got = pd.read_csv(os.path.join(out_dir, csvs[name]))
        want = _reference_rows(maps, vols[name], vols["feta"], tissue)
        assert list(got.columns) == ["roi", "index", "nvoxel", "nvalid"] + [f"{s}_{m}" for m in ("t2", "k", "sigma")
                                                                               for s in ("mean", "std", "median")]
        assert len(got) == len(want)
        for i, row in enumerate(want):
            assert got["index"][i] == row["index"] and got["nvoxel"][i] == row["nvoxel"] and str(got["roi"][i]) == str(row["index"])
            some += row["nvoxel"] > 0
            for key, v in row.items():
                if key in ("index", "nvoxel"):
                    continue
                if np.isnan(v):
                    assert np.isnan(got[key][i]), (name, key, i)
                elif key.startswith("median"):
                    assert np.float32(got[key][i]) == np.float32(v), (name, key, i)
                else:
                    assert np.isclose(got[key][i], v, rtol=1e-5, atol=1e-6), (name, key, i)
    assert some >= 6

    # one label image missing: a warning, the other tables, no error
    root2, out2, _, _ = _roi_tree(tmp_path / "gap", with_labels=("ho", "feta"))
    capsys.readouterr()
    R.main(["--path", root2] + base + ["--roi_stats", "ho:2", "--roi_stats", "jhu:3", "--roi_stats", "feta",
                                        "--roi_connectivity", "1", "--roi_erosion", "2"])
    text = capsys.readouterr().out
    assert "Warning" in text and "recon_1mm_jhu" in text
    assert sorted(os.listdir(out2)) == sorted(map_files + [csvs["ho"], csvs["feta"]])
