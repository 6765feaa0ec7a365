"""Host side of the in-vivo ROI statistics (no device): the table assembly of t2map.roi_table, the dense remapping of
sparse label ids, the --roi_stats flags and file naming of the CLI, and the ABI of the built library (version 5, the
two entry points, the argument checks that return before any HIP call).  tests/test_roi_stats_gpu.py runs the
kernels."""
import ctypes as C
import os

import numpy as np
import pytest


def test_roi_frame_columns_rounding_and_names():
    from fetal_t2mapping_amd import t2map

    mean = np.array([101.123456789, np.nan, -3.3])
    std = np.array([0.1, np.nan, 0.0])
    med = np.array([100.0000001, np.nan, 16777217.0])
    stats = {"t2": (mean, std, med), "k": (mean * 2, std * 2, med * 2)}
    f = t2map.roi_frame([4, 17, 1003], ["Frontal Pole", "Insular Cortex", "ctx-lh"], [10, 0, 3], [9, 0, 3], stats)
    assert list(f.columns) == ["roi", "index", "nvoxel", "nvalid", "mean_t2", "std_t2", "median_t2", "mean_k", "std_k", "median_k"]
    assert list(f["roi"]) == ["Frontal Pole", "Insular Cortex", "ctx-lh"] and list(f["index"]) == [4, 17, 1003]
    assert list(f["nvoxel"]) == [10, 0, 3] and list(f["nvalid"]) == [9, 0, 3] and f["nvoxel"].dtype == np.int64
    # rounded to the float32 numpy returns on a float32 map, stored as float64 (as phantom_frame does)
    for col, src in (("mean_t2", mean), ("median_t2", med), ("std_k", std * 2)):
        assert f[col].dtype == np.float64
        assert np.array_equal(f[col].to_numpy(), src.astype(np.float32).astype(np.float64), equal_nan=True)
    assert f["median_t2"][2] == 16777216.0 and f["mean_t2"][0] != mean[0]
    assert f.to_csv(index=False).splitlines()[1].startswith("Frontal Pole,4,10,9," + repr(float(np.float32(mean[0]))))
    # without names the ids stand in
    g = t2map.roi_frame([2, 3], None, [1, 1], [1, 1], {"t2": ([1.0, 2.0], [0.0, 0.0], [1.0, 2.0])})
    assert list(g["roi"]) == ["2", "3"]
    with pytest.raises(ValueError):
        t2map.roi_frame([2, 3], ["gm"], [1, 1], [1, 1], {})


def test_roi_table_runs_erosion_once_and_statistics_per_map(monkeypatch):
    """roi_table through its two seams (roi_erode, roi_stats), as phantom_frame is tested: what it asks for and how it
    assembles the answers."""
    import torch

    from fetal_t2mapping_amd import _gpu_roi, t2map

    calls = {"erode": [], "stats": []}
    label = np.zeros((2, 3, 4), np.int16)
    label[0] = 12
    label[1, 0] = 47

    def fake_erode(lab, tissue, tissue_value, *, labels, connectivity, iterations, device):
        calls["erode"].append((tissue_value, list(labels), connectivity, iterations))
        return t2map.dense_labels(torch.from_numpy(np.asarray(lab).astype(np.int64)), labels)

    def fake_stats(m, roi, n_labels, *, median=True, device=0):
        calls["stats"].append(n_labels)
        r = roi.numpy()
        cnt = np.array([np.sum(r == i + 1) for i in range(n_labels)], np.int64)
        mean = np.array([np.mean(np.asarray(m)[r == i + 1]) if cnt[i] else np.nan for i in range(n_labels)])
        return t2map.RoiStats(mean, mean * 0, mean, cnt, cnt)

    monkeypatch.setattr(_gpu_roi, "roi_erode", fake_erode)
    monkeypatch.setattr(_gpu_roi, "roi_stats", fake_stats)
    maps = {"t2": np.full(label.shape, 80.1, np.float32), "sigma": np.full(label.shape, 3.0, np.float32)}
    f = t2map.roi_table(maps, label, label, 12, labels=[47, 12, 5], names=["a", "b", "c"], connectivity=2, iterations=3)
    assert calls == {"erode": [(12, [47, 12, 5], 2, 3)], "stats": [3, 3]}
    assert list(f["roi"]) == ["a", "b", "c"] and list(f["index"]) == [47, 12, 5] and list(f["nvoxel"]) == [4, 12, 0]
    assert f["mean_t2"][0] == float(np.float32(80.1)) and np.isnan(f["mean_sigma"][2]) and f["median_sigma"][1] == 3.0
    with pytest.raises(ValueError):
        t2map.roi_table({"t2": maps["t2"][:, :, :-1]}, label, labels=[47])
    with pytest.raises(ValueError):
        t2map.roi_table({}, label, labels=[47])


def test_dense_labels_remaps_sparse_ids_on_cpu_tensors():
    import torch

    from fetal_t2mapping_amd import _gpu, t2map

    lab = torch.tensor([[[0, 1003, 17, 17], [2035, 4, 99, -1]]], dtype=torch.int64)
    out = t2map.dense_labels(lab, [1003, 17, 2035, 4])
    assert out.dtype == torch.int32 and out.shape == lab.shape
    assert out.tolist() == [[[0, 1, 2, 2], [3, 4, 0, 0]]]
    assert t2map.dense_labels(lab.to(torch.int16), [17]).tolist() == [[[0, 0, 1, 1], [0, 0, 0, 0]]]
    assert t2map.dense_labels(lab, range(1, 5)).tolist() == [[[0, 0, 0, 0], [0, 4, 0, 0]]]
    big = torch.arange(0, 1000, dtype=torch.int32).reshape(10, 10, 10)
    ids = [999, 0, 500] + list(range(1, 400))
    d = t2map.dense_labels(big, ids)
    want = np.zeros(1000, np.int32)
    for i, v in enumerate(ids):
        want[v] = i + 1
    assert np.array_equal(d.numpy().reshape(-1), want)
    with pytest.raises(ValueError):
        t2map.dense_labels(lab, [])
    with pytest.raises(ValueError):
        t2map.dense_labels(lab, [4, 17, 4])
    with pytest.raises(ValueError):
        _gpu.int_labels(np.zeros((2, 2, 2), np.float32))


def test_cli_roi_flags_and_csv_path(tmp_path):
    from fetal_t2mapping_amd import cli as R

    base = ["--path", "x", "--csv", "a.csv", "--in_vivo", "--gaussian", "--lf", "--sim", "7"]
    args = R.parse_arguments(base)
    assert args.roi_stats == [] and args.roi_specs == [] and args.roi_connectivity == 3 and args.roi_erosion == 1
    args = R.parse_arguments(base + ["--roi_stats", "ho:2", "--roi_stats", "jhu:3", "--roi_stats", "feta", "--roi_connectivity",
                                     "1", "--roi_erosion", "2"])
    assert args.roi_specs == [("ho", 2), ("jhu", 3), ("feta", None)] and args.roi_connectivity == 1 and args.roi_erosion == 2
    assert R.parse_roi_spec("aparc-aseg:42") == ("aparc-aseg", 42)
    for bad in ("", ":2", "ho:gm", "../x", "a/b:1"):
        with pytest.raises(ValueError):
            R.parse_roi_spec(bad)
    for argv in (["--roi_stats", "ho:gm"], ["--roi_connectivity", "4"], ["--roi_erosion", "9"], ["--roi_erosion", "-1"]):
        with pytest.raises(SystemExit):
            R.parse_arguments(base + argv)
    bids = str(tmp_path / "projects") + "/"
    acq = {"prj": "prj-004", "sub": "sub-002", "ses": "ses-01", "run": "run-03", "EchoTime": 0.299, "CoilString": "HeadNeck"}
    path = R.roi_csv_path(bids, acq, R.t2map_dirname, "7", "gaussian", "ho")
    assert os.path.relpath(path, bids) == ("prj-004/derivatives/recon_1mm_t2map/sub-002/ses-01/anat/"
                                           "sub-002_ses-01_recon_1mm_sim-7_ROI_ho_ada-gaussian.csv")
    # the phantom table's rule, with ROI_<name> where it has ROI_data
    phantom = R.get_img_path(bids, acq, R.t2map_dirname).replace("t2map.nii.gz", "sim-7_ROI_data_ada-gaussian.csv")
    assert path == phantom.replace("ROI_data", "ROI_ho")
    assert R.feta_dirname == "recon_1mm_feta"


def test_cli_roi_tables_skip_missing_label_images(tmp_path, monkeypatch, capsys):
    """save_roi_csvs on the host: label images are found under the last echo's name or another echo's, float atlases are
    rounded, a missing or misshapen image costs its table and a warning only.  (roi_table is replaced: no device.)"""
    import sys

    import pandas as pd

    from fetal_t2mapping_amd import cli as R
    from fetal_t2mapping_amd import nifti

    monkeypatch.setitem(sys.modules, "SimpleITK", None)
    seen = []

    def fake_table(maps, label, tissue=None, tissue_value=None, *, connectivity=3, iterations=1, device=0, **kw):
        seen.append((sorted(maps), label.dtype, int(label.max()), None if tissue is None else int(tissue.max()), tissue_value,
                     connectivity, iterations))
        return pd.DataFrame({"roi": ["1"], "index": [1]})

    monkeypatch.setattr(R.t2map, "roi_table", fake_table)
    bids = str(tmp_path / "projects") + "/"
    shape = (3, 4, 5)
    acqs = [{"prj": "prj-9", "sub": "sub-001", "ses": "ses-01", "run": f"run-{i}", "EchoTime": te, "CoilString": "HeadNeck"}
            for i, te in enumerate((0.114, 0.202, 0.299))]

    def put(name, acq, arr):
        nifti.WriteImage(nifti.GetImageFromArray(arr), R.get_img_path(bids, acq, "recon_1mm_" + name).replace(" ", ""))

    put("ho", acqs[-1], np.full(shape, 6.0, np.float32))   # a float atlas under the last echo's name
    put("feta", acqs[0], np.full(shape, 3, np.int16))       # the FeTA image under the first echo's
    put("odd", acqs[-1], np.ones((3, 4, 6), np.int16))      # wrong shape
    maps = [np.zeros(shape, np.float32)] * 3
    written = R.save_roi_csvs(*maps, [("ho", 3), ("jhu", 3), ("odd", None), ("feta", None)], 2, 1, bids, acqs, R.t2map_dirname,
                              "s", "rician")
    out = capsys.readouterr().out
    assert [os.path.basename(p) for p in written] == ["sub-001_ses-01_recon_1mm_sim-s_ROI_ho_ada-rician.csv",
                                                      "sub-001_ses-01_recon_1mm_sim-s_ROI_feta_ada-rician.csv"]
    assert all(os.path.exists(p) for p in written)
    assert seen == [(["k", "sigma", "t2"], np.dtype(np.int32), 6, 3, 3, 2, 1), (["k", "sigma", "t2"], np.dtype(np.int32), 3, None, None, 2, 1)]
    assert out.count("Warning") == 2 and "recon_1mm_jhu" in out and "'odd'" in out


def test_built_library_has_abi_5_and_refuses_bad_arguments_without_a_device():
    """The two entry points are in the built library and in the ctypes table, T2FIT_ABI_VERSION is 5 on both sides, and
    every argument check returns E_INVALID with a message before HIP is touched (this machine has no GPU)."""
    from fetal_t2mapping_amd import _abi, build

    assert _abi.ABI_VERSION == 5
    names = [s[0] for s in _abi.SYMBOLS]
    assert "t2fit_roi_erode_dev" in names and "t2fit_roi_stats_dev" in names
    header = open(os.path.join(os.path.dirname(build.PKG), "include", "t2fit.h")).read()
    assert "#define T2FIT_ABI_VERSION 5" in header and "t2fit_roi_erode_dev(" in header and "t2fit_roi_stats_dev(" in header
    assert any(src.endswith("t2fit_roi.hip") for src in build.SOURCES)
    import torch  # noqa: F401  (one HIP runtime per process: see _lib.load)

    lib = _abi.bind(C.CDLL(build.build()))
    assert lib.t2fit_abi_version() == 5
    p = 4096  # never dereferenced: every call below is refused first

    def erode(label=p, nz=4, ny=4, nx=4, n=4, conn=3, it=1, roi=2 * p):
        return lib.t2fit_roi_erode_dev(label, None, 0, nz, ny, nx, n, conn, it, roi, None)

    def stats(map_=p, roi=p, n_vox=64, n=4, mean=p, std=p, cnt=p):
        return lib.t2fit_roi_stats_dev(map_, roi, n_vox, n, mean, std, None, cnt, None, None)

    cases = {"NULL": [erode(label=None), erode(roi=None), stats(map_=None), stats(roi=None), stats(mean=None), stats(std=None),
                      stats(cnt=None)],
             "positive": [erode(nz=0), erode(ny=0), erode(nx=-3), stats(n_vox=0), stats(n_vox=-1)],
             "n_labels": [erode(n=0), erode(n=257), stats(n=0), stats(n=257)],
             "connectivity": [erode(conn=0), erode(conn=4)],
             "iterations": [erode(it=-1), erode(it=9)],
             "2^32": [erode(nz=1 << 16, ny=1 << 16, nx=1), erode(nz=1 << 11, ny=1 << 11, nx=1 << 11), stats(n_vox=1 << 32)],
             "must not be an input": [erode(roi=p)]}
    for word, rcs in cases.items():
        assert rcs == [_abi.E_INVALID] * len(rcs), word
    for word, call in (("NULL", lambda: erode(label=None)), ("positive", lambda: erode(nz=0)), ("n_labels", lambda: stats(n=257)),
                       ("connectivity", lambda: erode(conn=4)), ("iterations", lambda: erode(it=9)),
                       ("2^32", lambda: stats(n_vox=1 << 32)), ("must not be an input", lambda: erode(roi=p))):
        assert call() == _abi.E_INVALID and word in lib.t2fit_last_error().decode(), word
