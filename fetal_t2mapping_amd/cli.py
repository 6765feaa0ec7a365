"""CLI and volume driver: the reference's ``run_t2mapping.py`` surface on the MI355X fit.

    python -m fetal_t2mapping_amd.cli --path /data/qMRI --csv 2024083017_17510000.csv \
        --in_vivo --gaussian --lf --sim 1 [--TEs 114 202 299] [--no_prior] [--solver lbfgsb|lm|loglin|dict|nnls] [--gpus N]
        [--roi_stats ho:2 --roi_stats jhu:3 --roi_stats feta] [--roi_connectivity 3] [--roi_erosion 1]
        [--bootstrap 100 [--bootstrap_seed 0] [--bootstrap_alpha 0.05] [--bootstrap_noise background|sigma_map|mppca|<float>]]
        [--denoise tv|tv_joint [--denoise_weight 0.1|<c>sigma] [--denoise_dims 2|3] [--denoise_eps 2e-4] [--denoise_iter 200]
                               [--denoise_sigma background|mppca]]
        [--denoise mppca [--denoise_patch 2] [--denoise_dims 2|3]] [--write_noise_map]

--gpus N (N > 1) starts one process per GPU (torch.distributed.run, RCCL) before anything touches a GPU: with at
least N subjects in the CSVs each rank streams its own subjects (dist.subjects_of_rank: nothing is exchanged,
BASELINE.json config 5); with fewer, every volume is shared: each rank decodes 1/N of its echo files, one all-to-all
hands every rank all echoes of its balanced share of the voxels, the maps (and the per-voxel status) are all-gathered
(dist.exchange_echo_shares / gather_maps_cyclic, config 4); rank 0 writes the files of a shared volume.

Same flags, metadata CSVs, input/output file names and maps as the reference
(run_t2mapping.py:483-576, utils/metadata_utils.py, utils/qmri_utils.py:13-33,
utils/t2map_utils.py:18-59); the voxel loop (:411-461) is one call into the HIP library.  NIfTI I/O
stays SimpleITK on the host, as in the reference (nifti.py stands in where SimpleITK is not installed).
--roi_stats NAME[:TISSUE] (repeatable) adds, after the maps, the per-region table of the atlas image recon_1mm_<NAME>
(mean / std / median of t2, k, sigma over the eroded regions, inside FeTA tissue TISSUE when given): the loops of
utils/ada_utils.py:130-216 and :885-968 on the GPU (t2map.roi_table).
--bootstrap R adds, after the maps, R replicas of the parametric bootstrap (t2map.bootstrap_volume): the T2 standard
deviation, bias, percentile interval and replica count of every voxel as ..._T2stdmap / T2biasmap / T2cilomap /
T2cihimap / T2nokmap_ada-<fit>.nii.gz beside the four maps.
--denoise tv passes the decoded echo volumes through t2map.denoise_tv (TV-Chambolle as scikit-image defines it: the
reference's run_denoising, utils/qmri_utils.py:393-405, the last step of its reconstruction stage) before the union mask
and the fit; masks, geometry and output file names are unchanged.
--denoise tv_joint is vector-valued TV across the echoes (t2map.denoise_tv(joint=True)): one gradient norm per voxel,
sqrt(sum over echoes |grad u|^2), so all echoes share one edge set.  The weight is not rescaled by the echo count: the
joint norm of pure noise is about sqrt(nTE) times one echo's, so a weight that suits tv is about sqrt(nTE) too small.
--denoise mppca is Marchenko-Pastur PCA across the echoes (t2map.denoise_mppca; Veraart et al. 2016, MRtrix's dwidenoise):
no weight to tune; --denoise_patch R is the radius of its (2R+1)^dims window.  --write_noise_map writes the noise level and
the number of signal components it measures in tissue, on the echoes as they were read, as ..._mppcasigmamap / mppcarankmap
beside the four maps.  --bootstrap_noise mppca replicates from that per-voxel sigma map; --denoise_sigma mppca takes the
sigma of a <c>sigma TV weight from its median inside the mask instead of from the background.  The noise is treated as
Gaussian: at low SNR the Rician floor biases sigma low.
The convergence-study figures (:465-468) are written on request (--plots, convergence.py).  ``--csv prj-004``
(prj-003, prj-002) stands for the session logs of that project of the reference's paper, as in
utils/metadata_utils.py:19-85.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

from . import t2map

# derivative directory names (utils/metadata_utils.py:4-17)
recon_dirname = "recon_1mm"
mask_dirname = "recon_1mm_mask"
phantom_labels_dirname = "recon_1mm_label"
t2map_dirname = recon_dirname + "_t2map"
feta_dirname = recon_dirname + "_feta"  # FeTA tissue segmentation (utils/ada_utils.py:908): 2 = grey, 3 = white matter


def _sitk():
    """NIfTI I/O: SimpleITK as in the reference when it is importable, else the package's own NIfTI-1
    reader/writer (same five calls, same (Z,Y,X) arrays and LPS geometry; fetal_t2mapping_amd/nifti.py)."""
    try:
        import SimpleITK as sitk
    except ImportError:
        from . import nifti as sitk
    return sitk


_pinned = {}


def _pinned_stack(recon_paths):
    """Page-locked float32 staging block for one subject's echoes (kept for the next subject of the same size):
    the decoder writes into it and the host->device copy is a DMA from where the samples lie.  None when torch
    or a GPU is not there (the fit would fail loudly later anyway)."""
    try:
        import torch

        from . import nifti

        if not torch.cuda.is_available():
            return None
        with open(recon_paths[0], "rb") as f:
            head = f.read(4096)
        if head[:2] == b"\x1f\x8b":
            import zlib

            head = zlib.decompressobj(wbits=31).decompress(head, 352)
        n = len(recon_paths) * int(np.prod(nifti._parse_header(head).shape))
        if _pinned.get("n") != n:
            _pinned.clear()
            _pinned.update(n=n, buf=torch.empty(n, dtype=torch.float32).pin_memory())
        return _pinned["buf"].numpy()
    except Exception:
        return None


DECODED = {"echo": 0, "mask": 0}  # volume files this process has decoded (the shared-volume tests assert 1/G of them)


def _read_geometry(sitk, path):
    """Spacing / origin / direction of the image at `path` (an object with the three Get* methods) without decoding the
    voxels where the reader can: the maps carry the geometry of the LAST echo's image (run_t2mapping.py:377 /
    utils/t2map_utils.py:22-24), which the rank that writes them may not have decoded."""
    from . import nifti

    if sitk is nifti:
        return nifti.ReadGeometry(path)
    if hasattr(sitk, "ImageFileReader"):  # SimpleITK: header only
        r = sitk.ImageFileReader()
        r.SetFileName(path)
        r.ReadImageInformation()
        return nifti.Image(np.zeros((0, 0, 0), np.float32), r.GetSpacing(), r.GetOrigin(), r.GetDirection())
    return sitk.ReadImage(path)


def _read_subject(sitk, recon_paths, mask_paths, label_path):
    """All volumes of one (sub, ses): echoes, masks, optional vial labels, and the last recon image (its
    geometry goes onto the maps, run_t2mapping.py:377 / utils/t2map_utils.py:22-24).  With the native
    reader the files are decoded concurrently, the echoes straight into one float32 (nTE,Z,Y,X) block."""
    from . import nifti

    DECODED["echo"] += len(recon_paths)
    DECODED["mask"] += len(mask_paths)
    if not recon_paths:  # a rank of a shared volume with more ranks than echoes
        label = sitk.GetArrayFromImage(sitk.ReadImage(label_path)) if label_path else None
        return [], [], label, None

    if sitk is nifti:
        from concurrent.futures import ThreadPoolExecutor

        with ThreadPoolExecutor(8) as pool:
            masks_f = pool.map(nifti.ReadImage, mask_paths)
            label_f = pool.submit(nifti.ReadImage, label_path) if label_path else None
            stack, images = nifti.read_stack(recon_paths, out=_pinned_stack(recon_paths))
            masks = [m.arr for m in masks_f]
            label = label_f.result().arr if label_f else None
        return list(stack), masks, label, images[-1]
    vols, masks, recon_img = [], [], None
    for rp, mp in zip(recon_paths, mask_paths):
        recon_img = sitk.ReadImage(rp)
        masks.append(sitk.GetArrayFromImage(sitk.ReadImage(mp)))
        vols.append(sitk.GetArrayFromImage(recon_img))
    label = sitk.GetArrayFromImage(sitk.ReadImage(label_path)) if label_path else None
    return vols, masks, label, recon_img


def _read_masks(sitk, mask_paths, label_path):
    """The masks and the optional vial labels of one (sub, ses) when the echoes do not come from files (--reconstruct):
    ``([], masks, label, None)``, the shape of _read_subject's result."""
    DECODED["mask"] += len(mask_paths)
    masks = [sitk.GetArrayFromImage(sitk.ReadImage(mp)) for mp in mask_paths]
    label = sitk.GetArrayFromImage(sitk.ReadImage(label_path)) if label_path else None
    return [], masks, label, None


def _read_echoes(sitk, recon_paths):
    """The echo volumes of one (sub, ses) alone (--build_mask: no mask or label file is read): ``(vols, last image)``."""
    DECODED["echo"] += len(recon_paths)
    vols, recon_img = [], None
    for rp in recon_paths:
        recon_img = sitk.ReadImage(rp)
        vols.append(sitk.GetArrayFromImage(recon_img))
    return vols, recon_img


# ---- phantom masks and labels built on the device (--build_mask phantom) -------------------------
def load_seeds(path):
    """``--phantom_seeds FILE``: a JSON list of ``[x, y, z]`` voxel indices, one per vial in label order (the `seeds`
    list of the reference's run_qmri_reconstruction.py)."""
    import json

    with open(path) as f:
        seeds = json.load(f)
    if (not isinstance(seeds, list) or not seeds
            or not all(isinstance(s, list) and len(s) == 3 and all(isinstance(v, int) for v in s) for s in seeds)):
        raise ValueError(f"{path}: expected a JSON list of [x, y, z] integer triples")
    if len(seeds) > 255:
        raise ValueError(f"{path}: at most 255 seeds fit the uint8 label image")
    return seeds


def build_phantom_subject(vols, seeds, threshold=100, close_radius=15, dilate_radius=10, label_radius=6, device=0):
    """The masks of every echo volume (build_phantom_masks, utils/qmri_utils.py:591-623) and the vial labels
    (build_phantom_labels_v2, :868-933) of one (sub, ses) on the device: ``(masks: list of uint8 arrays, label: uint8
    array)``, what the recon_1mm_mask / recon_1mm_label files would hold."""
    masks = [t2map.phantom_mask(np.asarray(v, np.float32), threshold, close_radius, dilate_radius, device=device) for v in vols]
    label = t2map.phantom_labels(np.asarray(vols[0]).shape, seeds, label_radius, device=device)
    return [m.cpu().numpy() for m in masks], label.cpu().numpy()


# ---- metadata / paths --------------------------------------------------------------------------
def mk_bids_dir(bids_dir, *dirs):
    """utils/dcm_utils.py:189-195 (there: `if not exists: mkdir`; with --gpus N several ranks create the shared
    parents of their subjects' directories at the same moment, so an existing directory is not an error here)."""
    path = bids_dir
    for d in dirs:
        path = os.path.join(path, d)
        os.makedirs(path, exist_ok=True)


def get_img_path(bids_path, acq, type: str = "anat"):
    """File naming of utils/qmri_utils.py:13-33: raw images under <prj>/<sub>/<ses>/anat, everything
    else under <prj>/derivatives/<type>/<sub>/<ses>/anat; recon-type names carry the echo time (width 3)."""
    sub, ses = acq["sub"], acq["ses"]
    derived = [acq["prj"], "derivatives", type, sub, ses, "anat"]
    if type == "anat":
        dirs, stem = [acq["prj"], sub, ses, "anat"], [sub, ses, acq["run"] + "_T2w.nii.gz"]
    elif "t2map" in type:
        dirs, stem = derived, [sub, ses, type + ".nii.gz"]
    elif "recon" in type:
        simulated = acq["CoilString"] == "Simulation"
        te_field = f"te-{int(acq['EchoTime'] if simulated else acq['EchoTime'] * 1000):3}"
        dirs, stem = derived, [sub, ses] + ([f"t2-{int(acq['T2']):3}"] if simulated else []) + [te_field, type + ".nii.gz"]
    else:
        dirs, stem = derived, [sub, ses, acq["run"], "T2w", type + ".nii.gz"]
    mk_bids_dir(bids_path, *dirs)
    return os.path.join(bids_path, *dirs, "_".join(stem))


# `--csv prj-00X` instead of file names: the session logs of the three projects of the reference's paper
# (utils/metadata_utils.py:19-85), keyed by (project, low_field).  Data, not logic: the file names as the reference lists them
# (entries it has commented out are left out here too).  None: the reference has no such data and exits.
_PROJECT_LOGS = {
    ("prj-004", True): "2024083017_17510000 2024090320_55420000 2024090618_37050000 2024090811_14320000 2024091017_53530000_1 "
                       "2024091017_53530000_2 2024091020_45220000 2024091320_23400000 2024091321_22550000 2024091322_27490000 "
                       "2024092720_10110000 2024092719_10310000 2024102120_48480000",
    ("prj-004", False): "2024083019_26300000 2024090322_28560000 2024090619_26370000 2024090812_21470000 2024091021_57280000 "
                        "2024091319_13240000 2024091318_13560000 2024092721_25410000 2024102616_18560000 2024102122_28450000",
    ("prj-003", True): "20240806_30540000_1",
    ("prj-003", False): None,
    ("prj-002", True): "20240527_095111_2",
    ("prj-002", False): "20240609_50140000_2",
}
_PROJECT_BANNERS = {
    "prj-004": ["PRJ-004 - In vivo adult brain data acquired using the head coil"],
    "prj-003": ["PRJ-003 - In vitro NIST Phantom data acquired using the abdominal coil M",
                "Notes: only data selected for paper submission are processed."],
    "prj-002": ["PRJ-002 - In vitro NIST Phantom data acquired using the head coil.",
                "Notes: only data selected for paper submission are processed."],
}


def project_csvs(project: str, low_field: bool):
    """utils/metadata_utils.py:19-85 (`prj_004` / `prj_003` / `prj_002`): the CSV list a project name stands for."""
    logs = _PROJECT_LOGS[(project, bool(low_field))]
    if logs is None:
        print("Error: no data to process yet at 1.5 T.")
        raise SystemExit(1)
    return [name + ".csv" for name in logs.split()]


def set_metadata(csv_path, csvs, low_field):
    """utils/metadata_utils.py:92-125: concatenate the session log CSVs into one DataFrame; `--csv prj-004` (or
    prj-003 / prj-002) stands for that project's list of logs, with the reference's banner."""
    import pandas as pd

    if csvs[0] in _PROJECT_BANNERS:
        lines = _PROJECT_BANNERS[csvs[0]]
        rule = "*" * max(len(ln) for ln in lines)
        print("\n".join([rule] + lines + [rule]))
        csvs = project_csvs(csvs[0], low_field)
    elif ".csv" not in csvs[0].lower():
        print(f"Error: {csvs} is not a valid metadata log file nor a valid project to process (only prj-002, prj-003 and "
              "prj-004 metadata can be processed all at once.)")
        raise SystemExit(1)
    return pd.concat([pd.read_csv(os.path.join(csv_path, c)) for c in csvs])


def set_phantom_gt(low_field):
    """run_t2mapping.py:14-27 (NMR ground-truth T2 of the NIST phantom vials); returns (gt, id)."""
    if low_field:
        gt = [594, 416, 284, 221, 167, 122, 80, 53, 41]
        ids = ["T2-3", "T2-4", "T2-5", "T2-6", "T2-7", "T2-8", "T2-9", "T2-10", "T2-11"]
    else:
        gt = [1044, 624, 428, 258, 186, 137, 90, 63, 44, 27, 19, 15, 10, 8]
        ids = [f"T2-{i}" for i in range(1, 15)]
    return gt, ids


# ---- outputs -----------------------------------------------------------------------------------
def save_nifti_maps(t2_map, k_map, sigma_map, res_map, dirname, recon_img, bids_path, acq, sim, analysis):
    """utils/t2map_utils.py:18-29."""
    sitk = _sitk()
    items = []
    for arr, tag in zip([t2_map, k_map, sigma_map, res_map], ["t2", "k", "sigma", "res"]):
        img = sitk.GetImageFromArray(arr)
        img.SetSpacing(recon_img.GetSpacing())
        img.SetOrigin(recon_img.GetOrigin())
        img.SetDirection(recon_img.GetDirection())
        path = get_img_path(bids_path, acq.iloc[0], dirname)
        path = path.replace("t2map.nii.gz", "sim-" + str(sim) + f"_{tag}map_ada-{analysis}.nii.gz")
        items.append((img, path))
    if hasattr(sitk, "WriteImages"):  # native writer: the four maps are compressed concurrently
        sitk.WriteImages(items)
    else:
        for img, path in items:
            sitk.WriteImage(img, path)
    print(f"T2 map saved as nifti file in {dirname}")


def phantom_frame(stats, id, gt):
    """The table ``save_phantom_csv`` writes (utils/t2map_utils.py:55-66): ``stats`` maps the six column names to
    per-vial values.  ``np.nanmean`` / ``np.nanstd`` of a float32 map are float32 numbers (stored into float64 arrays,
    :37-48), so the values are rounded to float32 here; the text pandas then writes has the reference's digits."""
    import pandas as pd

    cols = {name: np.asarray(stats[name], np.float64).astype(np.float32).astype(np.float64)
            for name in ("meanT2", "stdT2", "meanK", "stdK", "meanC", "stdC")}
    return pd.DataFrame({"id": id, "trueT2": gt, **cols})


def save_phantom_csv(t2_map, k_map, sigma_map, label, id, gt, bids_path, acq, dirname, sim, analysis, device=0):
    """utils/t2map_utils.py:30-59: nanmean / nanstd of each map per vial label, reduced on the GPU
    (t2fit_label_stats_dev: mean, then mean squared deviation from it, as numpy computes them -- accumulated in float64
    where numpy sums the float32 values in float32, then rounded to the float32 numpy returns: the last float32 digit can
    differ from the reference's file, nothing more)."""
    n_roi = len(gt)
    stats = {}
    for arr, m, s in ((t2_map, "meanT2", "stdT2"), (k_map, "meanK", "stdK"), (sigma_map, "meanC", "stdC")):
        stats[m], stats[s], _ = t2map.label_stats(arr, label, n_roi, device=device)
    path = get_img_path(bids_path, acq.iloc[0], dirname).replace("t2map.nii.gz", f"sim-{sim}_ROI_data_ada-{analysis}.csv")
    phantom_frame(stats, id, gt).to_csv(path, index=False)


def parse_roi_spec(spec: str):
    """``--roi_stats NAME[:TISSUE]`` -> ``(NAME, TISSUE or None)``: the label image is the one of derivative directory
    ``recon_1mm_<NAME>``; with TISSUE only voxels whose FeTA label (``recon_1mm_feta``) equals it are taken."""
    name, sep, tissue = str(spec).partition(":")
    if not name or not all(ch.isalnum() or ch == "-" for ch in name):  # becomes part of a directory and a file name
        raise ValueError(f"--roi_stats {spec!r}: NAME must be made of letters, digits and '-'")
    if not sep:
        return name, None
    try:
        return name, int(tissue)
    except ValueError:
        raise ValueError(f"--roi_stats {spec!r}: TISSUE must be an integer FeTA label") from None


def roi_csv_path(bids_path, acq, dirname, sim, analysis, name):
    """The per-region table of atlas `name`, beside the maps: the phantom CSV's naming rule with ROI_<name>."""
    return get_img_path(bids_path, acq, dirname).replace("t2map.nii.gz", f"sim-{sim}_ROI_{name}_ada-{analysis}.csv")


def _read_label_image(sitk, bids_path, acqs, dirname):
    """The integer label volume of derivative directory `dirname` for this (sub, ses), or None when there is no such
    file.  The name carries an echo time, like the phantom's label image: the last echo's is looked for first (as
    phantom_labels_dirname is), then the other echoes' from the first on (utils/ada_utils.py:908 names the FeTA image
    after the first echo)."""
    for acq in [acqs[-1]] + list(acqs[:-1]):
        path = get_img_path(bids_path, acq, dirname).replace(" ", "")
        if os.path.exists(path):
            arr = np.asarray(sitk.GetArrayFromImage(sitk.ReadImage(path)))
            return (arr if arr.dtype.kind in "iu" else np.rint(arr)).astype(np.int32)
    return None


def save_roi_csvs(t2_map, k_map, sigma_map, specs, connectivity, erosion, bids_path, acqs, dirname, sim, analysis, device=0):
    """One CSV per ``--roi_stats`` entry: t2map.roi_table over t2 / k / sigma on the regions of the atlas image, eroded
    `erosion` times with generate_binary_structure(3, connectivity) (get_t2_per_roi, utils/ada_utils.py:130-216;
    compute_t2_per_tissue_feta, :885-968).  The maps are on disk by now: a label image that is missing or does not fit
    costs its table and a warning, nothing else.  Returns the paths written."""
    sitk = _sitk()
    maps = {"t2": t2_map, "k": k_map, "sigma": sigma_map}
    written = []
    for name, tissue in specs:
        label = _read_label_image(sitk, bids_path, acqs, recon_dirname + "_" + name)
        feta = _read_label_image(sitk, bids_path, acqs, feta_dirname) if tissue is not None else None
        if label is None or (tissue is not None and feta is None):
            missing = recon_dirname + "_" + name if label is None else feta_dirname
            print(f"Warning: no {missing} label image for {acqs[-1]['sub']}_{acqs[-1]['ses']}. ROI table '{name}' is skipped.")
            continue
        if label.shape != t2_map.shape or (feta is not None and feta.shape != t2_map.shape):
            print(f"Warning: label image of '{name}' does not have the maps' shape {t2_map.shape}. ROI table '{name}' is skipped.")
            continue
        frame = t2map.roi_table(maps, label, feta, tissue, connectivity=connectivity, iterations=erosion, device=device)
        path = roi_csv_path(bids_path, acqs[-1], dirname, sim, analysis, name)
        frame.to_csv(path, index=False)
        written.append(path)
        print(f"ROI table '{name}' saved as csv file in {dirname}")
    return written


BOOT_TAGS = ("T2std", "T2bias", "T2cilo", "T2cihi", "T2nok")


def parse_dict_arguments(args):
    """``--solver dict`` and its table: None without it, else ``{'t2': (lo, hi, n), 'csf': (t2_long, nf) or None}`` or
    ``{'file': path}``.  ValueError for what does not go together."""
    given = [f for f in ("dict_t2", "dict_csf", "dict_file") if getattr(args, f) is not None]
    if args.solver != "dict":
        if given:
            raise ValueError(f"--{given[0]} has no effect without --solver dict")
        return None
    if not args.gaussian:
        raise ValueError("--solver dict goes with --gaussian only: a dictionary is matched by least squares up to a scale "
                         "(a Rician expectation depends on k / sigma, so it is not scale-free)")
    if (args.dict_t2 is None) == (args.dict_file is None):
        raise ValueError("--solver dict needs a dictionary: one of --dict_t2 LO:HI:N (optionally with --dict_csf T2LONG:NF) and "
                         "--dict_file FILE.npz")
    if args.norm:
        raise ValueError("--solver dict cannot be combined with --norm: the match is scale-free already")
    if args.bootstrap:
        raise ValueError("--solver dict cannot be combined with --bootstrap: the replicas are refitted by the iterative solvers")
    if args.gpus > 1:
        raise ValueError("--solver dict runs on one GPU per volume: --gpus 1")
    n_te = len(args.TEs) if args.TEs is not None else 3
    if args.dict_file is not None:
        if args.dict_csf is not None:
            raise ValueError("--dict_csf goes with --dict_t2 (a --dict_file holds its own model)")
        from ._dict import Dictionary

        try:
            d = Dictionary.load(args.dict_file)
        except (OSError, KeyError, ValueError) as e:
            raise ValueError(f"--dict_file {args.dict_file!r}: {e}")
        if "t2" not in d.names:
            raise ValueError(f"--dict_file {args.dict_file!r} has no t2 column (it has {', '.join(d.names)})")
        if d.n_te != n_te:
            raise ValueError(f"--dict_file {args.dict_file!r} has {d.n_te} echoes per atom, {n_te} echoes are fitted")
        return {"file": args.dict_file}
    try:
        lo, hi, n = args.dict_t2.split(":")
        lo, hi, n = float(lo), float(hi), int(n)
    except ValueError:
        raise ValueError(f"--dict_t2 {args.dict_t2!r}: expected LO:HI:N, for example 20:2000:512")
    if not (0 < lo < hi and np.isfinite(hi)) or n < 2:
        raise ValueError("--dict_t2 needs 0 < LO < HI and N >= 2")
    csf = None
    if args.dict_csf is not None:
        try:
            t2_long, nf = args.dict_csf.split(":")
            t2_long, nf = float(t2_long), int(nf)
        except ValueError:
            raise ValueError(f"--dict_csf {args.dict_csf!r}: expected T2LONG:NF, for example 2000:32")
        if not (t2_long > 0 and np.isfinite(t2_long)) or nf < 1:
            raise ValueError("--dict_csf needs T2LONG > 0 and NF >= 1")
        csf = (t2_long, nf)
    if n * (csf[1] if csf else 1) > 65536:
        raise ValueError("the dictionary would have more than 65536 atoms")
    return {"t2": (lo, hi, n), "csf": csf}


def build_dictionary(spec, te_ms):
    """The dictionary of :func:`parse_dict_arguments` for these echo times [ms]."""
    from . import _dict

    if "file" in spec:
        d = _dict.Dictionary.load(spec["file"])
        if d.n_te != len(te_ms):
            raise ValueError(f"{spec['file']!r} has {d.n_te} echoes per atom, {len(te_ms)} echoes are fitted")
        return d
    grid = _dict.log_grid(*spec["t2"])
    if spec["csf"] is None:
        return _dict.monoexp(te_ms, grid)
    t2_long, nf = spec["csf"]
    return _dict.biexp(te_ms, grid, t2_long, np.arange(nf) / nf)


def _fit_subject_dict(vols, masks, keep, dictionary, device):
    """:func:`_fit_subject` for ``--solver dict``: same mask, the maps of t2map.dictionary.fit_volume_dict; sigma is 0 and res
    the RMSE of the matched atom.  Returns ``(mask, (t2, k, sigma, res), status, None, extras)`` with ``extras`` the further
    parameter maps and the atom index (int32)."""
    import torch

    echoes, mask, _ = t2map.stack_mask_flatten(vols, masks, device=device)
    if keep is not None:
        mask = mask & keep
    shape = mask.shape
    mask_d = torch.from_numpy(mask.astype(np.uint8).reshape(-1)).to(echoes.device)
    maps, extras = t2map.dictionary.fit_volume_dict(echoes.reshape((len(vols),) + shape), mask_d.reshape(shape), dictionary, device=device)
    torch.cuda.synchronize()
    out = tuple(getattr(maps, n).cpu().numpy() for n in ("t2", "k", "sigma", "res"))
    return mask, out, maps.status.cpu().numpy(), None, {n: t.cpu().numpy() for n, t in extras.items()}


def save_dict_maps(extras, recon_img, bids_path, acq, dirname, sim, analysis):
    """``--solver dict``: one map per further parameter column of the dictionary (tag = the column's name) and the atom index
    (tag dictindex, int32; -1 where nothing was matched), beside the four maps with their geometry and naming rule.  Returns
    the paths written."""
    sitk = _sitk()
    paths = []
    for name, arr in extras.items():
        img = sitk.GetImageFromArray(arr)
        img.SetSpacing(recon_img.GetSpacing())
        img.SetOrigin(recon_img.GetOrigin())
        img.SetDirection(recon_img.GetDirection())
        paths.append(boot_map_path(bids_path, acq, dirname, sim, analysis, "dictindex" if name == "index" else name))
        sitk.WriteImage(img, paths[-1])
    return paths


NNLS_DEFAULT_MU = 0.03  # t2map.spectrum.DEFAULT_MU: one sweep of the CPU statement on synth.py's phantom (README, "T2 spectra")
NNLS_CHI2_FACTOR = 1.02  # --nnls_chi2 without a value: the literature's factor (Whittall & MacKay 1989; DECAES's Chi2Factor)


def parse_nnls_arguments(args):
    """``--solver nnls`` and its grid: None without it, else ``{'t2': (lo, hi, n), 'mu': mu, 'windows': {name: (lo, hi)},
    'write_spectrum': bool}`` and, with ``--nnls_chi2`` only, ``'chi2': {'factor', 'mu_exact'}`` (``'mu'`` is then 0: the rule
    owns the weight).  ValueError for what does not go together."""
    given = ([f for f in ("nnls_t2", "nnls_mu", "nnls_window", "nnls_chi2", "nnls_chi2_fallback") if getattr(args, f, None) is not None]
             + (["write_spectrum"] if args.write_spectrum else []))
    if args.solver != "nnls":
        if given:
            raise ValueError(f"--{given[0]} has no effect without --solver nnls")
        return None
    if not args.gaussian:
        raise ValueError("--solver nnls goes with --gaussian only: the spectrum is fitted by (regularised) least squares, which is the "
                         "Gaussian likelihood")
    if args.nnls_t2 is None:
        raise ValueError("--solver nnls needs a T2 grid: --nnls_t2 LO:HI:N, for example 10:2000:40")
    if args.norm:
        raise ValueError("--solver nnls cannot be combined with --norm: --nnls_mu is absolute, in the units of the signal basis, and "
                         "the fractions are scale-free already")
    if args.bootstrap:
        raise ValueError("--solver nnls cannot be combined with --bootstrap: the replicas are refitted by the iterative solvers")
    if args.gpus > 1:
        raise ValueError("--solver nnls runs on one GPU per volume: --gpus 1")
    try:
        lo, hi, n = args.nnls_t2.split(":")
        lo, hi, n = float(lo), float(hi), int(n)
    except ValueError:
        raise ValueError(f"--nnls_t2 {args.nnls_t2!r}: expected LO:HI:N, for example 10:2000:40")
    if not (0 < lo < hi and np.isfinite(hi)) or not (2 <= n <= 64):
        raise ValueError("--nnls_t2 needs 0 < LO < HI and N in 2 .. 64")
    mu = NNLS_DEFAULT_MU if args.nnls_mu is None else float(args.nnls_mu)
    if not (mu >= 0 and np.isfinite(mu)):
        raise ValueError("--nnls_mu must be a number that is not negative")
    windows = {}
    for text in args.nnls_window or ():
        try:
            name, span = text.split("=")
            wlo, whi = (float(v) for v in span.split(":"))
        except ValueError:
            raise ValueError(f"--nnls_window {text!r}: expected NAME=LO:HI, for example csf=1000:2000")
        if not name.isalnum() or name == "lnT2" or name in windows:
            raise ValueError(f"--nnls_window {text!r}: NAME must be letters and digits, not lnT2, and given once")
        if not (0 < wlo <= whi and np.isfinite(whi)):
            raise ValueError(f"--nnls_window {text!r} needs 0 < LO <= HI")
        windows[name] = (wlo, whi)
    if len(windows) > 7:
        raise ValueError("--nnls_window can be given 7 times at most (the library takes 8 functionals, one is ln T2)")
    spec = {"t2": (lo, hi, n), "mu": mu, "windows": windows, "write_spectrum": bool(args.write_spectrum)}
    factor, fallback = getattr(args, "nnls_chi2", None), getattr(args, "nnls_chi2_fallback", None)
    if factor is None:
        if fallback is not None:
            raise ValueError("--nnls_chi2_fallback has no effect without --nnls_chi2")
        return spec
    if args.nnls_mu is not None:
        raise ValueError("--nnls_chi2 chooses the weight per voxel and cannot be combined with --nnls_mu")
    if not (factor > 1 and np.isfinite(factor)):
        raise ValueError("--nnls_chi2 FACTOR must be a number above 1, for example 1.02")
    if fallback is not None and not (fallback >= 0 and np.isfinite(fallback)):
        raise ValueError("--nnls_chi2_fallback must be a number that is not negative")
    spec["mu"] = 0.0  # the rule owns the weight
    spec["chi2"] = {"factor": float(factor), "mu_exact": NNLS_DEFAULT_MU if fallback is None else float(fallback)}
    return spec


def build_spectrum_basis(spec, te_ms):
    """The basis of :func:`parse_nnls_arguments` for these echo times [ms]."""
    return t2map.spectrum.spectrum_basis(te_ms, t2map.spectrum.log_grid(*spec["t2"]), spec["mu"], spec["windows"])


def _fit_subject_nnls(vols, masks, keep, basis, device, write_spectrum, chi2=None):
    """:func:`_fit_subject` for ``--solver nnls``: same mask, the maps of t2map.spectrum.fit_volume_nnls; t2 is the
    geometric-mean T2, k the total amplitude, sigma 0 and res the RMSE.  Returns ``(mask, (t2, k, sigma, res), status, None,
    extras)`` with ``extras`` the window fractions, nnlsiter, nnlsstatus, when asked for t2spectrum and, with ``chi2`` (the
    rule's numbers), nnlsmu, nnlschi2, nnlsrule and nnlssolves."""
    import torch

    echoes, mask, _ = t2map.stack_mask_flatten(vols, masks, device=device)
    if keep is not None:
        mask = mask & keep
    shape = mask.shape
    mask_d = torch.from_numpy(mask.astype(np.uint8).reshape(-1)).to(echoes.device)
    maps, extras = t2map.spectrum.fit_volume_nnls(echoes.reshape((len(vols),) + shape), mask_d.reshape(shape), basis, device=device,
                                                  spectrum=write_spectrum, **({"chi2": chi2} if chi2 else {}))
    torch.cuda.synchronize()
    out = tuple(getattr(maps, n).cpu().numpy() for n in ("t2", "k", "sigma", "res"))
    return mask, out, maps.status.cpu().numpy(), None, {n: t.cpu().numpy() for n, t in extras.items()}


def save_nnls_maps(extras, recon_img, bids_path, acq, dirname, sim, analysis):
    """``--solver nnls``: one map per window (tag <NAME>fraction), the outer steps (tag nnlsiter, int32), the solver's status
    (tag nnlsstatus, int32: -1 outside the mask, 0 done, 1 step limit, 2 breakdown, 3 non-finite sample), with --nnls_chi2 the
    chosen weight (tag nnlsmu), the misfit ratio reached (nnlschi2), the rule's code (nnlsrule, int32) and the solves (nnlssolves,
    int32) and, with
    --write_spectrum, the 4-D volume of the coefficients (tag t2spectrum: one volume per grid T2, written as NIfTI by this
    package's own writer), beside the four maps with their geometry and naming rule.  Returns the paths written."""
    sitk = _sitk()
    paths = []
    for name, arr in extras.items():
        paths.append(boot_map_path(bids_path, acq, dirname, sim, analysis, name))
        if arr.ndim == 4:
            from . import nifti

            nifti.WriteImage(nifti.Image(arr, recon_img.GetSpacing(), recon_img.GetOrigin(), recon_img.GetDirection()), paths[-1])
            continue
        img = sitk.GetImageFromArray(arr)
        img.SetSpacing(recon_img.GetSpacing())
        img.SetOrigin(recon_img.GetOrigin())
        img.SetDirection(recon_img.GetDirection())
        sitk.WriteImage(img, paths[-1])
    return paths


def parse_bootstrap_noise(text: str):
    """``--bootstrap_noise``: ``background`` / ``sigma_map`` / ``mppca`` as they are, anything else a noise level > 0."""
    if text in ("background", "sigma_map", "mppca"):
        return text
    try:
        level = float(text)
    except ValueError:
        raise ValueError(f"--bootstrap_noise {text!r}: expected 'background', 'sigma_map', 'mppca' or a number") from None
    if not (level > 0.0 and np.isfinite(level)):
        raise ValueError(f"--bootstrap_noise {text!r}: the noise level must be a positive number")
    return level


def boot_map_path(bids_path, acq, dirname, sim, analysis, tag):
    """A bootstrap map beside the four maps: their naming rule (save_nifti_maps) with tag T2std / T2bias / ..."""
    return get_img_path(bids_path, acq, dirname).replace("t2map.nii.gz", f"sim-{sim}_{tag}map_ada-{analysis}.nii.gz")


def save_bootstrap_maps(vols, mask, maps4, te_eff, fit, fit_params, prior, solver, precision, numpy_legacy, n_replicas, seed,
                        alpha, noise, recon_img, bids_path, acq, dirname, sim, device=0, mppca=None):
    """``--bootstrap R``: t2map.bootstrap_volume of the maps just written (the volume is not fitted again), then the
    T2 standard deviation, bias, interval bounds and replica counts as NIfTI maps with the T2 map's geometry.  Prints one
    line: noise level, R, seconds, replicas per second.  Returns the paths written.  ``noise`` ``'mppca'``: the replicas
    take the per-voxel sigma map of t2map.mppca_noise_map of the echoes (``mppca``: its radius and dims), on the path a
    fitted sigma map takes."""
    sitk = _sitk()
    t2_map, k_map, sigma_map, res_map = maps4
    echoes = np.stack([np.asarray(v, np.float32) for v in vols])
    t0 = time.time()
    level_map = t2map.mppca_noise_map(echoes, device=device, **(mppca or {}))[0] if noise == "mppca" else None
    boot = t2map.bootstrap_volume(echoes, mask, te_eff, fit, fit_params, prior=prior, n_replicas=n_replicas, seed=seed,
                                  alpha=alpha, noise_sigma=noise if level_map is None else level_map, solver=solver,
                                  precision=precision,
                                  maps=t2map.T2Maps(t2_map, k_map, sigma_map, res_map), numpy_legacy=numpy_legacy, device=device)
    dt = time.time() - t0
    level = ("the MP-PCA sigma map" if level_map is not None else
             "the fitted sigma map" if boot.noise_sigma is None else f"{boot.noise_sigma:.6g}")
    print(f"Bootstrap: noise level {level} ({noise if isinstance(noise, str) else 'given'}), {n_replicas} replicas in "
          f"{dt:.3f} sec ({n_replicas / max(dt, 1e-9):.1f} replicas/sec)")
    items = []
    for tag, arr in zip(BOOT_TAGS, (boot.boot_std, boot.boot_bias, boot.ci_lo, boot.ci_hi, boot.n_ok)):
        img = sitk.GetImageFromArray(arr)
        img.SetSpacing(recon_img.GetSpacing())
        img.SetOrigin(recon_img.GetOrigin())
        img.SetDirection(recon_img.GetDirection())
        items.append((img, boot_map_path(bids_path, acq, dirname, sim, fit, tag)))
    for img, path in items:
        sitk.WriteImage(img, path)
    return [path for _, path in items]


# ---- driver ------------------------------------------------------------------------------------
def parse_denoise_weight(text: str):
    """``--denoise_weight``: a number > 0 (intensity units), or ``<c>sigma`` = ``c`` times the background noise level of
    the stack (``sigma`` alone is ``1sigma``).  Returns ``("abs", w)`` or ``("sigma", c)``."""
    t = str(text).strip().lower()
    kind = "abs"
    if t.endswith("sigma"):
        kind, t = "sigma", (t[:-5].strip() or "1")
    try:
        v = float(t)
    except ValueError:
        raise ValueError(f"--denoise_weight {text!r}: expected a number or <c>sigma (e.g. 1sigma, 0.5sigma)") from None
    if not (v > 0.0 and np.isfinite(v)):
        raise ValueError(f"--denoise_weight {text!r}: the weight must be a positive number")
    return kind, v


def save_noise_maps(sigma, rank, recon_img, bids_path, acq, dirname, sim, analysis):
    """``--write_noise_map``: the MP-PCA noise level (float32) and signal rank (uint8) of every voxel beside the four maps,
    with their geometry and naming rule (tags mppcasigma, mppcarank).  Returns the paths written."""
    sitk = _sitk()
    paths = []
    for arr, tag in ((sigma, "mppcasigma"), (rank, "mppcarank")):
        img = sitk.GetImageFromArray(arr)
        img.SetSpacing(recon_img.GetSpacing())
        img.SetOrigin(recon_img.GetOrigin())
        img.SetDirection(recon_img.GetDirection())
        paths.append(boot_map_path(bids_path, acq, dirname, sim, analysis, tag))
        sitk.WriteImage(img, paths[-1])
    return paths


def _denoise_mppca_subject(vols, stack, radius, dims, device, maps, t0):
    """The ``--denoise mppca`` half of :func:`denoise_subject`."""
    out, noise = t2map.denoise_mppca(stack, radius=radius, dims=dims, out=stack, return_maps=True, device=device)
    host = out.cpu().numpy()
    sigma, rank = noise["sigma"].cpu().numpy(), noise["rank"].cpu().numpy()
    if maps is not None:
        maps["sigma"], maps["rank"] = sigma, rank
    seen = sigma > 0
    print(f"Denoising: MP-PCA {dims}-D, radius {radius} ({(2 * radius + 1) ** dims} voxels per window), median sigma "
          f"{float(np.median(sigma[seen])) if seen.any() else 0.0:.4g}, mean rank {float(rank[seen].mean()) if seen.any() else 0.0:.2f}, "
          f"{time.time() - t0:.3f} s")
    return [host[i] for i in range(len(vols))]


def denoise_subject(vols, masks, weight=None, dims=2, eps=2e-4, max_iter=200, device=0, joint=False, method="tv", radius=2,
                    sigma_from="background", maps=None):
    """``--denoise tv``: the decoded echo volumes through t2map.denoise_tv on the device (what the reference's
    run_denoising does to them on the host before run_t2mapping.py reads the file), ahead of the union mask and the
    fit.  ``weight``: parse_denoise_weight's pair; the ``sigma`` form measures the noise level on the voxels outside
    the union mask, before denoising.  Masks and geometry are untouched.  Returns the denoised volumes (float32).
    ``joint`` (``--denoise tv_joint``): vector-valued TV across the echoes, one problem per slice of all echoes
    (``dims=2``) or one in all (``dims=3``); the weight, ``<c>sigma`` included, is not rescaled by the echo count.
    ``sigma_from`` ``'mppca'`` (``--denoise_sigma mppca``): the ``sigma`` form takes the median of the MP-PCA noise map
    (t2map.mppca_noise_map, ``radius`` and ``dims`` as given) inside the union mask instead: a level measured in tissue.
    ``method`` ``'mppca'`` (``--denoise mppca``): the volumes through t2map.denoise_mppca instead (no weight; ``radius`` is
    that of its window); ``maps``, a dict, then receives the ``sigma`` and ``rank`` volumes it measured on the way."""
    import torch

    t0 = time.time()
    dev = torch.device("cuda", device)
    shape = tuple(np.asarray(vols[0]).shape)
    if len(shape) != 3:
        raise ValueError(f"--denoise tv needs 3-D echo volumes, got shape {shape}")
    stack = torch.empty((len(vols),) + shape, dtype=torch.float32, device=dev)
    for i, v in enumerate(vols):
        stack[i] = torch.from_numpy(np.ascontiguousarray(v).astype(np.float32, copy=False)).to(dev)
    if method == "mppca":
        return _denoise_mppca_subject(vols, stack, radius, dims, device, maps, t0)
    if weight is None:
        raise ValueError("--denoise tv needs a weight (parse_denoise_weight's pair)")
    kind, value = weight
    note = ""
    if kind == "sigma":
        union = np.zeros(shape, bool)
        for m in masks:
            union |= np.asarray(m) != 0
        if sigma_from == "mppca":
            level = t2map.mppca_noise_map(stack, radius=radius, dims=dims, device=device)[0].cpu().numpy()[union]
            sigma, count = (float(np.median(level)) if level.size else 0.0), int(level.size)
            note = f" ({value:g} x MP-PCA median sigma {sigma:.4g} over {count} voxels of the mask)"
        else:
            sigma, count = t2map.estimate_background_sigma(stack, union.astype(np.uint8), device=device)
            note = f" ({value:g} x background sigma {sigma:.4g} over {count} samples)"
        value = value * sigma
    out, info = t2map.denoise_tv(stack, value, eps=eps, max_iter=max_iter, dims=dims, out=stack, return_info=True,
                                 **({"joint": True} if joint else {}))
    n_iter = info["n_iter"].cpu().numpy()
    host = out.cpu().numpy()
    print(f"Denoising: TV-Chambolle {dims}-D{', joint across the echoes' if joint else ''}, weight {value:.4g}{note}, {n_iter.size} problems, n_iter mean "
          f"{float(n_iter.mean()):.1f} max {int(n_iter.max())}, {time.time() - t0:.3f} s")
    return [host[i] for i in range(len(vols))]


def _fit_subject(vols, masks, keep, te_eff, fit, fit_params, prior, norm, solver, precision, device, numpy_legacy=False):
    """One (sub, ses): union mask + flat indices on the device (bit-identical to
    run_t2mapping.py:383-384,412,421), fit, maps back to the host as (Z,Y,X) float32."""
    import torch

    echoes, mask, _ = t2map.stack_mask_flatten(vols, masks, device=device)
    if keep is not None:
        mask = mask & keep
    shape = mask.shape
    mask_d = torch.from_numpy(mask.astype(np.uint8).reshape(-1)).to(echoes.device)
    maps = t2map.fit_volume(echoes.reshape((len(vols),) + shape), mask_d, te_eff, fit, fit_params, prior=prior,
                            norm=norm, solver=solver, precision=precision, extras=True, numpy_legacy=numpy_legacy)
    torch.cuda.synchronize()
    out = tuple(getattr(maps, n).cpu().numpy() for n in ("t2", "k", "sigma", "res"))
    extras = {"nit": maps.nit.cpu().numpy(), "fun": maps.fun.cpu().numpy()}  # what the convergence figures need
    return mask, out, maps.status.cpu().numpy(), extras


def _dist_env():
    """(rank, world, local_rank) of this process: set by torch.distributed.run, else a single process."""
    return int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("LOCAL_RANK", "0"))


def _fit_share(e_share, m_share, te_eff, fit, fit_params, prior, norm, solver, precision, device, numpy_legacy=False):
    """This rank's share of a volume ((nTE, per) float32 and (per,) uint8: CUDA tensors, or host arrays that are sent
    first) -> ``(packed [6, per] float32 on the GPU: t2, k, sigma, res, fun, nit (int32 bit patterns), status (per,)
    uint8)``.  The only function of the shared-volume path that calls the fit."""
    import ctypes as C

    import torch

    from . import _abi
    from ._lib import check, require_gpu

    lib = require_gpu()
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        e_d = (e_share if torch.is_tensor(e_share) else torch.from_numpy(e_share)).to(dev, non_blocking=True).contiguous()
        m_d = (m_share if torch.is_tensor(m_share) else torch.from_numpy(m_share)).to(dev, non_blocking=True).contiguous()
        per = e_d.shape[1]
        packed = torch.empty((6, per), dtype=torch.float32, device=dev)
        status = torch.empty(per, dtype=torch.uint8, device=dev)
        cfg = t2map.make_config(fit, fit_params, te_eff, prior, norm, solver, precision, numpy_legacy)
        maps = _abi.T2FitMaps()
        maps.t2, maps.k, maps.sigma, maps.res, maps.fun, maps.nit = (packed[j].data_ptr() for j in range(6))
        maps.status = status.data_ptr()
        check(lib.t2fit_volume_dev(C.byref(cfg), e_d.data_ptr(), _abi.LAYOUT_TE_MAJOR, m_d.data_ptr(), per, C.byref(maps),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
    return packed, status


def _fit_subject_shared(sitk, recon_paths, mask_paths, label_path, fast, te_eff, fit, fit_params, prior, norm, solver,
                        precision, device, numpy_legacy=False):
    """One (sub, ses) over all ranks (BASELINE.json config 4, or any run with fewer subjects than ranks).

    Rank r decodes the echo files r, r + G, ... and their mask files only; the union mask (run_t2mapping.py:383-384) is
    an all-reduce of the partial unions; one all-to-all hands every rank all echoes of its balanced share of the voxels
    (dist.exchange_echo_shares); every rank fits its share; one all-gather assembles t2 / k / sigma / res / fun / nit on
    every rank and a second, a quarter its size, the status bytes -- so the `FAIL : Optimization failed` count
    (run_t2mapping.py:298-303) and the convergence figures work here as in the single-process run.
    Returns ``(mask, (t2, k, sigma, res), status, extras, recon_img, label, my_vols)``."""
    import torch
    import torch.distributed as dist

    from . import dist as t2dist

    rank, world = dist.get_rank(), dist.get_world_size()
    n_te = len(recon_paths)
    mine = t2dist.echoes_of_rank(n_te, rank, world)
    vols, masks, label, _ = _read_subject(sitk, [recon_paths[i] for i in mine], [mask_paths[i] for i in mine], label_path)
    recon_img = _read_geometry(sitk, recon_paths[-1])
    # shape of the volume: from an echo this rank decoded, else from the label, else from a peer (broadcast)
    shape = [tuple(np.asarray(vols[0]).shape) if vols else None]
    if world > 1:
        gathered = [None] * world
        dist.all_gather_object(gathered, shape[0])
        shape[0] = next(sh for sh in gathered if sh is not None)
    shape = tuple(shape[0])
    n = int(np.prod(shape))
    on_gpu = dist.get_backend() == "nccl"
    dev = torch.device("cuda", device) if on_gpu else torch.device("cpu")
    part = np.zeros(n, np.uint8)
    for m in masks:
        part |= (np.asarray(m).reshape(-1) != 0).astype(np.uint8)
    if vols:
        # (the native reader decodes into one page-locked block: sent as it lies, no staging copy)
        host = _one_block(vols) if _is_one_block(vols) else np.stack([np.asarray(v, np.float32).reshape(-1) for v in vols])
        mine_t = torch.from_numpy(host).to(dev, non_blocking=True)
    else:
        mine_t = torch.zeros((0, n), dtype=torch.float32, device=dev)
    mask_t = t2dist.union_mask_over_ranks(torch.from_numpy(part).to(dev))
    if fast and label is not None:  # run_t2mapping.py:394-400: fit the labelled vials only
        mask_t = mask_t * torch.from_numpy((np.asarray(label).reshape(-1) != 0).astype(np.uint8)).to(dev)
    e_share = t2dist.exchange_echo_shares(mine_t, n_te, n)
    m_share = t2dist.share_of(mask_t, n, rank, world)
    fitted = _fit_share(e_share, m_share, te_eff, fit, fit_params, prior, norm, solver, precision, device,
                        **({"numpy_legacy": True} if numpy_legacy else {}))
    packed, st_share = fitted if isinstance(fitted, tuple) else (fitted, None)
    if not on_gpu:
        packed = packed.cpu()
    full = t2dist.gather_maps_cyclic(packed, n).cpu().numpy()
    mask = mask_t.cpu().numpy().astype(bool).reshape(shape)
    out = tuple(np.ascontiguousarray(full[j]).reshape(shape) for j in range(4))
    if st_share is not None:
        status = t2dist.gather_maps_cyclic(st_share.view(1, -1) if on_gpu else st_share.cpu().view(1, -1), n)[0].cpu().numpy().reshape(shape)
    else:  # a fit stand-in without a status row (tests): NaN maps = infeasible bounds, everything else converged
        status = np.where(mask, np.where(np.isnan(out[0]), 4, 1), 0).astype(np.uint8)
    extras = None
    if full.shape[0] >= 6:
        extras = {"fun": np.ascontiguousarray(full[4]).reshape(shape),
                  "nit": np.ascontiguousarray(full[5]).view(np.int32).reshape(shape)}
    my_vols = {i: v for i, v in zip(mine, vols)}
    return mask, out, status, extras, recon_img, label, my_vols


def _is_one_block(vols):
    """True when the echo volumes are consecutive views of one C-contiguous float32 block (nifti.read_stack)."""
    try:
        a0 = vols[0]
        if a0.dtype != np.float32 or not a0.flags.c_contiguous:
            return False
        step = a0.nbytes
        base = a0.ctypes.data
        return all(v.dtype == np.float32 and v.flags.c_contiguous and v.ctypes.data == base + j * step for j, v in enumerate(vols))
    except AttributeError:
        return False


def _one_block(vols):
    """The (n, N) float32 view over the block `_is_one_block` recognised: no copy."""
    n = vols[0].size
    return np.lib.stride_tricks.as_strided(vols[0].reshape(-1), shape=(len(vols), n), strides=(vols[0].nbytes, 4))


def process_t2maps(metadata, bids_path, TEs, fit, fit_params, phantom, low_field, prior, fast, norm, sim,
                   solver="lbfgsb", precision="f64", device=0, plots=False, plot_seed=None, numpy_legacy=False,
                   roi_specs=(), roi_connectivity=3, roi_erosion=1, bootstrap=0, bootstrap_seed=0, bootstrap_alpha=0.05,
                   bootstrap_noise="background", denoise=None, reconstruct=None, build_mask=None, noise_map=None, dictionary=None,
                   spectrum=None):
    """run_t2mapping.py:333-479 with the voxel loop on the GPU.  ``plots``: also write the reference's
    convergence-study figures (:465-468) under <prj>/ada/convergence_analysis.  ``roi_specs``: (name, tissue) pairs
    of --roi_stats; each adds a per-region table after the maps (save_roi_csvs).  ``bootstrap`` > 0: that many
    replicas of the parametric bootstrap after the maps (save_bootstrap_maps).  ``denoise``: None, or the keyword
    arguments of denoise_subject (--denoise tv): the echoes are denoised after decoding, before the mask and the fit.
    ``reconstruct``: None, or the keyword arguments of recon.reconstruct_subject (--reconstruct): the echoes are not read
    from recon_1mm but reconstructed in memory from the acquired ax / cor / sag stacks, ahead of the denoiser.
    ``build_mask``: None, or the keyword arguments of build_phantom_subject (--build_mask phantom): the masks of every
    echo and the vial labels are built on the device from the volumes about to be fitted (after the reconstruction, if
    any) and used in place of the recon_1mm_mask / recon_1mm_label files.  ``noise_map``: None, or ``{'radius', 'dims'}`` of
    the MP-PCA noise map, with ``'write': True`` for --write_noise_map (save_noise_maps, of the echoes before any denoising);
    --bootstrap_noise mppca reads its radius and dims.  ``dictionary``: the table of ``--solver dict`` (parse_dict_arguments).
    ``spectrum``: the grid of ``--solver nnls`` (parse_nnls_arguments)."""
    sitk = _sitk()
    if (solver == "dict") != (dictionary is not None):
        raise ValueError("solver 'dict' and a dictionary go together")
    if (solver == "nnls") != (spectrum is not None):
        raise ValueError("solver 'nnls' and a spectrum grid go together")
    tes_s = [x / 1000 for x in TEs]
    metadata = metadata[metadata["EchoTime"].isin(tes_s)]
    # more than one process (--gpus N): whole subjects are dealt to the ranks when there are enough of them, otherwise
    # every volume is shared by all ranks and rank 0 writes its files
    rank, world, _ = _dist_env()
    subjects = [(prj, sub, ses) for prj, prj_md in metadata.groupby("prj") for (sub, ses), _ in prj_md.groupby(["sub", "ses"])]
    share_volumes = world > 1 and len(subjects) < world
    if denoise and share_volumes:
        raise ValueError("--denoise is not run on a volume that is shared by several ranks (each rank holds a part of the "
                         "echoes): give at least as many subjects as ranks, or run on one GPU")
    if reconstruct is not None and share_volumes:
        raise ValueError("--reconstruct is not run on a volume that is shared by several ranks (each rank holds a part of the "
                         "echoes): give at least as many subjects as ranks, or run on one GPU")
    if build_mask is not None and share_volumes:
        raise ValueError("--build_mask is not run on a volume that is shared by several ranks (each rank holds a part of the "
                         "echoes): give at least as many subjects as ranks, or run on one GPU")
    if build_mask is not None and not phantom:
        raise ValueError("--build_mask phantom goes with --in_vitro / --in_vitro_fast")
    write_noise = bool(noise_map and noise_map.get("write"))
    mppca_window = {k: noise_map[k] for k in ("radius", "dims") if k in noise_map} if noise_map else {}
    if write_noise and share_volumes:
        raise ValueError("--write_noise_map is not run on a volume that is shared by several ranks (each rank holds a part of the "
                         "echoes): give at least as many subjects as ranks, or run on one GPU")
    if dictionary is not None and share_volumes:
        raise ValueError("--solver dict is not run on a volume that is shared by several ranks: give at least as many subjects "
                         "as ranks, or run on one GPU")
    if spectrum is not None and share_volumes:
        raise ValueError("--solver nnls is not run on a volume that is shared by several ranks: give at least as many subjects "
                         "as ranks, or run on one GPU")
    mine = set(subjects if (world == 1 or share_volumes) else
               [subjects[i] for i in dist_subjects_of_rank(len(subjects), rank, world)])
    writer = (rank == 0) or not share_volumes
    for prj, prj_md in metadata.groupby("prj"):
        for (sub, ses), sub_md in prj_md.groupby(["sub", "ses"]):
            if (prj, sub, ses) not in mine:
                continue
            recon_paths, mask_paths, te_eff, label_path, acqs = [], [], [], None, []
            for echotime, acq in sub_md.groupby("EchoTime"):
                te_eff.append(echotime * 1000)
                acqs.append(acq.iloc[0])
                recon_paths.append(get_img_path(bids_path, acq.iloc[0], recon_dirname).replace(" ", ""))
                mask_paths.append(get_img_path(bids_path, acq.iloc[0], mask_dirname).replace(" ", ""))
                if phantom:
                    label_path = get_img_path(bids_path, acq.iloc[0], phantom_labels_dirname).replace(" ", "")
            te_eff = np.array(te_eff)
            if not np.array_equal(te_eff, TEs):
                print(f"Warning: one or more TEs selected to fit is missing for {sub}_{ses}. T2 fit is skipped.")
                continue
            print(f"T2 Mapping: {prj}_{sub}_{ses}")
            print(f"TEeffs: {te_eff}")
            print(f"Fitting using {fit} model ... ")
            my_vols = None
            if share_volumes:  # every rank decodes 1/G of the echo files; shares are swapped on the way to the fit
                t0 = time.time()
                mask, maps4, status, extras, recon_img, label, my_vols = _fit_subject_shared(
                    sitk, recon_paths, mask_paths, label_path, phantom and fast, te_eff, fit, fit_params, prior, norm, solver,
                    precision, device, numpy_legacy)
                vols = None
            else:
                if reconstruct is not None:
                    from . import recon

                    vols, recon_img = recon.reconstruct_subject(sitk, bids_path, sub_md, sub, ses, device=device, **reconstruct)
                    if build_mask is not None:
                        masks, label = build_phantom_subject(vols, device=device, **build_mask)
                    else:
                        _, masks, label, _ = _read_masks(sitk, mask_paths, label_path)
                    bad = [tuple(np.asarray(m).shape) for m in masks if tuple(np.asarray(m).shape) != vols[0].shape]
                    if bad:
                        raise ValueError(f"--reconstruct: the mask of {sub}_{ses} has shape {bad[0]}, the reconstructed grid "
                                         f"has {vols[0].shape}: masks must be drawn on the reconstruction that is fitted")
                elif build_mask is not None:
                    vols, recon_img = _read_echoes(sitk, recon_paths)
                    masks, label = build_phantom_subject(vols, device=device, **build_mask)
                else:
                    vols, masks, label, recon_img = _read_subject(sitk, recon_paths, mask_paths, label_path)
                keep = (label != 0) if (phantom and fast) else None  # :394-400
                noise_maps = {}
                if write_noise and not (denoise and denoise.get("method") == "mppca"):
                    noise_maps["sigma"], noise_maps["rank"] = t2map.mppca_noise_map(
                        np.stack([np.asarray(v, np.float32) for v in vols]), device=device, **mppca_window)
                if denoise:
                    vols = denoise_subject(vols, masks, device=device, **denoise,
                                           **({"maps": noise_maps} if write_noise and not noise_maps else {}))
                t0 = time.time()
                dict_maps = None
                if dictionary is not None:
                    mask, maps4, status, extras, dict_maps = _fit_subject_dict(vols, masks, keep, build_dictionary(dictionary, te_eff),
                                                                               device)
                elif spectrum is not None:
                    mask, maps4, status, extras, dict_maps = _fit_subject_nnls(vols, masks, keep, build_spectrum_basis(spectrum, te_eff),
                                                                               device, spectrum["write_spectrum"], spectrum.get("chi2"))
                else:
                    fitted = _fit_subject(vols, masks, keep, te_eff, fit, fit_params, prior, norm, solver, precision, device,
                                          **({"numpy_legacy": True} if numpy_legacy else {}))
                    mask, maps4, status = fitted[:3]
                    extras = fitted[3] if len(fitted) > 3 else None
            t2_map, k_map, sigma_map, res_map = maps4
            print(f"Dimensions of the t2w images: {mask.shape + (te_eff.size,)} (z,y,x,necho)")
            print(f"Mask Dimension: {mask.shape} -  Number of voxels inside mask: {int(np.sum(mask))}")
            if np.any(status == 4):  # scipy raises here and the reference's pool.map aborts the run
                raise ValueError("LBFGSB - one of the lower bounds is greater than an upper bound.")
            n_fail = int(np.sum((status != 1) & (status != 0)))
            if n_fail:
                print(f"FAIL : Optimization failed for {n_fail} voxels")
            print(f"... done. Time to fit: {round(time.time() - t0, 4)} sec")
            want_plots = plots and extras is not None and solver != "loglin"  # the closed form has no iterations to plot
            picks = rows = None
            if want_plots and share_volumes:
                # the sampled voxels' rows come from the ranks that decoded each echo: rank 0 draws the sample (the
                # reference's is unseeded), everybody contributes its echoes' columns
                import torch
                import torch.distributed as dist

                from . import convergence
                from . import dist as t2dist

                mask_idx = np.flatnonzero(mask.reshape(-1))
                box = [convergence.pick_voxels(len(mask_idx), plot_seed) if rank == 0 else None]
                dist.broadcast_object_list(box, src=0)
                picks = box[0]
                dev = torch.device("cuda", device) if dist.get_backend() == "nccl" else torch.device("cpu")
                rows = t2dist.rows_from_owners(mask_idx[list(picks[0]) + list(picks[1])], my_vols, len(te_eff), dev)
            if not writer:
                continue
            if want_plots:
                from . import convergence

                convergence.convergence_study(convergence.set_ada_path(bids_path, prj), vols,
                                              np.flatnonzero(mask.reshape(-1)), t2_map, extras["nit"], extras["fun"],
                                              te_eff, fit, fit_params, prior, norm, sub, ses, sim, solver=solver,
                                              precision=precision, device=device, seed=plot_seed, picks=picks, rows=rows,
                                              numpy_legacy=numpy_legacy)
            save_nifti_maps(t2_map, k_map, sigma_map, res_map, t2map_dirname, recon_img, bids_path, acq, sim, fit)
            if dictionary is not None:
                save_dict_maps(dict_maps, recon_img, bids_path, acq.iloc[0], t2map_dirname, sim, fit)
            if spectrum is not None:
                save_nnls_maps(dict_maps, recon_img, bids_path, acq.iloc[0], t2map_dirname, sim, fit)
            if write_noise:
                save_noise_maps(noise_maps["sigma"], noise_maps["rank"], recon_img, bids_path, acq.iloc[0], t2map_dirname, sim, fit)
            if phantom:
                # the reference unpacks (gt, id) as id, gt (run_t2mapping.py:27 vs :478), which swaps the
                # CSV's `id` and `trueT2` columns; kept so the output file is identical
                id_, gt_ = set_phantom_gt(low_field)
                save_phantom_csv(t2_map, k_map, sigma_map, label, id_, gt_, bids_path, acq, t2map_dirname, sim, fit,
                                 device=device)
            if roi_specs:  # (only the writer rank gets here; the maps are complete on it)
                save_roi_csvs(t2_map, k_map, sigma_map, roi_specs, roi_connectivity, roi_erosion, bids_path, acqs,
                              t2map_dirname, sim, fit, device=device)
            if bootstrap and vols is None:
                print("Warning: --bootstrap is not run on a volume that is shared by several ranks. Bootstrap maps are skipped.")
            elif bootstrap:
                save_bootstrap_maps(vols, mask, maps4, te_eff, fit, fit_params, prior, solver, precision, numpy_legacy,
                                    bootstrap, bootstrap_seed, bootstrap_alpha, bootstrap_noise, recon_img, bids_path,
                                    acq.iloc[0], t2map_dirname, sim, device=device,
                                    **({"mppca": mppca_window} if bootstrap_noise == "mppca" else {}))


def dist_subjects_of_rank(n_subjects, rank, world):
    from . import dist as t2dist

    return t2dist.subjects_of_rank(n_subjects, rank, world)


_EXCLUSIVE_GROUPS = (
    (("in_vivo", "in vivo subject data"),
     ("in_vitro", "NIST phantom, full maps"),
     ("in_vitro_fast", "NIST phantom, labelled vials only")),
    (("gaussian", "2-parameter least squares  k*exp(-TE/T2)"),
     ("gaussian_rician", "3-parameter least squares  sqrt(k^2 exp(-2TE/T2) + sigma^2)"),
     ("rician", "3-parameter Rician likelihood")),
    (("lf", "0.55 T tables and default echo times"),
     ("hf", "1.5 T tables and default echo times")),
)


def parse_arguments(argv=None):
    """Flag set of run_t2mapping.py:483-518 (three required one-of groups, --sim, --TEs, --no_prior,
    --norm) plus --solver / --precision / --device."""
    p = argparse.ArgumentParser(prog="fetal_t2mapping_amd.cli", description="voxel-wise T2 mapping on an MI355X")
    p.add_argument("--path", required=True, help="root of the qMRI tree (contains projects/ and dicom/logs/)")
    p.add_argument("--csv", nargs="+", required=True, help="metadata log CSV file name(s) under dicom/logs/")
    for group in _EXCLUSIVE_GROUPS:
        g = p.add_mutually_exclusive_group(required=True)
        for flag, text in group:
            g.add_argument("--" + flag, action="store_true", help=text)
    p.add_argument("--sim", required=True, help="identifier written into the output file names")
    p.add_argument("--TEs", nargs="+", type=int, help="echo times [ms] to fit (default 114/115, 202, 299)")
    p.add_argument("--no_prior", action="store_true", help="k >= S(TE0) instead of the table's lower bound")
    p.add_argument("--norm", action="store_true", help="divide each voxel's samples by their maximum")
    p.add_argument("--solver", choices=["lbfgsb", "lm", "loglin", "dict", "nnls"], default="lbfgsb",
                   help="lbfgsb: the reference's solver and stop rules (default); lm: converged bounded LM; "
                        "loglin: closed-form weighted log-linear fit (--gaussian only); dict: dictionary matching against "
                        "the table of --dict_t2 / --dict_csf / --dict_file (--gaussian only; the res map is then the RMSE of "
                        "the matched atom, sigma is 0, and every further parameter column and the atom index get a map)")
    p.add_argument("--nnls_t2", metavar="LO:HI:N",
                   help="--solver nnls (--gaussian only): a non-negative T2 spectrum over N (2..64) T2 values from LO to HI ms, "
                        "log-spaced, by regularised non-negative least squares; the t2 map is then the geometric-mean T2, k the "
                        "total amplitude, sigma 0 and res the RMSE")
    p.add_argument("--nnls_mu", type=float, metavar="MU",
                   help=f"--solver nnls: Tikhonov weight, absolute, in the units of the basis exp(-TE/T2) (default {NNLS_DEFAULT_MU})")
    p.add_argument("--nnls_chi2", type=float, nargs="?", const=NNLS_CHI2_FACTOR, metavar="FACTOR",
                   help="--solver nnls: choose the Tikhonov weight per voxel by the chi^2 rule: the weight at which the misfit is "
                        f"FACTOR (default {NNLS_CHI2_FACTOR}) times the unregularised misfit; not with --nnls_mu.  Also writes the maps "
                        "nnlsmu (the weight), nnlschi2 (the misfit ratio reached), nnlsrule (0 found, 1 exact fit: the fallback "
                        "weight, 2 the first weight is already above, 3 the last weight is still below) and nnlssolves")
    p.add_argument("--nnls_chi2_fallback", type=float, metavar="MU",
                   help=f"--nnls_chi2: the weight of a voxel whose unregularised fit is exact (default {NNLS_DEFAULT_MU})")
    p.add_argument("--nnls_window", action="append", metavar="NAME=LO:HI",
                   help="--solver nnls: also write the signal fraction with LO <= T2 <= HI ms as the map <NAME>fraction (up to 7)")
    p.add_argument("--write_spectrum", action="store_true",
                   help="--solver nnls: also write the coefficients as a 4-D volume, one volume per grid T2 (tag t2spectrum)")
    p.add_argument("--dict_t2", metavar="LO:HI:N", help="--solver dict: mono-exponential atoms at N T2 values from LO to HI ms, log-spaced")
    p.add_argument("--dict_csf", metavar="T2LONG:NF",
                   help="with --dict_t2: two compartments, (1 - f) exp(-TE/T2) + f exp(-TE/T2LONG), at NF fractions f = 0, 1/NF, .. "
                        "in [0, 1); writes a fraction map")
    p.add_argument("--dict_file", metavar="FILE.npz",
                   help="--solver dict: a dictionary saved by t2map.dictionary.Dictionary.save (atoms, params, names; a t2 "
                        "column; as many echoes as are fitted)")
    p.add_argument("--precision", choices=["f64", "f32"], default="f64", help="arithmetic of the lm solver")
    p.add_argument("--device", type=int, default=0, help="HIP device ordinal (one process; with --gpus each rank uses its own)")
    p.add_argument("--gpus", type=int, default=1,
                   help="GPUs of this node to use: N > 1 starts one process per GPU (torch.distributed.run, RCCL); subjects "
                        "are dealt to the ranks, or, with fewer subjects than ranks, every volume is cut over the ranks")
    p.add_argument("--numpy_legacy", action="store_true",
                   help="reproduce the reference as it runs under the numpy < 2 it freezes (requirements_frozen.txt:103): "
                        "float32 log term of the rician objective, float32 prediction of the residual map; default: numpy >= 2")
    p.add_argument("--plots", action="store_true",
                   help="write the reference's convergence-study PNGs (run_t2mapping.py:465-468) under "
                        "<prj>/ada/convergence_analysis; off by default, the reference always draws them")
    p.add_argument("--plot_seed", type=int, default=None, help="seed of the voxel sample in the figures")
    p.add_argument("--roi_stats", action="append", default=[], metavar="NAME[:TISSUE]",
                   help="after the maps, write the per-region table (mean / std / median of t2, k, sigma over the eroded "
                        "regions) of the label image recon_1mm_<NAME>, inside FeTA tissue TISSUE (recon_1mm_feta) when given; "
                        "repeatable: --roi_stats ho:2 --roi_stats jhu:3 --roi_stats feta are the reference's ROI routines")
    p.add_argument("--roi_connectivity", type=int, choices=[1, 2, 3], default=3,
                   help="erosion element generate_binary_structure(3, c): 6 / 18 / 26 neighbours (default 3, the reference's)")
    p.add_argument("--roi_erosion", type=int, default=1, help="erosion iterations of the regions, 0..8 (default 1)")
    p.add_argument("--bootstrap", type=int, default=0, metavar="R",
                   help="after the maps, R replicas of the parametric bootstrap (simulate from the fitted k, T2 with noise, refit "
                        "with the same solver and bounds): writes the T2std, T2bias, T2cilo, T2cihi and T2nok maps beside them")
    p.add_argument("--bootstrap_seed", type=int, default=0, help="seed of the replica stream (default 0)")
    p.add_argument("--bootstrap_alpha", type=float, default=0.05,
                   help="the interval maps are the alpha/2 and 1 - alpha/2 percentiles (default 0.05: a 95 %% interval)")
    p.add_argument("--bootstrap_noise", default="background", metavar="{background,sigma_map,mppca,<float>}",
                   help="noise level of the replicas: measured on the voxels outside the mask (default), the fitted sigma of "
                        "every voxel (3-parameter fits only), or a number")
    p.add_argument("--reconstruct", action="store_true",
                   help="do not read recon_1mm: reconstruct every echo in memory from the acquired ax / cor / sag stacks "
                        "(resample to --recon_res mm, merge on the --recon_fixed grid; python -m fetal_t2mapping_amd.recon "
                        "writes the same volumes), ahead of --denoise and the fit; off by default")
    p.add_argument("--recon_fixed", choices=["ax", "cor", "sag"], default="ax", help="grid of the reconstruction (default ax)")
    p.add_argument("--recon_res", type=float, default=1.0, help="isotropic resolution of the reconstruction [mm] (default 1)")
    p.add_argument("--recon_transforms", default=None, metavar="DIR",
                   help="rigid transforms <sub>_<ses>_<orientation>.txt of the moving stacks (4 x 4 text, fixed point -> "
                        "moving point); a missing file is the identity")
    p.add_argument("--recon_register", action="store_true",
                   help="with --reconstruct: find the transforms of the moving stacks on the GPU (recon.py --register)")
    p.add_argument("--recon_register_metric", choices=["corr", "mattes"], default="corr",
                   help="with --recon_register / --recon_register_echoes: the cost (recon.py --register_metric; default corr)")
    p.add_argument("--recon_n4", action="store_true",
                   help="with --reconstruct: N4 bias-field correction of the acquired stacks on the GPU first (recon.py --n4 "
                        "with its defaults)")
    p.add_argument("--recon_register_echoes", action="store_true",
                   help="with --reconstruct: register every merged echo onto the first one (recon.py --register_echoes)")
    from .recon import add_sr_arguments, add_unring_arguments, sr_arguments, unring_arguments

    add_sr_arguments(p, "recon_")
    add_unring_arguments(p, "recon_")
    p.add_argument("--build_mask", choices=["phantom"], default=None,
                   help="build the masks of every echo and the vial labels on the GPU from the volumes about to be fitted "
                        "(after --reconstruct if given) instead of reading recon_1mm_mask / recon_1mm_label: phantom = the "
                        "reference's build_phantom_masks and build_phantom_labels_v2; needs --phantom_seeds; off by default")
    p.add_argument("--phantom_seeds", default=None, metavar="FILE",
                   help="JSON list of [x, y, z] voxel indices, one per vial in label order")
    p.add_argument("--denoise", choices=["tv", "tv_joint", "mppca"], default=None,
                   help="denoise the echo volumes on the GPU before the fit: tv = TV-Chambolle as scikit-image's "
                        "denoise_tv_chambolle, the reference's run_denoising; tv_joint = vector-valued TV across the echoes "
                        "(one gradient norm per voxel, so all echoes share one edge set; the weight is not rescaled: the "
                        "joint norm of pure noise is about sqrt(nTE) times one echo's, so a weight that suits tv is about "
                        "sqrt(nTE) too small); mppca = Marchenko-Pastur PCA across the echoes (dwidenoise's estimator): no "
                        "weight to tune, --denoise_patch sets its window; off by default")
    p.add_argument("--denoise_weight", default="0.1", metavar="{W,<c>sigma}",
                   help="TV weight in intensity units (default 0.1, the reference's, which barely changes images with "
                        "values in the hundreds), or <c>sigma: c times the background noise level measured outside the mask")
    p.add_argument("--denoise_dims", type=int, choices=[2, 3], default=2,
                   help="2: every slice on its own (default, the reference's); 3: every volume as a whole")
    p.add_argument("--denoise_eps", type=float, default=2e-4, help="relative energy change that stops a problem (default 2e-4)")
    p.add_argument("--denoise_iter", type=int, default=200, help="iteration limit of a problem (default 200)")
    p.add_argument("--denoise_patch", type=int, default=2, metavar="R",
                   help="MP-PCA: radius of the (2R+1)^dims window, 1..4 (default 2); the window must hold more voxels than "
                        "there are echoes")
    p.add_argument("--denoise_sigma", choices=["background", "mppca"], default="background",
                   help="where the sigma of a <c>sigma weight of tv / tv_joint comes from: background = the voxels outside "
                        "the mask (default); mppca = the median of the MP-PCA noise map inside the mask")
    p.add_argument("--write_noise_map", action="store_true",
                   help="also write the MP-PCA noise level and signal rank of every voxel (of the echoes before any "
                        "denoising) beside the maps; window by --denoise_patch / --denoise_dims")
    args = p.parse_args(argv)
    try:
        args.dict_args = parse_dict_arguments(args)
        args.nnls_args = parse_nnls_arguments(args)
    except ValueError as e:
        p.error(str(e))
    args.reconstruct_args = None
    given = [f for f in ("--recon_fixed", "--recon_res", "--recon_transforms", "--recon_register", "--recon_register_echoes",
                         "--recon_n4", "--recon_register_metric", "--recon_method", "--recon_unring")
             if any(a == f or a.startswith(f + "=") for a in (argv if argv is not None else sys.argv[1:]))]
    if given and not args.reconstruct:
        p.error(f"{given[0]} has no effect without --reconstruct")
    if args.reconstruct:
        if not (args.recon_res > 0.0 and np.isfinite(args.recon_res)):
            p.error("--recon_res must be a positive number")
        if args.recon_transforms is not None and not os.path.isdir(args.recon_transforms):
            p.error(f"--recon_transforms {args.recon_transforms!r} is not a directory")
        if args.recon_transforms is not None and (args.recon_register or args.recon_register_echoes):
            p.error("--recon_transforms supplies the transforms: it does not go with --recon_register / --recon_register_echoes")
        args.reconstruct_args = {"fixed": args.recon_fixed, "res": args.recon_res, "transforms_dir": args.recon_transforms}
        if args.recon_register:
            args.reconstruct_args["register"] = True
        if args.recon_register_echoes:
            args.reconstruct_args["register_echoes"] = True
        if args.recon_register_metric != "corr":
            if not (args.recon_register or args.recon_register_echoes):
                p.error("--recon_register_metric has no effect without --recon_register / --recon_register_echoes")
            args.reconstruct_args["register_metric"] = args.recon_register_metric
        if args.recon_n4:
            from .recon import N4_DEFAULTS

            args.reconstruct_args["n4"] = dict(N4_DEFAULTS)
    unring = unring_arguments(p, args, "recon_", argv)  # (after the check above: --recon_unring needs --reconstruct)
    if unring is not None:
        args.reconstruct_args["unring"] = unring
    sr = sr_arguments(p, args, "recon_", argv)  # after the check above: --recon_method needs --reconstruct
    if sr is not None:
        args.reconstruct_args["sr"] = sr
    args.build_mask_args = None
    if args.phantom_seeds is not None and not args.build_mask:
        p.error("--phantom_seeds has no effect without --build_mask phantom")
    if args.build_mask:
        if not (args.in_vitro or args.in_vitro_fast):
            p.error("--build_mask phantom goes with --in_vitro / --in_vitro_fast")
        if args.phantom_seeds is None:
            p.error("--build_mask phantom needs --phantom_seeds FILE (the vial labels are painted at the seeds)")
        try:
            args.build_mask_args = {"seeds": load_seeds(args.phantom_seeds)}
        except (OSError, ValueError) as e:
            p.error(str(e))
    args.denoise_args = None
    given = [f for f in ("--denoise_weight", "--denoise_dims", "--denoise_eps", "--denoise_iter", "--denoise_patch", "--denoise_sigma")
             if any(a == f or a.startswith(f + "=") for a in (argv if argv is not None else sys.argv[1:]))]
    # what runs MP-PCA: the denoiser itself, the noise map, the bootstrap's noise level, the sigma of a TV weight
    uses_mppca = (args.denoise == "mppca" or args.write_noise_map or (args.bootstrap and args.bootstrap_noise == "mppca")
                  or (args.denoise in ("tv", "tv_joint") and args.denoise_sigma == "mppca"))
    window_flags = ("--denoise_patch", "--denoise_dims")
    stray = [f for f in given if not (f in window_flags and uses_mppca)]
    if "--denoise_patch" in given and not uses_mppca:
        p.error("--denoise_patch is the MP-PCA window: it goes with --denoise mppca, --denoise_sigma mppca, --write_noise_map or "
                "--bootstrap_noise mppca")
    if stray and not args.denoise:
        p.error(f"{stray[0]} has no effect without --denoise tv")
    if not 1 <= args.denoise_patch <= 4:
        p.error("--denoise_patch must be in 1..4")
    args.noise_map_args = None
    if uses_mppca:
        args.noise_map_args = {"radius": args.denoise_patch, "dims": args.denoise_dims}
        if args.write_noise_map:
            args.noise_map_args["write"] = True
    if args.denoise == "mppca":
        tv_only = [f for f in given if f in ("--denoise_weight", "--denoise_eps", "--denoise_iter", "--denoise_sigma")]
        if tv_only:
            p.error(f"{tv_only[0]} belongs to --denoise tv / tv_joint: MP-PCA has no weight and no iteration (its window is "
                    "--denoise_patch and --denoise_dims)")
        if args.bootstrap:
            p.error("--denoise cannot be combined with --bootstrap: the replicas would not pass through the denoiser, so "
                    "their spread would not be that of the fitted maps")
        args.denoise_args = {"method": "mppca", "radius": args.denoise_patch, "dims": args.denoise_dims}
    elif args.denoise:
        try:
            weight = parse_denoise_weight(args.denoise_weight)
        except ValueError as e:
            p.error(str(e))
        if not (args.denoise_eps >= 0.0 and np.isfinite(args.denoise_eps)):
            p.error("--denoise_eps must be >= 0")
        if args.denoise_iter < 1:
            p.error("--denoise_iter must be >= 1")
        if args.bootstrap:
            p.error("--denoise cannot be combined with --bootstrap: the replicas would not pass through the denoiser, so "
                    "their spread would not be that of the fitted maps")
        args.denoise_args = {"weight": weight, "dims": args.denoise_dims, "eps": args.denoise_eps, "max_iter": args.denoise_iter}
        if args.denoise == "tv_joint":
            args.denoise_args["joint"] = True
        if args.denoise_sigma == "mppca":
            if weight[0] != "sigma":
                p.error("--denoise_sigma mppca has no effect on a weight in intensity units: give --denoise_weight <c>sigma")
            args.denoise_args.update(sigma_from="mppca", radius=args.denoise_patch)
    if args.bootstrap:
        try:
            args.bootstrap_noise = parse_bootstrap_noise(args.bootstrap_noise)
        except ValueError as e:
            p.error(str(e))
        if not 2 <= args.bootstrap <= 512:
            p.error("--bootstrap needs 2..512 replicas (the interval maps are percentiles over them)")
        if not 0.0 < args.bootstrap_alpha < 1.0:
            p.error("--bootstrap_alpha must lie in (0, 1)")
        if args.norm:
            p.error("--bootstrap cannot be combined with --norm: the maps of a normalised fit are in per-voxel units, and the "
                    "noise level would have to be too")
        if args.in_vitro_fast:
            p.error("--bootstrap cannot be combined with --in_vitro_fast: the noise level is measured outside the mask, and the "
                    "fast phantom run masks everything but the vials; use --in_vitro")
        if args.bootstrap_noise == "sigma_map" and args.gaussian:
            p.error("--bootstrap_noise sigma_map needs a fitted sigma: use it with --gaussian_rician or --rician")
    try:
        args.roi_specs = [parse_roi_spec(spec) for spec in args.roi_stats]
    except ValueError as e:
        p.error(str(e))
    if not 0 <= args.roi_erosion <= 8:
        p.error("--roi_erosion must be in 0..8")
    return args


def _relaunch_per_gpu(args, argv):
    """--gpus N from a plain invocation: start N ranks of this module under torch.distributed.run as a child process
    and leave with its exit code.  Runs before anything has touched a GPU (a process that has initialised HIP must not
    spawn the ranks' parent on this platform, and needs no device itself)."""
    import socket
    import subprocess

    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "fetal_t2mapping_amd.cli",
           *(list(argv) if argv is not None else sys.argv[1:])]
    raise SystemExit(subprocess.call(cmd))


def main(argv=None):
    """run_t2mapping.py:522-576."""
    args = parse_arguments(argv)
    rank, world, local_rank = _dist_env()
    if args.gpus > 1 and world == 1:
        _relaunch_per_gpu(args, argv)
    if world > 1:  # a rank started by torch.distributed.run: its own GPU, one process group for the node
        import torch
        import torch.distributed as dist

        backend = os.environ.get("T2FIT_CLI_BACKEND", "nccl")  # "gloo": rehearsal of the control flow without RCCL
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC between the ranks' processes (before HIP starts)
        if backend == "nccl":
            args.device = local_rank
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    if not os.path.exists(args.path):
        print(f"Error: The specified path does not exist: {args.path}")
        raise SystemExit(1)
    bids_path = os.path.join(args.path, "projects/")
    csv_path = os.path.join(args.path, "dicom/logs/")
    low_field = bool(args.lf)
    TEs = args.TEs if args.TEs is not None else ([114, 202, 299] if args.lf else [115, 202, 299])
    phantom = bool(args.in_vitro or args.in_vitro_fast)
    fast = bool(args.in_vitro_fast)
    if args.norm:
        print("Warning: Fitting using normalization is not optimal !")
    fit, fit_params = t2map.set_fit_params(args)
    metadata = set_metadata(csv_path, args.csv, low_field)
    try:
        process_t2maps(metadata, bids_path, TEs, fit, fit_params, phantom, low_field, not args.no_prior, fast,
                       bool(args.norm), args.sim, solver=args.solver, precision=args.precision, device=args.device,
                       plots=args.plots, plot_seed=args.plot_seed, numpy_legacy=args.numpy_legacy,
                       roi_specs=args.roi_specs, roi_connectivity=args.roi_connectivity, roi_erosion=args.roi_erosion,
                       bootstrap=args.bootstrap, bootstrap_seed=args.bootstrap_seed, bootstrap_alpha=args.bootstrap_alpha,
                       bootstrap_noise=args.bootstrap_noise, **({"denoise": args.denoise_args} if args.denoise_args else {}),
                       **({"reconstruct": args.reconstruct_args} if args.reconstruct_args else {}),
                       **({"build_mask": args.build_mask_args} if args.build_mask_args else {}),
                       **({"noise_map": args.noise_map_args} if args.noise_map_args else {}),
                       **({"dictionary": args.dict_args} if args.dict_args else {}),
                       **({"spectrum": args.nnls_args} if args.nnls_args else {}))
    finally:
        if world > 1:
            import torch.distributed as dist

            if dist.is_initialized():
                dist.barrier()
                dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1:])
