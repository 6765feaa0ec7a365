"""Steps 1 and 2 of the reference's run_qmri_reconstruction.py on the GPU: every acquired thick-slice stack is resampled
to an isotropic grid (run_resample_volume, utils/qmri_utils.py:35-58), the cor and sag volumes of an echo are resampled
onto the ax grid and the three are averaged (run_reconstruct_volume, :359-391), and the result is denoised
(run_denoising, :393-405) and written under ``recon_1mm`` with the reference's file names, where cli.py reads it.

    python -m fetal_t2mapping_amd.recon --path <qMRI root> --csv <log.csv ...> (--in_vivo | --in_vitro) (--lf | --hf)

Rigid transforms of the moving stacks come from one of two places.  ``--transforms DIR`` supplies them as 4 x 4 text
matrices (fixed point -> moving point, LPS millimetres); a missing file is the identity, the reference's own reading of
``recon_1mm`` when nothing moved.  ``--register`` finds them on the GPU (``t2map.register.register_rigid``: the recipe of the
reference's registration_itk, or with ``--register_metric mattes`` the Mattes mutual information that elastix, which the
reference calls, minimises -- over every voxel and by another descent; parity unpinned): per echo, each moving 1 mm
volume onto the fixed one (utils/qmri_utils.py:82-136), and ``--write_transforms DIR`` saves them where
``--transforms`` reads them.  ``--register_echoes`` registers every merged echo onto the first one and resamples it
(:376-383).  Each echo is reconstructed once: the reference runs its loop body for each of the three rows of an echo and
writes the same file three times.

``--atlas_labels --atlas_template FILE --atlas NAME=FILE ...`` stands for the reference's extract_brain and
build_jhu_ho_labels (utils/qmri_utils.py:953-974, :1011-1037) without FSL: per (sub, ses) the first echo's recon_1mm
volume is masked by its recon_1mm_mask (``recon_1mm_bet``), the template is registered onto it on the GPU
(``t2map.atlas.atlas_labels``: 12 degrees of freedom, correlation ratio; not flirt, parity unpinned) and written on the subject's
grid as ``recon_1mm_mni152``, every atlas as ``recon_1mm_<NAME>`` -- the name ``cli.py --roi_stats NAME`` opens.
With ``--tissue_atlas FILE`` a tissue-label image on the template's grid follows the same transform and is refined on the
subject's echoes by expectation-maximisation on the GPU (``t2map.seg``), in place of the reference's SynthSeg steps 4 to 6
(utils/qmri_utils.py:424-466, :976-1009; another method, parity impossible to pin); the labels are written as
``recon_1mm_feta``, which ``cli.py --roi_stats feta`` and the tissue erosion read.

``--register_to_lf`` (``--hf --in_vivo``) stands for the reference's register_high_to_low_field (utils/qmri_utils.py:1039-1051,
step 3bis of run_qmri_reconstruction.py): every 1.5 T recon_1mm volume is registered rigidly (Mattes mutual information) onto
the 0.55 T one of the same subject -- the same path with ``ses-01`` and ``te-114`` --, resampled onto that grid and written
back over itself.  The 0.55 T data must have been processed first.

``--n4`` stands for the reference's run_biasfield_correction2 (utils/qmri_utils.py:296-357) without SimpleITK's N4 filter:
per (sub, ses) and orientation one log bias field is estimated on the raw stack of one echo (``--n4_echo MS``; default the
255 ms echo when present, else the first) on the GPU (``t2map.bias.n4_correct``; full width 0.25 for cor, 0.5 for ax and sag
as the reference sets them; parity with ITK unpinned), inside the stack's ``<run>_T2w_mask`` file under the derivative
directory ``mask`` when it exists, else inside ``build_mask`` of the stack, and every echo's stack of that orientation is
divided by that one field before step 1 -- the decay curve keeps its shape.  ``--write_n4`` writes the corrected stacks under
the derivative directory ``n4``.  The reference takes both directory names as arguments and never fixes them: ``mask`` and
``n4`` are this driver's choice.

``--unring`` (no reference counterpart) removes the Gibbs ringing of every raw stack of every echo on the GPU
(``t2map.unring.unring_volume``: local sub-voxel shifts, Kellner et al. 2016) before ``--n4`` and step 1.  A stack arrives
as ``(Z, Y, X)`` with Z the slice index whatever its orientation, so the acquired plane, which is what gets filtered, is
always (Y, X).  The stacks stop being integers: the pixel type is treated as under ``--n4``.  ``--write_unring`` writes them
under the derivative directory ``unring``.

``--mask_keep_largest K`` / ``--mask_min_size N`` (no reference counterpart) clean every mask that ``build_mask`` makes
here -- the registrations' and, without a mask file, the N4's -- of islands on the GPU (``t2map.components``).
``--phantom_find_seeds FILE.json`` (with ``--phantom_masks``) proposes the seeds of ``--phantom_seeds`` from the connected
components of an intensity window of the first echo's reconstruction (:func:`process_find_seeds`)."""
from __future__ import annotations

import argparse
import json
import os
import re
import sys
import time

import numpy as np

from . import _morph, _resample, _sr, t2map
from .cli import (_sitk, build_phantom_subject, feta_dirname, get_img_path, load_seeds, mask_dirname, phantom_labels_dirname, recon_dirname,
                  set_metadata)

in_dirname = "anat"
resamp_dirname = "resamp_1mm"
n4_dirname = "n4"             # --write_n4: the corrected stacks (a choice: the reference passes the name in)
unring_dirname = "unring"     # --write_unring: the unrung stacks, <sub>_<ses>_<run>_T2w_unring.nii.gz
stack_mask_dirname = "mask"   # --n4: <sub>_<ses>_<run>_T2w_mask.nii.gz of an acquired stack, when there is one
N4_DEFAULTS = {"fwhm_cor": 0.25, "fwhm": 0.5, "echo": None, "scale": 1.0}
N4_ECHO_MS = 255


def transform_path(transforms_dir, acq, orientation, echo=False):
    """``<DIR>/<sub>_<ses>_<orientation>.txt``: the rigid transform of moving stack `orientation` of this (sub, ses);
    with ``echo`` ``<DIR>/<sub>_<ses>_te-<ms>_<orientation>.txt``: that of this echo alone."""
    te = f"te-{int(round(acq['EchoTime'] * 1000))}_" if echo else ""
    return os.path.join(transforms_dir, f"{acq['sub']}_{acq['ses']}_{te}{orientation}.txt")


def load_transforms(transforms_dir, acq, fixed):
    """{moving orientation: 4 x 4} for the files that exist under `transforms_dir` (None: no directory given); the file
    of the echo of `acq`, if there is one, goes before the file of the (sub, ses)."""
    out = {}
    if not transforms_dir:
        return out
    for o in _resample.moving_order(fixed):
        own = [transform_path(transforms_dir, acq, o, echo=True)] if "EchoTime" in acq else []
        for path in own + [transform_path(transforms_dir, acq, o)]:
            if os.path.exists(path):
                m = np.loadtxt(path, dtype=np.float64)
                if m.shape != (4, 4) or not np.all(np.isfinite(m)):
                    raise ValueError(f"{path}: expected a finite 4 x 4 matrix")
                out[o] = m
                break
    return out


def save_transforms(transforms_dir, acq, transforms):
    """Write {orientation: 4 x 4} of the echo of `acq` where :func:`load_transforms` reads it, digits enough for the
    float64 to come back bit for bit.  Returns the paths."""
    os.makedirs(transforms_dir, exist_ok=True)
    paths = []
    for o, m in transforms.items():
        paths.append(transform_path(transforms_dir, acq, o, echo=True))
        np.savetxt(paths[-1], np.asarray(m, np.float64), fmt="%.17g")
    return paths


def slice_transforms_path(transforms_dir, acq, orientation, echo=False):
    """:func:`transform_path` with ``_slices`` before the extension: the rigid pose of every slice of stack `orientation`."""
    return transform_path(transforms_dir, acq, orientation, echo)[:-len(".txt")] + "_slices.txt"


def load_slice_transforms(transforms_dir, acq, geoms, fixed="ax"):
    """{orientation: (lz, 4, 4)} for the files that exist under `transforms_dir` (None: no directory given), the fixed stack
    included; lookup order as :func:`load_transforms`.  A file holds ``lz`` rows of 16 numbers, the 4 x 4 (fixed point ->
    stack point) of each slice row-major; another row count than the stack's slice count is an error naming the file."""
    out = {}
    if not transforms_dir:
        return out
    for o in [fixed] + _resample.moving_order(fixed):
        if o not in geoms:
            continue
        own = [slice_transforms_path(transforms_dir, acq, o, echo=True)] if "EchoTime" in acq else []
        for path in own + [slice_transforms_path(transforms_dir, acq, o)]:
            if os.path.exists(path):
                m = np.atleast_2d(np.loadtxt(path, dtype=np.float64))
                lz = int(_resample.as_geometry(geoms[o]).GetSize()[2])
                if m.ndim != 2 or m.shape[1] != 16 or not np.all(np.isfinite(m)):
                    raise ValueError(f"{path}: expected rows of 16 finite numbers (a 4 x 4 per slice, row-major)")
                if m.shape[0] != lz:
                    raise ValueError(f"{path}: {m.shape[0]} rows, but stack {o!r} has {lz} slices")
                out[o] = m.reshape(lz, 4, 4)
                break
    return out


def save_slice_transforms(transforms_dir, acq, slice_transforms):
    """Write {orientation: (lz, 4, 4)} of the echo of `acq` where :func:`load_slice_transforms` reads it, one row of 16
    numbers per slice, digits enough for the float64 to come back bit for bit.  Returns the paths."""
    os.makedirs(transforms_dir, exist_ok=True)
    paths = []
    for o, m in slice_transforms.items():
        m = np.asarray(m, np.float64)
        if m.ndim != 3 or m.shape[1:] != (4, 4):
            raise ValueError(f"slice transforms of {o!r} must be (lz, 4, 4), got shape {m.shape}")
        paths.append(slice_transforms_path(transforms_dir, acq, o, echo=True))
        np.savetxt(paths[-1], m.reshape(len(m), 16), fmt="%.17g")
    return paths


def _clean_args(mask_clean):
    """The keyword that hands ``mask_clean`` down; none without it, so that a run without the flags makes the calls it made."""
    return {"mask_clean": mask_clean} if mask_clean else {}


def cleaned_masks(fixed, moving, mask_clean, device=0):
    """The ``fixed_mask`` / ``moving_mask`` keywords of a registration under ``--mask_keep_largest`` / ``--mask_min_size``
    (`mask_clean`: the keywords of ``t2map.build_mask``); none without them: the registration then builds its own."""
    if not mask_clean:
        return {}
    return {"fixed_mask": t2map.build_mask(fixed, device=device, **mask_clean),
            "moving_mask": t2map.build_mask(moving, device=device, **mask_clean)}


def register_stacks(stacks, geoms, *, fixed="ax", res=1.0, integer_cast=False, mask_clean=None, device=0, **register_args):
    """{moving orientation: 4 x 4} of one echo: every stack ``(Z, Y, X)`` is resampled to its own ``res`` mm grid (stage 1)
    and each moving volume ``H_m`` is registered onto the fixed one ``H_0`` (``t2map.register.register_rigid``)."""
    order = [fixed] + _resample.moving_order(fixed)
    hi = {o: t2map.resample_volume(stacks[o], geoms[o], res=res, integer_cast=integer_cast, device=device) for o in order}
    return {o: t2map.register.register_rigid(hi[fixed][0], hi[o][0], hi[fixed][1], hi[o][1], device=device, **register_args,
                                             **cleaned_masks(hi[fixed][0], hi[o][0], mask_clean, device)).transform
            for o in order[1:]}


def _same_transforms(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[o], b[o]) for o in a)


def _metric_args(register_metric):
    """The keyword of ``register_rigid`` for ``--register_metric``: none for its default."""
    return {} if register_metric == "corr" else {"metric": register_metric}


def merge_echoes(stacks, geoms, acqs, *, fixed="ax", res=1.0, integer_cast=False, transforms_dir=None, register=False,
                 write_transforms=None, register_echoes=False, register_metric="corr", sr=None, mask_clean=None, device=0):
    """Stages 1 and 2 and the merge of the echoes of one batch (`acqs`: the fixed orientation's metadata row of every
    echo).  The transforms of an echo are read (``transforms_dir``) or found (``register``); echoes with the same
    transforms share a call, so without either the batch is one call.  ``register_echoes``: every merged echo but the
    first is registered onto the first and resampled onto it by one more single stage.  ``register_metric``: 'corr' or
    'mattes', for both.  ``sr``: None for the averaged merge, or the keyword arguments of ``t2map.sr.reconstruct_sr``
    (``--recon_method sr``: the super-resolution reconstruction, which starts from that merge and keeps the float result,
    whatever ``integer_cast`` says); its entry ``slice_transforms_dir`` (``--sr_slice_transforms``) names a directory of
    :func:`load_slice_transforms` files, read per echo and passed on as ``slice_transforms``; its entry ``estimate_slices``
    (``--sr_estimate_slices``) is the number of rounds of ``t2map.sr.reconstruct_svr``, which finds those poses on the first
    echo of each call, and ``write_slice_transforms_dir`` where they are written for every echo; its entry
    ``write_slice_weights`` (``--sr_write_slice_weights``, with ``robust``) names the CSV of :func:`save_slice_weights`.
    ``mask_clean``: see :func:`cleaned_masks`, for both registrations.  Returns ``(float32 CUDA tensor
    (n, Z, Y, X), header, transforms per echo)``."""
    import torch

    n = len(acqs)
    dev = torch.device("cuda", device)
    if register:
        stacks = {o: torch.from_numpy(np.ascontiguousarray(stacks[o], np.float32)).to(dev) for o in stacks}
        per_echo = [register_stacks({o: stacks[o][i] for o in stacks}, geoms, fixed=fixed, res=res, integer_cast=integer_cast,
                                    device=device, **_metric_args(register_metric), **_clean_args(mask_clean)) for i in range(n)]
        if write_transforms:
            for acq, t in zip(acqs, per_echo):
                save_transforms(write_transforms, acq, t)
    else:
        per_echo = [load_transforms(transforms_dir, acq, fixed) for acq in acqs]
    slices_dir = rounds = write_slices = weights_file = None
    robust_info = []
    if sr is not None:
        sr = dict(sr)
        slices_dir, rounds = sr.pop("slice_transforms_dir", None), sr.pop("estimate_slices", None)
        write_slices = sr.pop("write_slice_transforms_dir", None)
        weights_file = sr.pop("write_slice_weights", None)
        if weights_file and (rounds or not sr.get("robust")):
            raise ValueError("write_slice_weights needs robust and is not available with estimate_slices")
    per_slice = [load_slice_transforms(slices_dir, acq, geoms, fixed) for acq in acqs]
    groups = []
    for i in range(n):
        for g in groups:
            if _same_transforms(per_echo[g[0]], per_echo[i]) and _same_transforms(per_slice[g[0]], per_slice[i]):
                g.append(i)
                break
        else:
            groups.append([i])
    merged = None
    for g in groups:
        part = stacks if len(g) == n else {o: stacks[o][g] for o in stacks}
        if sr is not None and rounds:
            out, header, found = t2map.sr.reconstruct_svr(part, geoms, rounds=rounds, fixed=fixed, res=res, transforms=per_echo[g[0]],
                                                          device=device, **sr)
            for i in g if write_slices else ():
                save_slice_transforms(write_slices, acqs[i], found.transforms)
        elif sr is not None:
            poses = {"slice_transforms": per_slice[g[0]]} if slices_dir else {}
            if weights_file:
                out, header, info = t2map.sr.reconstruct_sr(part, geoms, fixed=fixed, res=res, transforms=per_echo[g[0]],
                                                            device=device, return_info=True, **sr, **poses)
                robust_info.append((g, info))
            else:
                out, header = t2map.sr.reconstruct_sr(part, geoms, fixed=fixed, res=res, transforms=per_echo[g[0]], device=device,
                                                      **sr, **poses)
        else:
            out, header = t2map.reconstruct_stacks(part, geoms, fixed=fixed, res=res, transforms=per_echo[g[0]],
                                                   integer_cast=integer_cast, device=device)
        if len(g) == n:
            merged = out
        else:
            merged = torch.empty((n,) + tuple(out.shape[1:]), dtype=out.dtype, device=out.device) if merged is None else merged
            merged[g] = out
    if weights_file and robust_info and robust_info[0][1].get("sigma2") is not None:
        order = [fixed] + [o for o in geoms if o in stacks and o != fixed]
        lz = [int(stacks[o].shape[-3]) for o in order]
        weights = [np.ones((n, k), np.float64) for k in lz]
        sums, sigma2 = np.zeros((n, sum(lz), 2), np.float64), np.zeros(n, np.float64)
        for g, info in robust_info:
            for s in range(len(order)):
                weights[s][g] = info["slice_weights"][s].cpu().numpy()
            sums[g], sigma2[g] = info["robust_sums"].cpu().numpy(), info["sigma2"].cpu().numpy()
        save_slice_weights(weights_file, order, weights, sums, sigma2)
    if register_echoes:
        grid = _resample.as_geometry(header, tuple(merged.shape[1:]))
        for i in range(1, n):
            found = t2map.register.register_rigid(merged[0], merged[i], grid, grid, device=device, **_metric_args(register_metric),
                                                  **cleaned_masks(merged[0], merged[i], mask_clean, device))
            merged[i] = t2map.resample_volume(merged[i], grid, like=grid, transform=found.transform,
                                              integer_cast=integer_cast, device=device)[0]
    return merged, header, per_echo


def echo_groups(metadata):
    """[(prj, sub, ses, [(echo time [s], {orientation: row})])] in the reference's iteration order: (prj, sub, ses),
    then EchoTime; an echo's rows are keyed by ImageOrientationPatientSTR (a later row of the same orientation replaces
    an earlier one, as the reference's dict does)."""
    out = []
    for (prj, sub, ses), sub_md in metadata.groupby(["prj", "sub", "ses"]):
        echoes = []
        for echotime, te_md in sub_md.groupby("EchoTime"):
            echoes.append((float(echotime), {acq["ImageOrientationPatientSTR"]: acq for _, acq in te_md.iterrows()}))
        out.append((prj, sub, ses, echoes))
    return out


def _same_grid(a, b):
    return (a.GetSize() == b.GetSize() and a.GetSpacing() == b.GetSpacing() and a.GetOrigin() == b.GetOrigin()
            and a.GetDirection() == b.GetDirection())


def _int16_on_disk(img, sitk):
    arr = sitk.GetArrayFromImage(img)
    return arr.dtype == np.int16


def read_echoes(sitk, bids_path, echoes, sub, ses):
    """The acquired stacks of the echoes that have the three orientations: [(echo time, rows, {orientation: image})]."""
    ready = []
    for echotime, rows in echoes:
        if not all(o in rows for o in _resample.ORIENTATIONS) or len(rows) != 3:
            print(f"Warning: TE {int(echotime * 1000):3} ms of {sub}_{ses} has orientations {sorted(rows)}. "
                  "Reconstruction is skipped.")
            continue
        imgs = {o: sitk.ReadImage(get_img_path(bids_path, rows[o], in_dirname)) for o in _resample.ORIENTATIONS}
        ready.append((echotime, rows, imgs))
    return ready


def batches_of(ready):
    """Echoes whose three stacks lie on the same grids share a call."""
    batches = []
    for item in ready:
        for batch in batches:
            if all(_same_grid(_resample.as_geometry(item[2][o]), _resample.as_geometry(batch[0][2][o]))
                   for o in _resample.ORIENTATIONS):
                batch.append(item)
                break
        else:
            batches.append([item])
    return batches


def batch_inputs(sitk, batch, integer_cast=None):
    """``(stacks, geoms, cast)`` of a batch: float32 ``(n, Z, Y, X)`` per orientation, the first echo's images as
    geometries, and whether the pixel type is kept (None: yes when every stack is int16 on disk, as the reference)."""
    geoms = {o: batch[0][2][o] for o in _resample.ORIENTATIONS}
    stacks = {o: np.stack([np.asarray(sitk.GetArrayFromImage(it[2][o]), np.float32) for it in batch])
              for o in _resample.ORIENTATIONS}
    cast = all(_int16_on_disk(it[2][o], sitk) for it in batch for o in _resample.ORIENTATIONS) \
        if integer_cast is None else bool(integer_cast)
    return stacks, geoms, cast


def n4_echo_index(echo_ms, echo=None):
    """The echo the field is estimated on: ``echo`` [ms] when given, else the 255 ms echo when present, else the first."""
    echo_ms = [int(round(float(t))) for t in echo_ms]
    if echo is not None:
        if int(echo) not in echo_ms:
            raise ValueError(f"--n4_echo {int(echo)}: the echo times are {echo_ms} ms")
        return echo_ms.index(int(echo))
    return echo_ms.index(N4_ECHO_MS) if N4_ECHO_MS in echo_ms else 0


def correct_stacks(stacks, masks, echo_ms, *, fwhm_cor=0.25, fwhm=0.5, echo=None, scale=1.0, mask_clean=None, device=0):
    """run_biasfield_correction2 on the stacks of a batch: ``stacks`` {orientation: float32 ``(n, Z, Y, X)``}, ``masks``
    {orientation: mask or None (``build_mask``)}.  Per orientation ONE log field, estimated on the echo of
    :func:`n4_echo_index`, divides every echo.  ``mask_clean``: the keywords of ``t2map.build_mask`` for a mask that is
    built (``--mask_keep_largest`` / ``--mask_min_size``).  Returns ``(corrected stacks, {orientation: log field})``."""
    at = n4_echo_index(echo_ms, echo)
    out, fields = {}, {}
    for o in _resample.ORIENTATIONS:
        mask = masks.get(o)
        if mask is None and mask_clean:
            mask = t2map.build_mask(np.asarray(stacks[o][at], np.float32), device=device, **mask_clean)
        found = t2map.bias.n4_correct(stacks[o][at], mask, fwhm=fwhm_cor if o == "cor" else fwhm, device=device)
        fields[o] = np.asarray(found.log_field, np.float32)
        out[o] = np.stack([np.asarray(t2map.bias.apply_field(v, fields[o], scale, device=device), np.float32) for v in stacks[o]])
        print(f"N4 bias field correction: {o.upper()}, TE {int(round(float(echo_ms[at])))} ms, iterations {found.iterations}")
    return out, fields


def read_stack_masks(sitk, bids_path, rows, shapes):
    """{orientation: the ``_T2w_mask`` array of the stack of `rows`, or None when there is no such file}."""
    masks = {}
    for o in _resample.ORIENTATIONS:
        path = get_img_path(bids_path, rows[o], stack_mask_dirname)
        masks[o] = None
        if os.path.isfile(path):
            masks[o] = np.asarray(sitk.GetArrayFromImage(sitk.ReadImage(path)))
            if masks[o].shape != tuple(shapes[o]):
                raise ValueError(f"--n4: {path} has shape {masks[o].shape}, the stack has {tuple(shapes[o])}")
    return masks


def n4_batch(sitk, bids_path, batch, stacks, n4, device=0, mask_clean=None):
    """The stacks of a batch after ``--n4`` (`n4`: the keyword arguments of :func:`correct_stacks`)."""
    echo_ms = [it[0] * 1000.0 for it in batch]
    at = n4_echo_index(echo_ms, n4.get("echo"))
    masks = read_stack_masks(sitk, bids_path, batch[at][1], {o: stacks[o].shape[1:] for o in _resample.ORIENTATIONS})
    return correct_stacks(stacks, masks, echo_ms, device=device, **_clean_args(mask_clean), **n4)[0]


UNRING_DEFAULTS = {"K": 20, "min_w": 1, "max_w": 3}


def unring_batch(stacks, unring, device=0):
    """The stacks of a batch after ``--unring`` (`unring`: K, min_w, max_w): every (Y, X) slice of every echo of every
    orientation, Z being the slice index of a raw stack."""
    out = {}
    for o in _resample.ORIENTATIONS:
        info = {}
        out[o] = np.asarray(t2map.unring.unring_volume(np.ascontiguousarray(stacks[o], dtype=np.float32), slice_axis=0, info=info,
                                                       device=device, **unring), np.float32)
        skipped = f", {info['skipped']} slices with non-finite samples left as they are" if info.get("skipped") else ""
        print(f"Gibbs-ringing removal: {o.upper()}, {stacks[o].shape[0]} echoes of {stacks[o].shape[1]} slices{skipped}")
    return out


def write_stacks(sitk, bids_path, batch, stacks, geoms, dirname):
    """The stacks of a batch under the derivative directory `dirname`, named after the raw stacks (:func:`get_img_path`)."""
    for o in _resample.ORIENTATIONS:
        for it, vol in zip(batch, stacks[o]):
            img = sitk.GetImageFromArray(vol)
            g = geoms[o]
            img.SetSpacing(g.GetSpacing()), img.SetOrigin(g.GetOrigin()), img.SetDirection(g.GetDirection())
            path = get_img_path(bids_path, it[1][o], dirname)
            sitk.WriteImage(img, path)
            print(f"Image saved in : {path}")


def process_recon(metadata, bids_path, *, fixed="ax", res=1.0, transforms_dir=None, write_resamp=False, denoise=True,
                  integer_cast=None, register=False, write_transforms=None, register_echoes=False, n4=None, write_n4=False,
                  register_metric="corr", sr=None, unring=None, write_unring=False, mask_clean=None, device=0):
    """Reconstruct every echo of every (prj, sub, ses) of `metadata` that has the three orientations and write it.
    The echoes of a subject whose stacks share their geometry per orientation go through one call.  ``integer_cast``:
    None keeps the pixel type as the reference does (cast when the stacks are int16 on disk).  ``register`` /
    ``write_transforms`` / ``register_echoes`` / ``register_metric``: see :func:`merge_echoes`.  ``n4``: None, or the keyword arguments of
    :func:`correct_stacks` (``--n4``): the stacks are bias-corrected before step 1 and are no longer integers, so the
    pixel type is not kept unless ``integer_cast`` says so; ``write_n4`` writes them under ``n4``.  ``sr``: see
    :func:`merge_echoes` (same file names).  ``unring``: None, or K, min_w, max_w of :func:`unring_batch` (``--unring``): the
    raw stacks are unrung first, before ``n4``, and the pixel type is treated as under ``n4``; ``write_unring`` writes them
    under ``unring``.  ``mask_clean``: None, or ``keep_largest`` / ``min_size`` of ``t2map.build_mask`` for every mask that is built
    here (the registrations', the N4's).  Returns the paths written under ``recon_1mm``."""
    import torch

    sitk = _sitk()
    written = []
    for prj, sub, ses, echoes in echo_groups(metadata):
        for batch in batches_of(read_echoes(sitk, bids_path, echoes, sub, ses)):
            t0 = time.time()
            stacks, geoms, cast = batch_inputs(sitk, batch, integer_cast)
            if unring is not None:
                stacks, cast = unring_batch(stacks, unring, device), bool(integer_cast)
                if write_unring:
                    write_stacks(sitk, bids_path, batch, stacks, geoms, unring_dirname)
            if n4 is not None:
                stacks, cast = n4_batch(sitk, bids_path, batch, stacks, n4, device, **_clean_args(mask_clean)), bool(integer_cast)
                if write_n4:
                    for o in _resample.ORIENTATIONS:
                        for it, vol in zip(batch, stacks[o]):
                            img = sitk.GetImageFromArray(vol)
                            g = geoms[o]
                            img.SetSpacing(g.GetSpacing()), img.SetOrigin(g.GetOrigin()), img.SetDirection(g.GetDirection())
                            path = get_img_path(bids_path, it[1][o], n4_dirname)
                            sitk.WriteImage(img, path)
                            print(f"Image saved in : {path}")
            print(f"===== Reconstruction: {prj}_{sub}_{ses}, TE {[int(it[0] * 1000) for it in batch]} ms, fixed {fixed}, "
                  f"transforms {'registered' if register else (transforms_dir or 'identity')} =====")
            if write_resamp:  # the intermediate volumes of step 1, as run_resample_volume leaves them
                for o in _resample.ORIENTATIONS:
                    hi, g = t2map.resample_volume(stacks[o], geoms[o], res=res, integer_cast=cast, device=device)
                    for it, vol in zip(batch, hi):
                        img = sitk.GetImageFromArray(vol)
                        img.SetSpacing(g.GetSpacing()), img.SetOrigin(g.GetOrigin()), img.SetDirection(g.GetDirection())
                        path = get_img_path(bids_path, it[1][o], resamp_dirname)
                        sitk.WriteImage(img, path)
                        print(f"Image saved in : {path}")
            merged, header, _ = merge_echoes(stacks, geoms, [it[1][fixed] for it in batch], fixed=fixed, res=res,
                                             integer_cast=cast, transforms_dir=transforms_dir, register=register,
                                             write_transforms=write_transforms, register_echoes=register_echoes,
                                             register_metric=register_metric, sr=sr, device=device, **_clean_args(mask_clean))
            if denoise:
                merged = t2map.denoise_tv(merged, out=merged)
            torch.cuda.synchronize(merged.device)
            host = merged.cpu().numpy()
            for it, vol in zip(batch, host):
                img = sitk.GetImageFromArray(vol)
                img.SetSpacing(header.GetSpacing()), img.SetOrigin(header.GetOrigin()), img.SetDirection(header.GetDirection())
                path = get_img_path(bids_path, it[1][fixed], recon_dirname)
                sitk.WriteImage(img, path)
                written.append(path)
                print(f"Image saved in : {path}")
            print(f"... done. Time to reconstruct: {round(time.time() - t0, 4)} sec")
    return written


def label_file_name(recon_name):
    """The reference names a label file ``recon_name.replace("T2w", "T2w_labels")``.  A recon_1mm name has no "T2w", which
    leaves the label under the volume's own name where the fit (``…_recon_1mm_label``) does not look for it; such a name
    gets the suffix the fit reads."""
    name = recon_name.replace("T2w", "T2w_labels")
    return name if name != recon_name else recon_name.replace(recon_dirname, phantom_labels_dirname)


def process_phantom_masks(metadata, bids_path, *, seeds=None, fixed="ax", threshold=100, close_radius=15, dilate_radius=10,
                          label_radius=6, device=0):
    """``--phantom_masks``: for every reconstructed echo volume under recon_1mm, the phantom mask (build_phantom_masks,
    utils/qmri_utils.py:591-623) under recon_1mm_mask and, with ``seeds``, the vial labels (build_phantom_labels_v2,
    :868-933) under recon_1mm_label, uint8, built on the device.  Returns the paths written."""
    sitk = _sitk()
    written = []

    def write(arr, like, path):
        img = sitk.GetImageFromArray(arr)
        img.SetSpacing(like.GetSpacing()), img.SetOrigin(like.GetOrigin()), img.SetDirection(like.GetDirection())
        sitk.WriteImage(img, path)
        written.append(path)
        print(f"Image saved in : {path}")

    for prj, sub, ses, echoes in echo_groups(metadata):
        for echotime, rows in echoes:
            acq = rows[fixed] if fixed in rows else next(iter(rows.values()))
            recon_path = get_img_path(bids_path, acq, recon_dirname).replace(" ", "")
            img = sitk.ReadImage(recon_path)
            masks, label = build_phantom_subject([sitk.GetArrayFromImage(img)], seeds or [[0, 0, 0]], threshold, close_radius,
                                                 dilate_radius, label_radius, device=device)
            name = os.path.basename(recon_path)
            mask_dir = os.path.dirname(get_img_path(bids_path, acq, mask_dirname))
            write(masks[0], img, os.path.join(mask_dir, name.replace(recon_dirname, recon_dirname + "_mask")))
            if seeds:
                label_dir = os.path.dirname(get_img_path(bids_path, acq, phantom_labels_dirname))
                write(label, img, os.path.join(label_dir, label_file_name(name)))
    return written


def seeds_file_name(path, sub, ses, several):
    """The file ``--phantom_find_seeds`` writes: `path`, or with several subjects `path` with ``_<sub>_<ses>`` before its
    extension."""
    if not several:
        return path
    root, ext = os.path.splitext(path)
    return f"{root}_{sub}_{ses}{ext}"


def process_find_seeds(metadata, bids_path, path, *, window, erode=2, size=(1, 0), fixed="ax", device=0):
    """``--phantom_find_seeds FILE``: per subject, the vials of the first echo's recon_1mm volume as connected components
    -- ``window[0] <= volume <= window[1]``, eroded by the ball of radius ``erode``, labelled (6 neighbours), the sizes
    ``size[0]..size[1]`` kept (0: no upper limit) -- and their centroids as the JSON list of ``[x, y, z]`` that
    ``--phantom_seeds`` reads, in label order.  A proposal: nothing is labelled here, and which vial is which is the
    user's to check.  Returns the paths written."""
    sitk = _sitk()
    groups = echo_groups(metadata)
    written = []
    for prj, sub, ses, echoes in groups:
        rows = echoes[0][1]
        acq = rows[fixed] if fixed in rows else next(iter(rows.values()))
        recon_path = get_img_path(bids_path, acq, recon_dirname).replace(" ", "")
        vol = np.asarray(sitk.GetArrayFromImage(sitk.ReadImage(recon_path)), np.float32)
        m = t2map.binary_threshold(vol, window[0], window[1], device=device)
        if erode > 0:
            m = t2map.binary_erode(m, _morph.ball(erode), out=m, device=device)
        seeds = t2map.components.seeds(m, 1, size[0], size[1], device=device)
        if not 1 <= len(seeds) <= 255:
            raise ValueError(f"--phantom_find_seeds: {len(seeds)} components of {recon_path} lie in the window {window[0]:g}..{window[1]:g} "
                             f"with a size in {size[0]}..{size[1] or 'inf'} after the erosion; --phantom_seeds takes 1..255")
        out = seeds_file_name(path, sub, ses, len(groups) > 1)
        with open(out, "w") as f:
            json.dump(seeds, f)
        written.append(out)
        print(f"Vial seeds proposed: {len(seeds)} from {recon_path} -> {out}")
    return written


atlas_bet_dirname = recon_dirname + "_bet"
atlas_template_dirname = recon_dirname + "_mni152"


def parse_atlas_spec(spec):
    """``--atlas NAME=FILE`` -> ``(NAME, FILE)``; NAME becomes part of ``recon_1mm_<NAME>`` and is held to the letters,
    digits and '-' that ``--roi_stats NAME`` takes."""
    name, sep, path = str(spec).partition("=")
    if not sep or not path:
        raise ValueError(f"--atlas {spec!r}: expected NAME=FILE")
    if not name or not all(ch.isalnum() or ch == "-" for ch in name):
        raise ValueError(f"--atlas {spec!r}: NAME must be made of letters, digits and '-'")
    if name in ("bet", "mni152", "mask", "label", "feta"):
        raise ValueError(f"--atlas {spec!r}: recon_1mm_{name} is another image's name")
    return name, path


LF_SESSION, LF_ECHO = "ses-01", "te-114"          # the 0.55 T volume every 1.5 T one is registered onto
LF_EXCLUDED = (("sub-003", 299), ("sub-004", 299))  # (sub, echo time [ms]) the reference leaves where they are


def low_field_path(high_path):
    """The fixed image of ``--register_to_lf``: the same path with ``ses-NN`` -> ``ses-01`` and ``te-N`` -> ``te-114``."""
    return re.sub(r"te-\d+", LF_ECHO, re.sub(r"ses-\d{2}", LF_SESSION, high_path))


def process_register_to_lf(metadata, bids_path, *, write_transforms=None, device=0):
    """``--register_to_lf``: every high-field recon_1mm volume of `metadata` is registered rigidly onto its low-field
    counterpart (:func:`low_field_path`) with Mattes mutual information, resampled linearly onto that grid and written over
    the moving file, as the reference's register_high_to_low_field does.  A volume whose counterpart is missing is
    skipped with a line; ``write_transforms``: the 4 x 4 (fixed point -> moving point) goes there as
    ``<sub>_<ses>_te-<ms>_<orientation>_to_lf.txt``.  Returns the paths written."""
    sitk = _sitk()
    written = []
    for (prj, sub, ses, echotime), sub_md in metadata.groupby(["prj", "sub", "ses", "EchoTime"]):
        for _, acq in sub_md.iterrows():
            if (sub, int(round(float(echotime) * 1000))) in LF_EXCLUDED:
                continue
            moving_path = get_img_path(bids_path, acq, recon_dirname).replace(" ", "")
            fixed_path = low_field_path(moving_path)
            if not (os.path.isfile(fixed_path) and os.path.isfile(moving_path)):
                print(f"Warning: {fixed_path if os.path.isfile(moving_path) else moving_path} does not exist. "
                      f"Registration of {os.path.basename(moving_path)} to the low field is skipped.")
                continue
            t0 = time.time()
            fixed_img, moving_img = sitk.ReadImage(fixed_path), sitk.ReadImage(moving_path)
            fixed = np.asarray(sitk.GetArrayFromImage(fixed_img), np.float32)
            moving = np.asarray(sitk.GetArrayFromImage(moving_img), np.float32)
            found = t2map.register.register_rigid(fixed, moving, fixed_img, moving_img, metric="mattes", device=device)
            out = t2map.resample_volume(moving, moving_img, like=_resample.as_geometry(fixed_img, fixed.shape),
                                        transform=found.transform, device=device)[0]
            img = sitk.GetImageFromArray(np.asarray(out, np.float32))
            img.SetSpacing(fixed_img.GetSpacing()), img.SetOrigin(fixed_img.GetOrigin()), img.SetDirection(fixed_img.GetDirection())
            sitk.WriteImage(img, moving_path)
            written.append(moving_path)
            if write_transforms:
                os.makedirs(write_transforms, exist_ok=True)
                path = transform_path(write_transforms, acq, acq["ImageOrientationPatientSTR"], echo=True).replace(".txt", "_to_lf.txt")
                np.savetxt(path, found.transform, fmt="%.17g")
                written.append(path)
            print(f"Image saved in : {moving_path}")
            print(f"... registered to the low field: -MI {found.metric:.4f}, iterations {found.iterations}, "
                  f"{round(time.time() - t0, 4)} sec")
    return written


TISSUE_DEFAULT_CLASSES = (1, 2, 3, 4, 5, 6, 7)  # the FeTA values
tissue_prior_dirname = feta_dirname + "_prior"


def parse_tissue_classes(text):
    """``--tissue_classes 1,2,...`` -> a tuple of at least 2 distinct positive label values."""
    try:
        values = tuple(int(v) for v in str(text).split(","))
    except ValueError:
        raise ValueError(f"--tissue_classes {text!r}: expected integers separated by commas") from None
    if len(values) < 2:
        raise ValueError(f"--tissue_classes {text!r}: a segmentation needs at least 2 classes")
    if len(values) > 8 or len(set(values)) != len(values) or min(values) < 1:
        raise ValueError(f"--tissue_classes {text!r}: at most 8 distinct values >= 1")
    return values


def tissue_echo_rows(echoes, wanted_ms):
    """The rows of the echoes [ms] the tissue segmentation reads, in the order asked for, out of ``echo_groups``' list of
    one (sub, ses); None: the first echo.  An echo that is not among the reconstructed ones raises."""
    if wanted_ms is None:
        return [echoes[0][1]]
    by_ms = {int(round(te * 1000)): rows for te, rows in echoes}
    missing = [ms for ms in wanted_ms if ms not in by_ms]
    if missing:
        raise ValueError(f"--tissue_echoes: no echo of {missing[0]} ms is reconstructed (there are {', '.join(map(str, sorted(by_ms)))} ms)")
    return [by_ms[ms] for ms in wanted_ms]


def process_atlas_labels(metadata, bids_path, template_path, atlas_specs, *, fixed="ax", dof=12, bins=32, metric="cr", tissue=None,
                         nonrigid=None, write_warp=False, device=0):  # noqa: A002
    """``--atlas_labels``: for every (sub, ses), from the first echo's recon_1mm volume and recon_1mm_mask: the masked volume
    under recon_1mm_bet, the registered template under recon_1mm_mni152 with the 4 x 4 transform beside it (``.txt``:
    subject point -> template point, LPS millimetres, the text form of --write_transforms; not FSL's convention), and
    every atlas (int32, nearest neighbour) under recon_1mm_<NAME>.  ``metric``: 'cr' or 'mattes'.

    ``tissue`` (``--tissue_atlas``): a dict with ``path`` (a tissue-label image on the template's grid), ``classes``,
    ``echoes`` (echo times [ms], None: the first echo) and optionally ``sigma``, ``beta``, ``n_iter``, ``write_prior``.  The
    tissue atlas follows the same transform and is refined on the recon_1mm volumes of those echoes by expectation-
    maximisation (``t2map.atlas.atlas_labels(tissue=...)``); the result goes, int32, under recon_1mm_feta, which
    ``cli.py --roi_stats feta`` reads, and with ``write_prior`` the propagated, unrefined labels under recon_1mm_feta_prior.

    ``nonrigid`` (``--atlas_nonrigid``): None, True or a dict, ``t2map.atlas.atlas_labels(nonrigid=...)``: a B-spline free-form
    deformation after the affine carries the template and the atlases; the transform text file still holds the affine.
    ``write_warp`` (``--write_atlas_warp``): the affine and the lattice go beside it as ``.npz`` (``transform`` 4 x 4,
    ``lattice`` float64 ``(3, c, c, c)`` in voxels of the subject's grid, ``min_jacobian``, ``n_folded``).
    Returns the paths written."""
    sitk = _sitk()
    template_img = sitk.ReadImage(template_path)
    template = np.asarray(sitk.GetArrayFromImage(template_img), np.float32)

    def read_labels(flag, path):
        img = sitk.ReadImage(path)
        arr = np.asarray(sitk.GetArrayFromImage(img))
        if arr.shape != template.shape or any(getattr(img, get)() != getattr(template_img, get)()
                                              for get in ("GetSpacing", "GetOrigin", "GetDirection")):
            raise ValueError(f"{flag}={path}: the atlas does not lie on the template's grid")
        return (arr if arr.dtype.kind in "iu" else np.rint(arr)).astype(np.int32)

    atlases = {name: read_labels(f"--atlas {name}", path) for name, path in atlas_specs}
    tissue_labels = None if tissue is None else read_labels("--tissue_atlas ", tissue["path"])
    written = []

    def write(arr, like, path):
        img = sitk.GetImageFromArray(arr)
        img.SetSpacing(like.GetSpacing()), img.SetOrigin(like.GetOrigin()), img.SetDirection(like.GetDirection())
        sitk.WriteImage(img, path)
        written.append(path)
        print(f"Image saved in : {path}")

    for prj, sub, ses, echoes in echo_groups(metadata):
        rows = echoes[0][1]
        acq = rows[fixed] if fixed in rows else next(iter(rows.values()))
        recon_path = get_img_path(bids_path, acq, recon_dirname).replace(" ", "")
        mask_path = get_img_path(bids_path, acq, mask_dirname).replace(" ", "")
        img = sitk.ReadImage(recon_path)
        mask = np.asarray(sitk.GetArrayFromImage(sitk.ReadImage(mask_path)))
        t0 = time.time()
        subject = np.asarray(sitk.GetArrayFromImage(img), np.float32)
        more = {} if metric == "cr" else {"metric": metric}
        if nonrigid is not None:
            more["nonrigid"] = nonrigid
        if tissue is not None:
            channels = []
            for ch_rows in tissue_echo_rows(echoes, tissue.get("echoes")):
                ch_acq = ch_rows[fixed] if fixed in ch_rows else next(iter(ch_rows.values()))
                ch = np.asarray(sitk.GetArrayFromImage(sitk.ReadImage(get_img_path(bids_path, ch_acq, recon_dirname).replace(" ", ""))),
                                np.float32)
                if ch.shape != subject.shape:
                    raise ValueError(f"--tissue_echoes: the echoes of {sub}_{ses} do not share a grid")
                channels.append(ch)
            more["tissue"] = {"labels": tissue_labels, "classes": tissue["classes"], "channels": np.stack(channels),
                              **{k: tissue[k] for k in ("sigma", "beta", "n_iter", "min_island") if tissue.get(k) is not None}}
        warped, labels, found, *refined = t2map.atlas.atlas_labels(subject, img, template, template_img, atlases, mask=mask, dof=dof,
                                                             bins=bins, device=device, **more)
        write(t2map.atlas.extract_brain(subject, mask), img, get_img_path(bids_path, acq, atlas_bet_dirname).replace(" ", ""))
        template_out = get_img_path(bids_path, acq, atlas_template_dirname).replace(" ", "")
        write(warped, img, template_out)
        np.savetxt(template_out.replace(".nii.gz", ".txt"), found.transform, fmt="%.17g")
        written.append(template_out.replace(".nii.gz", ".txt"))
        if nonrigid is not None and write_warp:
            np.savez(template_out.replace(".nii.gz", ".npz"), transform=found.transform, lattice=found.lattice,
                     min_jacobian=found.min_jacobian, n_folded=found.n_folded)
            written.append(template_out.replace(".nii.gz", ".npz"))
        for name, lab in labels.items():
            write(lab, img, get_img_path(bids_path, acq, recon_dirname + "_" + name).replace(" ", ""))
        if refined:
            write(np.asarray(refined[0]["labels"], np.int32), img, get_img_path(bids_path, acq, feta_dirname).replace(" ", ""))
            if tissue.get("write_prior"):
                write(np.asarray(refined[0]["propagated"], np.int32), img, get_img_path(bids_path, acq, tissue_prior_dirname).replace(" ", ""))
            dead = [int(c) for c, d in zip(tissue["classes"], refined[0]["model"].dead) if d]
            print(f"... tissue labels of {sub}_{ses}: {refined[0]['n_iter']} EM iterations over {len(channels)} echo(es)"
                  + (f", classes without voxels: {dead}" if dead else ""))
        affine = found if nonrigid is None else found.affine
        warp_note = "" if nonrigid is None else (f"non-rigid side {found.side}, cost {found.cost:.4f}, iterations {found.iterations}, "
                                                 f"min det J {found.min_jacobian:.4f}, folded {found.n_folded}, ")
        print(f"... atlas labels of {sub}_{ses}: {'CR' if metric == 'cr' else '-MI'} {affine.metric:.4f}, iterations {affine.iterations}, "
              f"{warp_note}{round(time.time() - t0, 4)} sec")
    return written


def reconstruct_subject(sitk, bids_path, sub_md, sub, ses, *, fixed="ax", res=1.0, transforms_dir=None, integer_cast=None,
                        register=False, register_echoes=False, n4=None, register_metric="corr", sr=None, unring=None, device=0):
    """cli.py --reconstruct: the echoes of one (sub, ses) (`sub_md`: its metadata rows) reconstructed in memory.  Every
    echo must have the three orientations and the echoes must share their grids.  ``n4``, ``sr``, ``unring``: as
    :func:`process_recon`.
    Returns ``(volumes: list of (Z, Y, X) float32 arrays in EchoTime order, header)``."""
    echoes = [(float(te), {acq["ImageOrientationPatientSTR"]: acq for _, acq in te_md.iterrows()})
              for te, te_md in sub_md.groupby("EchoTime")]
    ready = read_echoes(sitk, bids_path, echoes, sub, ses)
    if len(ready) != len(echoes):
        raise ValueError(f"--reconstruct: {sub}_{ses} lacks an orientation (ax, cor, sag) at one or more echo times")
    batches = batches_of(ready)
    if len(batches) != 1:
        raise ValueError(f"--reconstruct: the stacks of {sub}_{ses} do not lie on the same grids at every echo time")
    stacks, geoms, cast = batch_inputs(sitk, batches[0], integer_cast)
    if unring is not None:
        stacks, cast = unring_batch(stacks, unring, device), bool(integer_cast)
    if n4 is not None:
        stacks, cast = n4_batch(sitk, bids_path, batches[0], stacks, n4, device), bool(integer_cast)
    merged, header, _ = merge_echoes(stacks, geoms, [it[1][fixed] for it in ready], fixed=fixed, res=res, integer_cast=cast,
                                     transforms_dir=transforms_dir, register=register, register_echoes=register_echoes,
                                     register_metric=register_metric, sr=sr, device=device)
    host = merged.cpu().numpy()
    return [host[i] for i in range(host.shape[0])], header


SR_FLAGS = ("sr_weight", "sr_iter", "sr_profile", "sr_thickness", "sr_slice_transforms", "sr_estimate_slices",
            "sr_write_slice_transforms", "sr_robust", "sr_robust_slice", "sr_robust_huber", "sr_write_slice_weights", "sr_tv")
SLICE_WEIGHT_COLUMNS = ("stack", "slice", "echo", "weight", "count", "mean_square_residual")


def save_slice_weights(path, order, weights, sums, sigma2):
    """The slice weights of a robust reconstruction as CSV: a row (stack, slice, echo, weight, count, mean square residual)
    per slice and echo, then a line ``sigma,<echo>,<sigma>`` per echo.  ``weights``: per stack of ``order`` ``(n, lz)``;
    ``sums``: ``(n, n_slices, 2)`` count and sum of squares, stack-major; ``sigma2``: ``(n,)``.  Numbers are written with
    ``repr``, so reading them back gives the same float64."""
    n = len(sigma2)
    lines = [",".join(SLICE_WEIGHT_COLUMNS)]
    k0 = 0
    for o, w in zip(order, weights):
        for k in range(w.shape[1]):
            for e in range(n):
                c, q2 = float(sums[e, k0 + k, 0]), float(sums[e, k0 + k, 1])
                lines.append(f"{o},{k},{e},{float(w[e, k])!r},{int(c)},{(q2 / c if c > 0 else 0.0)!r}")
        k0 += w.shape[1]
    lines += [f"sigma,{e},{float(np.sqrt(sigma2[e]))!r}" for e in range(n)]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def load_slice_weights(path):
    """``(rows, sigma)`` of a :func:`save_slice_weights` file: ``rows`` a list of ``(stack, slice, echo, weight, count, mean
    square residual)``, ``sigma`` ``{echo: sigma}``."""
    rows, sigma = [], {}
    with open(path) as f:
        header = f.readline().strip().split(",")
        if tuple(header) != SLICE_WEIGHT_COLUMNS:
            raise ValueError(f"{path}: expected the columns {SLICE_WEIGHT_COLUMNS}, got {header}")
        for line in f:
            v = line.strip().split(",")
            if v[0] == "sigma" and len(v) == 3:
                sigma[int(v[1])] = float(v[2])
            elif len(v) == 6:
                rows.append((v[0], int(v[1]), int(v[2]), float(v[3]), int(v[4]), float(v[5])))
            elif line.strip():
                raise ValueError(f"{path}: cannot read the line {line.strip()!r}")
    return rows, sigma


def add_sr_arguments(p, prefix):
    """``--recon_method`` and the ``--sr_*`` flags (cli.py gives them the prefix ``recon_``)."""
    p.add_argument("--recon_method", choices=["average", "sr"], default="average",
                   help="average: resample every stack to the grid and average them (default, the reference's); sr: the "
                        "TV-regularised super-resolution reconstruction, which models every thick slice as the slice-profile "
                        "average of the 1 mm volume and inverts that model, starting from the average")
    p.add_argument(f"--{prefix}sr_weight", type=float, default=_sr.DEFAULT_WEIGHT,
                   help=f"sr: weight of the total variation, in intensity units (default {_sr.DEFAULT_WEIGHT}; 0: plain "
                        "iterative back-projection)")
    p.add_argument(f"--{prefix}sr_iter", type=int, default=_sr.DEFAULT_N_ITER,
                   help=f"sr: proximal-gradient iterations (default {_sr.DEFAULT_N_ITER})")
    p.add_argument(f"--{prefix}sr_tv", choices=["channel", "joint"], default="channel",
                   help="sr: the total variation of every echo on its own (channel, default), or joint: vector-valued TV across "
                        "the echoes, one gradient norm per voxel, so the echoes of the volume share one edge set (the weight is "
                        "not rescaled by the echo count)")
    p.add_argument(f"--{prefix}sr_profile", choices=sorted(_sr.PROFILES), default="box",
                   help="sr: slice profile, box or a cubic B-spline of that full width at half maximum (default box)")
    p.add_argument(f"--{prefix}sr_thickness", type=float, default=None, metavar="MM",
                   help="sr: slice thickness [mm] (default: each stack's slice spacing)")
    p.add_argument(f"--{prefix}sr_slice_transforms", default=None, metavar="DIR",
                   help="sr: a rigid pose per slice, for stacks of a subject that moved between slices: "
                        "<DIR>/<sub>_<ses>_[te-<ms>_]<orientation>_slices.txt with one row of 16 numbers per slice, the 4 x 4 "
                        "(fixed point -> stack point, LPS millimetres) row-major; stacks without a file keep their stack transform")
    p.add_argument(f"--{prefix}sr_estimate_slices", type=int, default=None, metavar="ROUNDS",
                   help="sr: find the pose of every slice instead of reading it: ROUNDS times, register every slice of every "
                        f"stack onto the current volume and reconstruct again with the poses found (not with --{prefix}sr_slice_transforms)")
    p.add_argument(f"--{prefix}sr_write_slice_transforms", default=None, metavar="DIR",
                   help=f"sr: write the poses --{prefix}sr_estimate_slices found where --{prefix}sr_slice_transforms reads them")
    p.add_argument(f"--{prefix}sr_robust", action="store_true",
                   help="sr: outlier weighting: every iteration weights each slice and each sample down by its residual, scaled by "
                        "a robust noise estimate per echo (drop-outs, stripes and misplaced slices stop writing into the volume)")
    p.add_argument(f"--{prefix}sr_robust_slice", type=float, default=None, metavar="T",
                   help=f"sr, with --{prefix}sr_robust: a slice is weighted down when its mean square residual exceeds T^2 sigma^2 "
                        f"(default {_sr.ROBUST_DEFAULTS['slice_threshold']})")
    p.add_argument(f"--{prefix}sr_robust_huber", type=float, default=None, metavar="H",
                   help=f"sr, with --{prefix}sr_robust: a sample is weighted down when its residual exceeds H sigma "
                        f"(default {_sr.ROBUST_DEFAULTS['huber']})")
    p.add_argument(f"--{prefix}sr_write_slice_weights", default=None, metavar="FILE.csv",
                   help=f"sr, with --{prefix}sr_robust: write the slice weights of the last iteration (stack, slice, echo, weight, "
                        "count, mean square residual; then sigma per echo)")


def sr_arguments(p, args, prefix, argv):
    """None for ``--recon_method average`` (an ``sr`` flag is then an error), else the keyword arguments of reconstruct_sr."""
    given = [f"--{prefix}{f}" for f in SR_FLAGS
             if any(a == f"--{prefix}{f}" or a.startswith(f"--{prefix}{f}=") for a in (argv if argv is not None else sys.argv[1:]))]
    if args.recon_method != "sr":
        if given:
            p.error(f"{given[0]} has no effect without --recon_method sr")
        return None
    weight, n_iter, thick = (getattr(args, f"{prefix}sr_{k}") for k in ("weight", "iter", "thickness"))
    if not (weight >= 0.0 and np.isfinite(weight)):
        p.error(f"--{prefix}sr_weight must be a finite number >= 0")
    if n_iter < 0:
        p.error(f"--{prefix}sr_iter must be >= 0")
    if thick is not None and not (thick > 0.0 and np.isfinite(thick)):
        p.error(f"--{prefix}sr_thickness must be a positive number")
    out = {"weight": weight, "n_iter": n_iter, "profile": getattr(args, f"{prefix}sr_profile"), "thickness": thick}
    if getattr(args, f"{prefix}sr_tv") == "joint":
        out["tv"] = "joint"
    slices_dir = getattr(args, f"{prefix}sr_slice_transforms")
    if slices_dir is not None:
        out["slice_transforms_dir"] = slices_dir
    rounds, write_dir = (getattr(args, f"{prefix}sr_{k}") for k in ("estimate_slices", "write_slice_transforms"))
    if rounds is not None:
        if slices_dir is not None:
            p.error(f"--{prefix}sr_estimate_slices finds the poses that --{prefix}sr_slice_transforms reads: give one of them")
        if rounds < 1:
            p.error(f"--{prefix}sr_estimate_slices must be >= 1")
        out["estimate_slices"] = rounds
    if write_dir is not None:
        if rounds is None:
            p.error(f"--{prefix}sr_write_slice_transforms needs --{prefix}sr_estimate_slices")
        out["write_slice_transforms_dir"] = write_dir
    robust, weights_file = getattr(args, f"{prefix}sr_robust"), getattr(args, f"{prefix}sr_write_slice_weights")
    tuned = {k: getattr(args, f"{prefix}sr_robust_{f}") for k, f in (("slice_threshold", "slice"), ("huber", "huber"))}
    for k, f in (("slice_threshold", "slice"), ("huber", "huber")):
        if tuned[k] is not None and not robust:
            p.error(f"--{prefix}sr_robust_{f} needs --{prefix}sr_robust")
        if tuned[k] is not None and not (tuned[k] > 0.0 and np.isfinite(tuned[k])):
            p.error(f"--{prefix}sr_robust_{f} must be a finite number > 0")
    if weights_file is not None and not robust:
        p.error(f"--{prefix}sr_write_slice_weights needs --{prefix}sr_robust")
    if weights_file is not None and rounds is not None:
        p.error(f"--{prefix}sr_write_slice_weights is not available with --{prefix}sr_estimate_slices")
    if robust:
        out["robust"] = {k: v for k, v in tuned.items() if v is not None} or True
    if weights_file is not None:
        out["write_slice_weights"] = weights_file
    return out


def parse_arguments(argv=None):
    """Flag set of run_qmri_reconstruction.py:93-112 plus what this reconstruction can be told."""
    p = argparse.ArgumentParser(prog="fetal_t2mapping_amd.recon",
                                description="resample three orthogonal stacks per echo to 1 mm and merge them on an MI355X")
    p.add_argument("--path", required=True, help="root of the qMRI tree (contains projects/ and dicom/logs/)")
    p.add_argument("--csv", nargs="+", required=True, help="metadata log CSV file name(s) under dicom/logs/, or prj-00X")
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--in_vivo", action="store_true", help="process in vivo data")
    g.add_argument("--in_vitro", action="store_true", help="process NIST phantom data")
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--lf", action="store_true", help="low-field 0.55 T data")
    g.add_argument("--hf", action="store_true", help="high-field 1.5 T data")
    p.add_argument("--fixed", choices=list(_resample.ORIENTATIONS), default="ax",
                   help="the orientation whose grid the result lies on (default ax, the reference's orient_fix_type)")
    p.add_argument("--res", type=float, default=1.0, help="isotropic resolution [mm] (default 1, the reference's high_res)")
    p.add_argument("--transforms", default=None, metavar="DIR",
                   help="directory of rigid transforms <sub>_<ses>_<orientation>.txt (4 x 4 text, fixed point -> moving "
                        "point); a missing file is the identity")
    p.add_argument("--register", action="store_true",
                   help="find the rigid transforms on the GPU: per echo, each moving 1 mm volume is registered onto the fixed "
                        "one (correlation metric, masks from build_mask, 4/2/1 pyramid; not elastix); off by default")
    p.add_argument("--write_transforms", default=None, metavar="DIR",
                   help="with --register: save the transforms as <sub>_<ses>_te-<ms>_<orientation>.txt, which --transforms reads")
    p.add_argument("--register_echoes", action="store_true",
                   help="after the merge, register every echo onto the first one and resample it; off by default")
    p.add_argument("--register_metric", choices=["corr", "mattes"], default="corr",
                   help="with --register / --register_echoes: corr = the squared correlation of registration_itk (default); "
                        "mattes = Mattes mutual information, 32 x 32 bins, the cost of elastix's default rigid map (every "
                        "voxel sampled, another descent: parity with elastix unpinned)")
    p.add_argument("--register_to_lf", action="store_true",
                   help="--hf --in_vivo: after the reconstruction, register every recon_1mm volume rigidly (Mattes mutual "
                        "information) onto the 0.55 T one of the subject (same path, ses-01, te-114), resample it onto that grid "
                        "and write it over itself (the reference's register_high_to_low_field); --write_transforms applies; "
                        "off by default")
    p.add_argument("--write_resamp", action="store_true", help="also write the 1 mm volume of every stack under resamp_1mm/")
    p.add_argument("--no_denoise", action="store_true",
                   help="skip the TV-Chambolle pass the reference applies to the merged volume (denoising=True)")
    p.add_argument("--phantom_masks", action="store_true",
                   help="--in_vitro: after the reconstruction, build the phantom mask of every echo on the GPU and write it "
                        "under recon_1mm_mask/ (the reference's build_phantom_masks); off by default")
    p.add_argument("--phantom_seeds", default=None, metavar="FILE",
                   help="with --phantom_masks: JSON list of [x, y, z] voxel indices, one per vial; the vial labels are written "
                        "under recon_1mm_label/ (the reference's build_phantom_labels_v2)")
    p.add_argument("--phantom_find_seeds", default=None, metavar="FILE.json",
                   help="with --phantom_masks: propose the seeds.  The first echo's reconstruction is thresholded into "
                        "--phantom_vial_window, eroded, split into connected components on the GPU, and the centroids of those "
                        "with a size in --phantom_vial_size are written as the JSON --phantom_seeds reads (with several subjects: "
                        "FILE_<sub>_<ses>.json).  Nothing is labelled from it in this run; check the order of the vials")
    p.add_argument("--phantom_vial_window", default=None, metavar="LO,HI",
                   help="with --phantom_find_seeds: the intensity window of the vials, both ends included (needed)")
    p.add_argument("--phantom_vial_erode", type=int, default=None, metavar="R",
                   help="with --phantom_find_seeds: radius of the ball that erodes the window's mask, 0..32 (default 2)")
    p.add_argument("--phantom_vial_size", default=None, metavar="MIN,MAX",
                   help="with --phantom_find_seeds: voxels of a vial after the erosion; MAX 0 is no upper limit (default 1,0)")
    p.add_argument("--mask_keep_largest", type=int, default=0, metavar="K",
                   help="keep the K largest connected components of every mask build_mask makes here (--register, "
                        "--register_echoes, --n4 without a mask file); 0, the default, keeps the mask as it is")
    p.add_argument("--mask_min_size", type=int, default=0, metavar="N",
                   help="drop the connected components of fewer than N voxels from every such mask; 0, the default, drops none")
    p.add_argument("--atlas_labels", action="store_true",
                   help="after the reconstruction: register --atlas_template onto the first echo's recon_1mm volume masked by "
                        "recon_1mm_mask (affine, correlation ratio, on the GPU; stands for the reference's flirt call, parity "
                        "unpinned) and write recon_1mm_bet, recon_1mm_mni152 and one recon_1mm_<NAME> per --atlas, which "
                        "cli.py --roi_stats NAME reads; the 4 x 4 transform is written beside recon_1mm_mni152 as text: "
                        "subject point -> template point in LPS millimetres, not FSL's convention; off by default")
    p.add_argument("--atlas_template", default=None, metavar="FILE", help="with --atlas_labels: the template image (MNI152 T1)")
    p.add_argument("--atlas", action="append", default=[], metavar="NAME=FILE",
                   help="with --atlas_labels: a label image on the template's grid, repeatable (ho=..., jhu=...)")
    p.add_argument("--atlas_dof", type=int, choices=[6, 7, 9, 12], default=12, help="degrees of freedom (default 12, as flirt's)")
    p.add_argument("--atlas_bins", type=int, default=32, help="bins of the correlation ratio, 1..64 (default 32)")
    p.add_argument("--atlas_metric", choices=["cr", "mattes"], default="cr",
                   help="with --atlas_labels: cr = the correlation ratio (default, flirt's cost); mattes = Mattes mutual information")
    p.add_argument("--atlas_nonrigid", action="store_true",
                   help="with --atlas_labels: after the affine, a B-spline free-form deformation under Mattes mutual information "
                        "(t2map.register.register_ffd) carries the template and the atlases; parity with elastix / NiftyReg / ANTs "
                        "is unpinned")
    p.add_argument("--atlas_nonrigid_sides", default=None, metavar="4,5,7",
                   help="with --atlas_nonrigid: the lattice side per level, from 4,5,7,11,19, never falling; the shrink factors are "
                        "the last of 4,2,1 (default 4,5,7)")
    p.add_argument("--atlas_nonrigid_weight", type=float, default=None, help="with --atlas_nonrigid: weight of the bending term (default 0.05)")
    p.add_argument("--atlas_nonrigid_iter", type=int, default=None, help="with --atlas_nonrigid: moves per level at most (default 20)")
    p.add_argument("--write_atlas_warp", action="store_true",
                   help="with --atlas_nonrigid: write the affine and the lattice as .npz beside the transform text file")
    p.add_argument("--tissue_atlas", default=None, metavar="FILE",
                   help="with --atlas_labels: a tissue-label image on the template's grid.  It follows the found transform, is "
                        "blurred into spatial priors and refined on the subject's own echoes by expectation-maximisation on the "
                        "GPU (Gaussian mixture with a Potts term; stands for the reference's SynthSeg steps, parity impossible to "
                        "pin); the labels are written under recon_1mm_feta, which cli.py --roi_stats feta reads; off by default")
    p.add_argument("--tissue_classes", default=None, metavar="1,2,...", help="with --tissue_atlas: the label values that are tissue "
                                                                             "classes, 2 .. 8 of them (default 1,2,3,4,5,6,7: FeTA's)")
    p.add_argument("--tissue_echoes", type=int, nargs="+", default=None, metavar="MS",
                   help="with --tissue_atlas: the echoes [ms] whose recon_1mm volumes are the channels, at most 4 (default: the "
                        "first echo, which the atlas registration uses)")
    p.add_argument("--tissue_sigma", type=float, default=None, help="with --tissue_atlas: blur of the priors in voxels (default 2)")
    p.add_argument("--tissue_beta", type=float, default=None, help="with --tissue_atlas: weight of the Potts term (default 0.5)")
    p.add_argument("--tissue_iter", type=int, default=None, help="with --tissue_atlas: EM iterations (default 15)")
    p.add_argument("--tissue_min_island", type=int, default=None, metavar="N",
                   help="with --tissue_atlas: islands of the tissue labels with fewer than N voxels take the class of their "
                        "surroundings (the class at the nearest voxel of a larger region; default 0: off)")
    p.add_argument("--write_tissue_prior", action="store_true",
                   help="with --tissue_atlas: also write the propagated, unrefined labels under recon_1mm_feta_prior")
    p.add_argument("--n4", action="store_true",
                   help="N4 bias-field correction of the acquired stacks on the GPU before step 1 (the reference's "
                        "run_biasfield_correction2; parity with ITK unpinned): per orientation one log field, estimated on one "
                        "echo inside the stack's <run>_T2w_mask file under derivatives/mask (else build_mask), divides every "
                        "echo; off by default")
    p.add_argument("--n4_fwhm_cor", type=float, default=N4_DEFAULTS["fwhm_cor"],
                   help="with --n4: full width at half maximum of the deconvolution for the cor stack (default 0.25)")
    p.add_argument("--n4_fwhm", type=float, default=N4_DEFAULTS["fwhm"], help="with --n4: for the ax and sag stacks (default 0.5)")
    p.add_argument("--n4_echo", type=int, default=None, metavar="MS",
                   help="with --n4: the echo [ms] the field is estimated on (default 255 when present, else the first)")
    p.add_argument("--n4_scale", type=float, default=N4_DEFAULTS["scale"],
                   help="with --n4: factor on the corrected stacks (default 1; run_biasfield_correction's 0.25 is --n4_scale 0.25)")
    p.add_argument("--write_n4", action="store_true", help="with --n4: also write the corrected stacks under derivatives/n4/")
    add_unring_arguments(p, "")
    add_sr_arguments(p, "")
    p.add_argument("--device", type=int, default=0, help="HIP device ordinal")
    args = p.parse_args(argv)
    args.sr_args = sr_arguments(p, args, "", argv)
    args.unring_args = unring_arguments(p, args, "", argv)
    given = [f for f in ("--n4_fwhm_cor", "--n4_fwhm", "--n4_echo", "--n4_scale", "--write_n4")
             if any(a == f or a.startswith(f + "=") for a in (argv if argv is not None else sys.argv[1:]))]
    if given and not args.n4:
        p.error(f"{given[0]} has no effect without --n4")
    args.n4_args = None
    if args.n4:
        if not (args.n4_fwhm_cor > 0.0 and args.n4_fwhm > 0.0 and np.isfinite(args.n4_fwhm_cor + args.n4_fwhm + args.n4_scale)):
            p.error("--n4_fwhm_cor and --n4_fwhm must be positive numbers and --n4_scale finite")
        args.n4_args = {"fwhm_cor": args.n4_fwhm_cor, "fwhm": args.n4_fwhm, "echo": args.n4_echo, "scale": args.n4_scale}
    if args.atlas_labels:
        if args.atlas_template is None or not os.path.isfile(args.atlas_template):
            p.error(f"--atlas_labels needs --atlas_template FILE, an existing image (got {args.atlas_template!r})")
        if not args.atlas:
            p.error("--atlas_labels needs at least one --atlas NAME=FILE")
        if not 1 <= args.atlas_bins <= 64:
            p.error("--atlas_bins is in 1..64")
        try:
            args.atlas_specs = [parse_atlas_spec(spec) for spec in args.atlas]
        except ValueError as e:
            p.error(str(e))
        if len({n for n, _ in args.atlas_specs}) != len(args.atlas_specs):
            p.error("--atlas: a NAME is given twice")
        for _, path in args.atlas_specs:
            if not os.path.isfile(path):
                p.error(f"--atlas: {path!r} does not exist")
    elif args.atlas_template is not None or args.atlas:
        p.error("--atlas_template / --atlas have no effect without --atlas_labels")
    tissue_flags = [f for f, v in (("--tissue_classes", args.tissue_classes), ("--tissue_echoes", args.tissue_echoes),
                                   ("--tissue_sigma", args.tissue_sigma), ("--tissue_beta", args.tissue_beta),
                                   ("--tissue_iter", args.tissue_iter), ("--tissue_min_island", args.tissue_min_island),
                                   ("--write_tissue_prior", args.write_tissue_prior or None))
                    if v is not None]
    args.tissue_args = None
    args.nonrigid_args = None
    nonrigid_flags = [f for f, v in (("--atlas_nonrigid_sides", args.atlas_nonrigid_sides), ("--atlas_nonrigid_weight", args.atlas_nonrigid_weight),
                                     ("--atlas_nonrigid_iter", args.atlas_nonrigid_iter), ("--write_atlas_warp", args.write_atlas_warp or None))
                      if v is not None]
    if args.atlas_nonrigid:
        if not args.atlas_labels:
            p.error("--atlas_nonrigid has no effect without --atlas_labels")
        args.nonrigid_args = {}
        if args.atlas_nonrigid_sides is not None:
            try:
                sides = [int(v) for v in args.atlas_nonrigid_sides.split(",")]
            except ValueError:
                p.error(f"--atlas_nonrigid_sides {args.atlas_nonrigid_sides!r}: expected integers separated by commas")
            if not 1 <= len(sides) <= 3 or any(c not in (4, 5, 7, 11, 19) for c in sides) or sorted(sides) != sides:
                p.error("--atlas_nonrigid_sides: one to three sides from 4,5,7,11,19 that never fall")
            args.nonrigid_args["schedule"] = tuple(zip((4, 2, 1)[-len(sides):], sides))
        if args.atlas_nonrigid_weight is not None:
            if not (args.atlas_nonrigid_weight >= 0.0 and np.isfinite(args.atlas_nonrigid_weight)):
                p.error("--atlas_nonrigid_weight is finite and >= 0")
            args.nonrigid_args["weight"] = args.atlas_nonrigid_weight
        if args.atlas_nonrigid_iter is not None:
            if args.atlas_nonrigid_iter < 0:
                p.error("--atlas_nonrigid_iter is >= 0")
            args.nonrigid_args["max_iter"] = args.atlas_nonrigid_iter
        args.nonrigid_args = args.nonrigid_args or True
    elif nonrigid_flags:
        p.error(f"{nonrigid_flags[0]} has no effect without --atlas_nonrigid")
    if args.tissue_atlas is not None:
        if not args.atlas_labels:
            p.error("--tissue_atlas has no effect without --atlas_labels")
        if not os.path.isfile(args.tissue_atlas):
            p.error(f"--tissue_atlas: {args.tissue_atlas!r} does not exist")
        try:
            classes = TISSUE_DEFAULT_CLASSES if args.tissue_classes is None else parse_tissue_classes(args.tissue_classes)
        except ValueError as e:
            p.error(str(e))
        if args.tissue_echoes is not None and not 1 <= len(args.tissue_echoes) <= 4:
            p.error("--tissue_echoes takes 1 .. 4 echo times")
        if args.tissue_echoes is not None and len(set(args.tissue_echoes)) != len(args.tissue_echoes):
            p.error("--tissue_echoes: an echo is given twice")
        if args.tissue_sigma is not None and not 0.0 <= args.tissue_sigma <= 8.0:
            p.error("--tissue_sigma is in 0 .. 8 voxels")
        if args.tissue_beta is not None and not (args.tissue_beta >= 0.0 and np.isfinite(args.tissue_beta)):
            p.error("--tissue_beta must be a number >= 0")
        if args.tissue_iter is not None and args.tissue_iter < 1:
            p.error("--tissue_iter must be >= 1")
        if args.tissue_min_island is not None and args.tissue_min_island < 0:
            p.error("--tissue_min_island must be >= 0")
        args.tissue_args = {"path": args.tissue_atlas, "classes": classes, "echoes": args.tissue_echoes, "sigma": args.tissue_sigma,
                            "beta": args.tissue_beta, "n_iter": args.tissue_iter, "write_prior": args.write_tissue_prior}
        if args.tissue_min_island:  # (the key is there only when the flag asks for something)
            args.tissue_args["min_island"] = args.tissue_min_island
    elif tissue_flags:
        p.error(f"{tissue_flags[0]} has no effect without --tissue_atlas")
    args.error = p.error
    if args.phantom_masks and not args.in_vitro:
        p.error("--phantom_masks goes with --in_vitro")
    if args.phantom_seeds is not None and not args.phantom_masks:
        p.error("--phantom_seeds has no effect without --phantom_masks")
    args.seeds = None
    if args.phantom_seeds is not None:
        try:
            args.seeds = load_seeds(args.phantom_seeds)
        except (OSError, ValueError) as e:
            p.error(str(e))
    vial_flags = [f for f, v in (("--phantom_vial_window", args.phantom_vial_window), ("--phantom_vial_erode", args.phantom_vial_erode),
                                 ("--phantom_vial_size", args.phantom_vial_size)) if v is not None]
    args.find_seeds = None
    if args.phantom_find_seeds is not None:
        if not args.phantom_masks:
            p.error("--phantom_find_seeds has no effect without --phantom_masks")
        if args.phantom_vial_window is None:
            p.error("--phantom_find_seeds needs --phantom_vial_window LO,HI (the intensities of the vials)")
        try:
            lo, hi = (float(v) for v in args.phantom_vial_window.split(","))
        except ValueError:
            p.error(f"--phantom_vial_window {args.phantom_vial_window!r}: expected LO,HI")
        if not lo <= hi:  # (also a NaN)
            p.error("--phantom_vial_window: LO must not be above HI")
        erode = 2 if args.phantom_vial_erode is None else args.phantom_vial_erode
        if not 0 <= erode <= 32:
            p.error("--phantom_vial_erode is in 0..32")
        try:
            smin, smax = (int(v) for v in (args.phantom_vial_size or "1,0").split(","))
        except ValueError:
            p.error(f"--phantom_vial_size {args.phantom_vial_size!r}: expected MIN,MAX")
        if smin < 1 or smax < 0 or (smax and smax < smin):
            p.error("--phantom_vial_size: MIN is at least 1 and MAX is 0 (no limit) or at least MIN")
        args.find_seeds = {"window": (lo, hi), "erode": erode, "size": (smin, smax)}
    elif vial_flags:
        p.error(f"{vial_flags[0]} has no effect without --phantom_find_seeds")
    if args.mask_keep_largest < 0 or args.mask_min_size < 0:
        p.error("--mask_keep_largest and --mask_min_size must not be negative")
    if (args.mask_keep_largest or args.mask_min_size) and not (args.register or args.register_echoes or args.n4):
        p.error("--mask_keep_largest / --mask_min_size have no effect without --register, --register_echoes or --n4")
    args.mask_clean = ({"keep_largest": args.mask_keep_largest, "min_size": args.mask_min_size}
                       if args.mask_keep_largest or args.mask_min_size else None)
    if not (args.res > 0.0 and np.isfinite(args.res)):
        p.error("--res must be a positive number")
    if args.transforms is not None and not os.path.isdir(args.transforms):
        p.error(f"--transforms {args.transforms!r} is not a directory")
    if args.transforms is not None and (args.register or args.register_echoes):
        p.error("--transforms supplies the transforms: it does not go with --register / --register_echoes, which find them")
    if args.register_to_lf and not (args.hf and args.in_vivo):
        p.error("--register_to_lf goes with --hf --in_vivo: it registers the 1.5 T volumes onto the 0.55 T ones")
    if args.write_transforms is not None and not (args.register or args.register_to_lf):
        p.error("--write_transforms has no effect without --register")
    return args


def add_unring_arguments(p, prefix):
    """``--unring`` and its sub-flags (recon.py), or ``--recon_unring`` .. (cli.py, `prefix` "recon_")."""
    with_ = f"with --{prefix}unring"
    p.add_argument(f"--{prefix}unring", action="store_true",
                   help="Gibbs-ringing removal (local sub-voxel shifts, Kellner et al. 2016) of every acquired slice of every raw "
                        "stack of every echo on the GPU, before --n4 and step 1; off by default")
    p.add_argument(f"--{prefix}unring_shifts", type=int, default=None, metavar="K",
                   help=f"{with_}: sub-voxel shifts per side, 1 .. 32 (default 20: 41 candidates)")
    p.add_argument(f"--{prefix}unring_window", default=None, metavar="MIN,MAX",
                   help=f"{with_}: the window of the total variation in samples, 1 <= MIN <= MAX <= 8 (default 1,3)")
    if not prefix:
        p.add_argument("--write_unring", action="store_true", help="with --unring: also write the unrung stacks under derivatives/unring/")


def unring_arguments(p, args, prefix, argv):
    """None without ``--unring``, else K, min_w, max_w for :func:`unring_batch`; a sub-flag without the flag is an error."""
    from ._unring import MAX_K, MAX_W

    flags = [f"--{prefix}unring_shifts", f"--{prefix}unring_window"] + ([] if prefix else ["--write_unring"])
    given = [f for f in flags if any(a == f or a.startswith(f + "=") for a in (argv if argv is not None else sys.argv[1:]))]
    on = getattr(args, f"{prefix}unring")
    if given and not on:
        p.error(f"{given[0]} has no effect without --{prefix}unring")
    if not on:
        return None
    out = dict(UNRING_DEFAULTS)
    shifts, window = getattr(args, f"{prefix}unring_shifts"), getattr(args, f"{prefix}unring_window")
    if shifts is not None:
        if not 1 <= shifts <= MAX_K:
            p.error(f"--{prefix}unring_shifts is in 1 .. {MAX_K}")
        out["K"] = shifts
    if window is not None:
        try:
            lo, hi = (int(v) for v in window.split(","))
        except ValueError:
            p.error(f"--{prefix}unring_window {window!r}: expected MIN,MAX")
        if not 1 <= lo <= hi <= MAX_W:
            p.error(f"--{prefix}unring_window: 1 <= MIN <= MAX <= {MAX_W}")
        out["min_w"], out["max_w"] = lo, hi
    return out


def main(argv=None):
    args = parse_arguments(argv)
    if not os.path.exists(args.path):
        print(f"Error: The specified path does not exist: {args.path}")
        raise SystemExit(1)
    bids_path = os.path.join(args.path, "projects/")
    csv_path = os.path.join(args.path, "dicom/logs/")
    metadata = set_metadata(csv_path, args.csv, bool(args.lf))
    if args.tissue_args is not None:
        try:
            for _, _, _, echoes in echo_groups(metadata):
                tissue_echo_rows(echoes, args.tissue_args["echoes"])
        except ValueError as e:
            args.error(str(e))
    process_recon(metadata, bids_path, fixed=args.fixed, res=args.res, transforms_dir=args.transforms,
                  write_resamp=args.write_resamp, denoise=not args.no_denoise, register=args.register,
                  write_transforms=args.write_transforms, register_echoes=args.register_echoes, n4=args.n4_args,
                  write_n4=args.write_n4, register_metric=args.register_metric, sr=args.sr_args, unring=args.unring_args,
                  write_unring=args.write_unring, mask_clean=args.mask_clean, device=args.device)
    if args.register_to_lf:
        process_register_to_lf(metadata, bids_path, write_transforms=args.write_transforms, device=args.device)
    if args.find_seeds is not None:
        try:
            process_find_seeds(metadata, bids_path, args.phantom_find_seeds, fixed=args.fixed, device=args.device, **args.find_seeds)
        except ValueError as e:
            args.error(str(e))
    if args.phantom_masks:
        process_phantom_masks(metadata, bids_path, seeds=args.seeds, fixed=args.fixed, device=args.device)
    if args.atlas_labels:
        process_atlas_labels(metadata, bids_path, args.atlas_template, args.atlas_specs, fixed=args.fixed, dof=args.atlas_dof,
                             bins=args.atlas_bins, metric=args.atlas_metric, device=args.device,
                             **({} if args.tissue_args is None else {"tissue": args.tissue_args}),
                             **({} if args.nonrigid_args is None else {"nonrigid": args.nonrigid_args, "write_warp": args.write_atlas_warp}))


if __name__ == "__main__":
    main(sys.argv[1:])
