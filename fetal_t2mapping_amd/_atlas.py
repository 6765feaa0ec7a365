"""Atlas labels on a subject's grid, restated in numpy: the statement of ``t2map.atlas.atlas_labels``.  Stands for the
reference's ``extract_brain`` (utils/qmri_utils.py:953-974: the reconstruction times its mask) and
``build_jhu_ho_labels`` (:1011-1037): FSL's flirt registers the MNI152 T1 template onto the brain-extracted T2w volume
(12 degrees of freedom, correlation ratio) and the matrix carries the JHU and Harvard-Oxford label volumes over with
nearest-neighbour interpolation.  Here the registration is :func:`_register.register_affine` -- the same cost and
transform model, another optimizer and no search: parity with flirt is not pinned."""
from __future__ import annotations

import numpy as np

from . import _ffd, _register, _resample, _seg


def extract_brain(vol, mask):
    """``sitk.Mask``: the volume where the mask is not 0, zero elsewhere (float32)."""
    vol, mask = np.asarray(vol, np.float32), np.asarray(mask)
    if vol.ndim != 3 or mask.shape != vol.shape:
        raise ValueError("extract_brain takes a (Z, Y, X) volume and a mask of its shape")
    return np.where(mask != 0, vol, np.float32(0.0))


def check_atlases(atlases, template_shape):
    """{name: int32 (Z, Y, X) on the template's grid}."""
    out = {}
    for name, lab in dict(atlases).items():
        lab = np.asarray(lab)
        if lab.shape != tuple(template_shape):
            raise ValueError(f"atlas {name!r} has shape {lab.shape}, the template {tuple(template_shape)}: they share a grid")
        if lab.dtype.kind not in "iu":
            raise ValueError(f"atlas {name!r} must have an integer dtype")
        out[str(name)] = lab.astype(np.int32)
    return out


def subject_mask(subject, mask):
    """The mask given, or -- None -- ``build_mask`` of the subject."""
    return _register.build_mask(subject) if mask is None else (np.asarray(mask) != 0).astype(np.uint8)


def atlas_labels(subject, subject_geom, template, template_geom, atlases, *, mask=None, bins=32, dof=12, levels=(4, 2, 1),
                 max_iter=100, init="centroids", metric="cr", tissue=None, nonrigid=None):
    """``(warped template float32, {name: int32 labels}, Registration)`` on the subject's grid: the brain is extracted
    (``mask``; None: ``build_mask``), the template (moving, its mask ``template > 0``) is registered onto it (fixed) with
    the correlation ratio (``metric`` 'cr') or Mattes mutual information ('mattes'), and the found transform resamples the
    template (linear) and every atlas (nearest, 0 outside).

    ``tissue``: a dict with ``labels`` (a tissue-label atlas on the template's grid), ``classes`` (its K label values),
    ``channels`` (1 .. 4 volumes of the subject, e.g. echoes) and optionally ``sigma`` (default 2 voxels) and the keywords of
    ``_seg.segment_em``.  The tissue atlas follows the found transform by nearest neighbour, is blurred into spatial priors
    and refined on the channels by expectation-maximisation inside the subject mask; a fourth value is returned, a dict
    with ``labels`` (int32), ``propagated`` (the unrefined labels), ``prior``, ``model``, ``s0_trace`` and ``n_iter``.

    ``nonrigid``: None (the affine alone), True or a dict of :func:`_ffd.register_ffd`'s keywords (``schedule``, ``weight``,
    ``max_iter``, ``max_step``, ``bins``, ``moving_bins``).  After the affine, :func:`_ffd.register_ffd` starts from it; the
    template is warped linearly and every atlas and the tissue atlas by nearest neighbour through :func:`_ffd.warp`, and the
    third value is the :class:`_ffd.FFDRegistration` (its ``transform`` is the affine's).  The affine stage keeps the
    ``metric`` the caller chose; the deformation always uses Mattes mutual information."""
    subject, template = np.asarray(subject, np.float32), np.asarray(template, np.float32)
    atlases = check_atlases(atlases, template.shape)
    if tissue is not None:
        t_labels, t_classes, t_channels, t_sigma, t_em = _seg.tissue_arguments(tissue, template.shape, subject.shape)
    fmask = subject_mask(subject, mask)
    brain = extract_brain(subject, fmask)
    sg, tg = _resample.as_geometry(subject_geom, subject.shape), _resample.as_geometry(template_geom, template.shape)
    found = _register.register_affine(brain, template, sg, tg, metric=metric, bins=bins, dof=dof, fixed_mask=fmask,
                                      moving_mask=(template > 0).astype(np.uint8), levels=levels, max_iter=max_iter, init=init)
    a = _resample.index_affine(sg, tg, found.transform)
    if nonrigid is None:
        def carry(vol, interp="linear"):
            return _resample.resample(vol, a, subject.shape, interp=interp, default=0)
    else:
        found = _ffd.register_ffd(brain, template, sg, tg, affine=found, fixed_mask=fmask, moving_mask=(template > 0).astype(np.uint8),
                                  **_ffd.nonrigid_options(nonrigid))

        def carry(vol, interp="linear"):
            return _ffd.warp(vol, a, found.lattice, subject.shape, interp=interp, default=0)
    warped = carry(template)
    labels = {n: carry(lab, "nearest") for n, lab in atlases.items()}
    if tissue is None:
        return warped, labels, found
    propagated = carry(t_labels, "nearest")
    prior = _seg.priors_from_labels(propagated, t_classes, t_sigma)
    return warped, labels, found, _seg.tissue_result(propagated, prior, _seg.segment_em(t_channels, fmask, prior, t_classes, **t_em))
