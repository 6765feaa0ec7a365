"""Atlas labels on a subject's grid with the registration's sums and the resampling on the GPU;
:mod:`fetal_t2mapping_amd._atlas` states the stage in numpy."""
import numpy as np

from . import _atlas, _ffd, _gpu_ffd, _gpu_register, _gpu_seg, _resample, _seg
from ._gpu import is_tensor, pick_device, volume
from ._gpu_morph import build_mask
from ._gpu_resample import resample_volume


def extract_brain(vol, mask, *, device=0):
    """``sitk.Mask`` (the reference's ``extract_brain``, utils/qmri_utils.py:953-974): ``vol`` where ``mask`` is not 0, zero
    elsewhere, float32.  numpy in, numpy out; a CUDA tensor in, a tensor out.  A selection, no arithmetic."""
    import torch

    if not (is_tensor(vol) or is_tensor(mask)):
        return _atlas.extract_brain(vol, mask)
    dev = pick_device((vol, mask), device)
    v, m = volume(vol, torch.float32, dev, "vol"), volume(mask, torch.uint8, dev, "mask")
    if v.shape != m.shape:
        raise ValueError("extract_brain takes a (Z, Y, X) volume and a mask of its shape")
    return torch.where(m != 0, v, torch.zeros((), dtype=torch.float32, device=dev))


def atlas_labels(subject, subject_geom, template, template_geom, atlases, *, mask=None, bins=32, dof=12, levels=(4, 2, 1),
                 max_iter=100, init="centroids", metric="cr", tissue=None, nonrigid=None, device=0):  # noqa: A002
    """The reference's ``build_jhu_ho_labels`` (utils/qmri_utils.py:1011-1037) without FSL: ``subject`` (float32
    ``(Z, Y, X)``, e.g. the first-echo reconstruction) is brain-extracted with ``mask`` (None: :func:`build_mask`), the
    ``template`` (e.g. MNI152 T1; its mask is ``template > 0``) is registered onto it by
    ``register.register_affine(metric='cr')`` with ``dof`` degrees of freedom and ``bins`` bins, and the found transform
    resamples the template (linear) and every volume of ``atlases`` ({name: integer labels on the template's grid}) with
    nearest-neighbour interpolation (t2fit_resample_dev, int32, 0 outside) onto the subject's grid.  Returns ``(warped
    template float32, {name: int32 labels}, Registration)`` as numpy arrays; ``Registration.transform`` is the 4 x 4
    (subject point -> template point, LPS mm -- not FSL's convention).  Equal to :func:`_atlas.atlas_labels`.  Parity with
    flirt is not pinned: the cost and the transform model are its, the optimizer and the (absent) search are not.
    ``metric``: 'cr', or 'mattes' for Mattes mutual information.

    ``tissue``: a dict with ``labels`` (a tissue-label atlas on the template's grid), ``classes`` (its K label values),
    ``channels`` (1 .. 4 volumes of the subject, e.g. echoes) and optionally ``sigma`` (default 2 voxels) and the keywords of
    ``seg.segment_em``.  The tissue atlas follows the found transform by nearest neighbour, is blurred into spatial priors
    (``seg.priors_from_labels``) and refined on the channels by expectation-maximisation inside the subject mask
    (``seg.segment_em``), all on the device; a fourth value is returned, a dict of numpy arrays with ``labels`` (int32),
    ``propagated`` (the unrefined labels), ``prior``, ``model``, ``s0_trace`` and ``n_iter``.  ``tissue=None`` changes nothing.

    ``nonrigid``: None (the affine alone: no new kernel runs), True or a dict of ``register.register_ffd``'s keywords
    (``schedule``, ``weight``, ``max_iter``, ``max_step``, ``bins``, ``moving_bins``).  After the affine,
    ``register.register_ffd`` starts from it: a B-spline free-form deformation on top of the affine.  The template is then
    warped linearly and every atlas and the tissue atlas by nearest neighbour through ``register.ffd_warp``
    (t2fit_ffd_warp_dev), and the third value is the :class:`_ffd.FFDRegistration` (``transform`` / ``parameters`` are the
    affine's, ``lattice``, ``min_jacobian``, ``n_folded``).  The affine stage keeps the ``metric`` the caller chose; the
    deformation always uses Mattes mutual information.  Equal to :func:`_atlas.atlas_labels` with the same keyword."""
    import torch

    dev = pick_device((subject, template, mask), device)
    template_host = template.cpu().numpy() if is_tensor(template) else np.asarray(template, np.float32)
    atlases = _atlas.check_atlases({n: (a.cpu().numpy() if is_tensor(a) else a) for n, a in dict(atlases).items()}, template_host.shape)
    s, t = volume(subject, torch.float32, dev, "subject"), volume(template, torch.float32, dev, "template")
    if tissue is not None:
        tis = {k: (v.cpu().numpy() if is_tensor(v) else v) for k, v in dict(tissue).items()}
        t_labels, t_classes, t_channels, t_sigma, t_em = _seg.tissue_arguments(tis, template_host.shape, tuple(s.shape))
    fmask = build_mask(s, device=dev.index) if mask is None else volume(mask, torch.uint8, dev, "mask")
    brain = extract_brain(s, fmask)
    sg, tg = _resample.as_geometry(subject_geom, tuple(s.shape)), _resample.as_geometry(template_geom, tuple(t.shape))
    found = _gpu_register.register_affine(brain, t, sg, tg, metric=metric, bins=bins, dof=dof, fixed_mask=fmask,
                                          moving_mask=(t > 0).to(torch.uint8), levels=levels, max_iter=max_iter, init=init,
                                          device=dev.index)
    if nonrigid is None:
        def carry(vol, interp="linear"):
            return resample_volume(vol, tg, like=sg, transform=found.transform, interp=interp, default=0)[0]
    else:
        found = _gpu_ffd.register_ffd(brain, t, sg, tg, affine=found, fixed_mask=fmask, moving_mask=(t > 0).to(torch.uint8),
                                      device=dev.index, **_ffd.nonrigid_options(nonrigid))
        a = _resample.index_affine(sg, tg, found.transform)

        def carry(vol, interp="linear"):
            return _gpu_ffd.ffd_warp(vol, a, found.lattice, tuple(s.shape), interp=interp, default=0, device=dev.index)
    warped = carry(t).cpu().numpy()
    labels = {n: carry(torch.from_numpy(lab).to(dev), "nearest").cpu().numpy() for n, lab in atlases.items()}
    if tissue is None:
        return warped, labels, found
    propagated = carry(torch.from_numpy(t_labels).to(dev), "nearest")
    prior = _gpu_seg.priors_from_labels(propagated, t_classes, t_sigma)
    res = _gpu_seg.segment_em(torch.from_numpy(t_channels).to(dev), fmask, prior, t_classes, **t_em)
    return warped, labels, found, _seg.tissue_result(propagated.cpu().numpy(), prior.cpu().numpy(),
                                                     res._replace(labels=res.labels.cpu().numpy()))
