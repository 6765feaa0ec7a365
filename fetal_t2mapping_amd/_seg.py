"""Atlas-prior EM tissue segmentation, stated in numpy: the definition ``csrc/t2fit_seg.hip`` is held to.

A Gaussian mixture over ``C`` channels (a few echoes of one subject) and ``K`` tissue classes, with spatial priors blurred
from a propagated label atlas and a mean-field Potts term (Van Leemput et al. 1999; Habas et al. 2010 for fetal brains; FSL
FAST and ANTs Atropos are of this family).  Arrays are ``(Z, Y, X)`` with x fastest; ``y`` is ``(C, Z, Y, X)`` float32,
posteriors and priors are ``(K, Z, Y, X)`` float32.  ``M`` is the set of voxels where ``mask != 0`` and every channel is
finite (:func:`effective_mask`).  Every sum below is float64, one rounding per operation in the order written, and one
rounding to float32 where a float32 is stored; include/t2fit.h says the same in words.

Host code shared by the numpy and the device path: :func:`gauss_taps`, :func:`class_model`, :func:`pack_model` and the
driver :func:`segment_em`, which takes the step functions as ``steps`` (the device's are in ``_gpu_seg``), so the loop
exists once.

The defaults (``sigma = 2`` voxels for the priors, ``beta = 0.5``, ``prior_floor = 1e-3``, 15 iterations) come from a sweep on
one synthetic phantom and nothing else (DESIGN.md 8p has the table): nested ellipsoids of 4 classes in 32 x 40 x 48 voxels,
2 channels, noise 40 on contrasts of 120 .. 400, the atlas displaced by (1, -2, 2) voxels and mis-scaled.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

MAX_CLASSES, MAX_CHANNELS, MAX_RADIUS = 8, 4, 32
VOX_PER_LANE, LANES, WAVE, FAN = 4, 256, 64, 256  # the tree of moment_sums
VOX_PER_BLOCK = VOX_PER_LANE * LANES

SegSteps = namedtuple("SegSteps", "effective_mask normalise_priors moment_sums e_step hard_labels")
SegModel = namedtuple("SegModel", "mean cov precision logc dead")
SegResult = namedtuple("SegResult", "labels model s0_trace n_iter posteriors n_reassigned", defaults=(0,))


def n_moments(n_chan):
    return 1 + n_chan + n_chan * (n_chan + 1) // 2


def gauss_taps(sigma):
    """The ``2 r + 1`` float64 taps of a Gaussian of ``sigma`` voxels, ``r = int(4 sigma + 0.5)`` (scipy's rule at
    ``truncate=4``): ``exp(-j^2 / (2 sigma^2))`` for ``j = -r .. r`` divided by their sum.  ``sigma == 0``: the identity."""
    sigma = float(sigma)
    if not (sigma >= 0.0) or not np.isfinite(sigma):
        raise ValueError(f"sigma must be finite and >= 0, got {sigma}")
    r = int(4.0 * sigma + 0.5)
    if r > MAX_RADIUS:
        raise ValueError(f"sigma = {sigma} needs a radius of {r} taps; at most {MAX_RADIUS}")
    if r == 0:
        return np.ones(1, np.float64)
    j = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-(j * j) / (2.0 * sigma * sigma))
    return w / math.fsum(w)  # the correctly rounded sum: the taps then add up to 1 within 2^-52


def _axis_taps(sigma):
    s = np.broadcast_to(np.asarray(sigma, np.float64), (3,)) if np.ndim(sigma) <= 1 else None
    if s is None or (np.ndim(sigma) == 1 and len(sigma) != 3):
        raise ValueError("sigma must be a scalar or (sigma_z, sigma_y, sigma_x)")
    return [gauss_taps(v) for v in s]


def _classes(classes):
    c = np.asarray(classes)
    if c.ndim != 1 or not (2 <= c.size <= MAX_CLASSES) or c.dtype.kind not in "iu":
        raise ValueError(f"classes must be 2 .. {MAX_CLASSES} integer label values")
    c = c.astype(np.int64)
    if len(set(c.tolist())) != c.size or np.any(c == 0) or np.any(np.abs(c) > 2**31 - 1):
        raise ValueError("classes must be distinct, non-zero and fit int32")
    return c.astype(np.int32)


def blur_axis(vol, w, axis):
    """One pass: ``float32(sum_j w_j (double)in[i + j - r])``, j ascending from 0.0, taps beyond the volume left out."""
    r = (len(w) - 1) // 2
    src = np.moveaxis(np.asarray(vol, np.float32).astype(np.float64), axis, -1)
    n = src.shape[-1]
    acc = np.zeros(src.shape, np.float64)
    for j in range(2 * r + 1):
        o = j - r  # out[i] takes in[i + o]
        lo, hi = max(0, -o), min(n, n - o)
        if lo < hi:
            acc[..., lo:hi] = acc[..., lo:hi] + w[j] * src[..., lo + o:hi + o]
    return np.ascontiguousarray(np.moveaxis(acc.astype(np.float32), -1, axis))


def priors_from_labels(labels, classes, sigma=2.0):
    """``(K, Z, Y, X)`` float32: plane k is the one-hot image ``labels == classes[k]`` blurred along x, then y, then z."""
    labels = np.asarray(labels)
    if labels.ndim != 3:
        raise ValueError("labels must be (Z, Y, X)")
    classes = _classes(classes)
    wz, wy, wx = _axis_taps(sigma)
    out = np.empty((len(classes),) + labels.shape, np.float32)
    for k, c in enumerate(classes):
        v = (labels == c).astype(np.float32)
        out[k] = blur_axis(blur_axis(blur_axis(v, wx, 2), wy, 1), wz, 0)
    return out


def effective_mask(y, mask):
    """``M``: uint8 0 / 1, ``mask != 0`` (None: everywhere) and every channel finite."""
    y = np.asarray(y)
    m = np.ones(y.shape[1:], bool) if mask is None else np.asarray(mask) != 0
    return (m & np.all(np.isfinite(y), axis=0)).astype(np.uint8)


def normalise_priors(prior, mask, floor=1e-3):
    """``pi_ik = float32(((double)prior_ik + floor) / (sum_l (double)prior_il + K floor))``, l ascending; 0 outside the mask."""
    prior = np.asarray(prior, np.float32)
    K = prior.shape[0]
    m = np.asarray(mask) != 0
    total = np.zeros(prior.shape[1:], np.float64)
    for l in range(K):
        total = total + prior[l].astype(np.float64)
    den = total + float(K) * float(floor)
    out = np.zeros(prior.shape, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(K):
            out[k] = np.where(m, ((prior[k].astype(np.float64) + float(floor)) / den).astype(np.float32), np.float32(0.0))
    return out


def _tree(terms):
    """The fixed tree over the flat voxels of ``terms`` (float64, zero where a voxel is left out; adding +0.0 to a sum that
    starts at +0.0 changes no bit, so a zero term and a skipped one are the same).  Lane by lane:

    * workgroup ``b`` takes the voxels ``1024 b .. 1024 b + 1023``; its lane ``t`` (0 .. 255) adds those at
      ``1024 b + 256 j + t``, ``j = 0, 1, 2, 3`` in this order from 0.0;
    * each wave (64 consecutive lanes) folds by the butterfly ``v = v + v[lane ^ s]``, ``s = 32, 16, 8, 4, 2, 1``;
    * the four waves add as ``((w0 + w1) + w2) + w3``;
    * the workgroup values are folded in passes until one is left, at least one pass: a pass turns 256 consecutive values
      (zeros beyond the end) into one by ``s[t] = s[t] + s[t + h]`` for ``t < h``, ``h = 128, 64, .. 1``."""
    flat = np.asarray(terms, np.float64).reshape(-1)
    nb = -(-flat.size // VOX_PER_BLOCK)
    v = np.zeros(nb * VOX_PER_BLOCK, np.float64)
    v[:flat.size] = flat
    v = v.reshape(nb, VOX_PER_LANE, LANES)
    acc = np.zeros((nb, LANES), np.float64)
    for j in range(VOX_PER_LANE):
        acc = acc + v[:, j]
    acc = acc.reshape(nb, LANES // WAVE, WAVE)
    lane = np.arange(WAVE)
    s = WAVE // 2
    while s >= 1:
        acc = acc + acc[..., lane ^ s]
        s //= 2
    w = acc[..., 0]
    vals = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    while True:
        n_out = -(-vals.size // FAN)
        s_ = np.zeros(n_out * FAN, np.float64)
        s_[:vals.size] = vals
        s_ = s_.reshape(n_out, FAN)
        h = FAN // 2
        while h >= 1:
            s_[:, :h] = s_[:, :h] + s_[:, h:2 * h]
            h //= 2
        vals = s_[:, 0].copy()
        if n_out == 1:
            return float(vals[0])


def moment_sums(p, y, mask):
    """``(K, 1 + C + C (C + 1) / 2)`` float64: per class ``S0 = sum p``, ``S1_c = sum p y_c``, ``S2_cd = sum (p y_c) y_d``
    (c <= d, row-major) over ``M``, each in the tree of :func:`_tree`."""
    p, y = np.asarray(p, np.float32), np.asarray(y, np.float32)
    K, C = p.shape[0], y.shape[0]
    M = effective_mask(y, mask).astype(bool)
    yd = np.where(M, y.astype(np.float64), 0.0)
    out = np.zeros((K, n_moments(C)), np.float64)
    for k in range(K):
        pv = np.where(M, p[k].astype(np.float64), 0.0)
        out[k, 0] = _tree(pv)
        m = 1 + C
        for c in range(C):
            py = pv * yd[c]
            out[k, 1 + c] = _tree(py)
            for d in range(c, C):
                out[k, m] = _tree(py * yd[d])
                m += 1
    return out


def class_model(sums, n_chan, var_floor=1e-6):
    """Means, covariances, precisions and ``c_k = -0.5 log det Sigma_k`` from the sums of :func:`moment_sums`.
    ``Sigma_k = S2 / S0 - mu mu^T + var_floor diag(pooled variance of each channel)``, the pooled variance from the same
    sums added over the classes.  A class with ``S0 < C + 1``, or whose covariance is not positive definite, is dead; all
    classes dead raises."""
    sums = np.asarray(sums, np.float64)
    K, C = sums.shape[0], int(n_chan)
    if sums.shape[1] != n_moments(C):
        raise ValueError("sums does not have 1 + C + C (C + 1) / 2 columns")
    tot = np.zeros(n_moments(C))
    for k in range(K):
        tot = tot + sums[k]
    iu = [(c, d) for c in range(C) for d in range(c, C)]
    pooled = np.zeros(C)
    if tot[0] > 0:
        for c in range(C):
            mu = tot[1 + c] / tot[0]
            pooled[c] = max(tot[1 + C + iu.index((c, c))] / tot[0] - mu * mu, 0.0)
    mean, cov, prec = np.zeros((K, C)), np.zeros((K, C, C)), np.zeros((K, C, C))
    logc, dead = np.zeros(K), np.zeros(K, bool)
    for k in range(K):
        s0 = sums[k, 0]
        if not (s0 >= C + 1):
            dead[k] = True
            continue
        mean[k] = sums[k, 1:1 + C] / s0
        for m, (c, d) in enumerate(iu):
            v = sums[k, 1 + C + m] / s0 - mean[k, c] * mean[k, d]
            cov[k, c, d] = cov[k, d, c] = v
        cov[k] += var_floor * np.diag(pooled)
        sign, logdet = np.linalg.slogdet(cov[k])
        if not (sign > 0) or not np.isfinite(logdet) or not np.all(np.isfinite(cov[k])) or np.any(np.diag(cov[k]) <= 0):
            dead[k] = True
            continue
        prec[k] = np.linalg.inv(cov[k])
        prec[k] = 0.5 * (prec[k] + prec[k].T)
        logc[k] = -0.5 * logdet
    if dead.all():
        raise ValueError("segment_em: every class is dead (no class holds C + 1 voxels' worth of posterior mass inside the mask)")
    return SegModel(mean, cov, prec, logc, dead)


def pack_model(model):
    """``(K, C + C (C + 1) / 2 + 1)`` float64 rows ``(mu, upper triangle of P row-major, c)`` and int32 live flags: what the
    E-step takes."""
    K, C = model.mean.shape
    rows = np.zeros((K, C + C * (C + 1) // 2 + 1), np.float64)
    for k in range(K):
        rows[k, :C] = model.mean[k]
        m = C
        for c in range(C):
            for d in range(c, C):
                rows[k, m] = model.precision[k, c, d]
                m += 1
        rows[k, m] = model.logc[k]
    return rows, (~model.dead).astype(np.int32)


def e_step(p_old, pi, y, mask, model, beta):
    """One mean-field E-step (Jacobi: reads ``p_old``, returns new posteriors).  For a voxel of ``M`` and a live class:
    ``t_c = y_c - mu_c``; ``d = sum_{c<=d} (((c == d ? 1 : 2) P_cd) t_c) t_d`` row-major from 0.0; ``n = sum (1 - p_old_jk)``
    from 0.0 over the neighbours inside the volume and in ``M``, in the order -z, -y, -x, +x, +y, +z;
    ``a_k = (c_k - 0.5 d) - beta n``; ``q_k = pi_ik exp(a_k - max a)``; ``p_ik = float32(q_k / sum_k q_k)``, k ascending.
    Dead classes and voxels outside ``M`` get +0.0."""
    p_old, pi, y = np.asarray(p_old, np.float32), np.asarray(pi, np.float32), np.asarray(y, np.float32)
    K, C = p_old.shape[0], y.shape[0]
    rows, live = pack_model(model) if isinstance(model, SegModel) else (np.asarray(model[0], np.float64), np.asarray(model[1]))
    M = effective_mask(y, mask).astype(bool)
    Z, Y, X = M.shape
    Mp = np.zeros((Z + 2, Y + 2, X + 2), bool)
    Mp[1:-1, 1:-1, 1:-1] = M
    shifts = [(0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 2), (1, 2, 1), (2, 1, 1)]  # -z, -y, -x, +x, +y, +z
    yd = np.where(M, y.astype(np.float64), 0.0)
    a = np.full((K, Z, Y, X), -np.inf)
    for k in range(K):
        if not live[k]:
            continue
        t = [yd[c] - rows[k, c] for c in range(C)]
        d = np.zeros((Z, Y, X))
        m = C
        for c in range(C):
            for e in range(c, C):
                d = d + (((1.0 if c == e else 2.0) * rows[k, m]) * t[c]) * t[e]
                m += 1
        pp = np.zeros((Z + 2, Y + 2, X + 2))
        pp[1:-1, 1:-1, 1:-1] = p_old[k].astype(np.float64)
        nb = np.zeros((Z, Y, X))
        for (sz, sy, sx) in shifts:
            inm = Mp[sz:sz + Z, sy:sy + Y, sx:sx + X]
            nb = np.where(inm, nb + (1.0 - pp[sz:sz + Z, sy:sy + Y, sx:sx + X]), nb)
        a[k] = (rows[k, m] - 0.5 * d) - float(beta) * nb
    top = a.max(axis=0)
    q = np.zeros((K, Z, Y, X))
    s = np.zeros((Z, Y, X))
    for k in range(K):
        if live[k]:
            q[k] = pi[k].astype(np.float64) * np.exp(a[k] - top)
            s = s + q[k]
    out = np.zeros((K, Z, Y, X), np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(K):
            if live[k]:
                out[k] = np.where(M, (q[k] / s).astype(np.float32), np.float32(0.0))
    return out


def hard_labels(p, classes, mask):
    """int32 ``classes[first argmax_k p]`` where ``mask != 0``, 0 elsewhere."""
    p = np.asarray(p, np.float32)
    classes = _classes(classes)
    return np.where(np.asarray(mask) != 0, classes[np.argmax(p, axis=0)], 0).astype(np.int32)


NUMPY_STEPS = SegSteps(effective_mask, normalise_priors, moment_sums, e_step, hard_labels)


def check_em_arguments(n_class, n_chan, beta, prior_floor, var_floor, n_iter, tol):
    if not 2 <= n_class <= MAX_CLASSES:
        raise ValueError(f"segment_em takes 2 .. {MAX_CLASSES} classes, got {n_class}")
    if not 1 <= n_chan <= MAX_CHANNELS:
        raise ValueError(f"segment_em takes 1 .. {MAX_CHANNELS} channels, got {n_chan}")
    for name, v in (("beta", beta), ("prior_floor", prior_floor), ("var_floor", var_floor), ("tol", tol)):
        if not (float(v) >= 0.0) or not np.isfinite(float(v)):
            raise ValueError(f"{name} must be finite and >= 0, got {v}")
    if int(n_iter) < 1:
        raise ValueError("n_iter must be >= 1")


def run_em(pi, y, M, n_chan, steps, *, beta, var_floor, n_iter, tol):
    """The loop both paths run, on whatever array type the ``steps`` work on: ``p0 = pi``; an iteration takes the sums of
    the current p, the model from them, then the E-step.  With ``tol > 0`` it stops once
    ``max_k |S0_k - S0_k(previous)| <= tol sum_k S0_k``.  Returns ``(p, model, s0_trace, iterations)``."""
    p, model, trace, prev, it = pi, None, [], None, 0
    while it < int(n_iter):
        sums = np.asarray(steps.moment_sums(p, y, M), np.float64)
        s0 = sums[:, 0].copy()
        if tol > 0 and prev is not None and np.max(np.abs(s0 - prev)) <= tol * np.sum(s0):
            break
        model = class_model(sums, n_chan, var_floor)
        trace.append(s0)
        p = steps.e_step(p, pi, y, M, model, beta)
        prev = s0
        it += 1
    return p, model, np.array(trace, np.float64), it


def segment_em(y, mask, prior, classes, *, beta=0.5, prior_floor=1e-3, var_floor=1e-6, n_iter=15, tol=0.0, steps=None,
               return_posteriors=False, min_island=0):
    """Segment ``y`` ``(C, Z, Y, X)`` inside ``mask`` into the ``classes`` from spatial priors ``prior`` ``(K, Z, Y, X)``
    (:func:`priors_from_labels`) by expectation-maximisation.  Returns a :class:`SegResult`: int32 labels (0 outside ``M``),
    the last model (:class:`SegModel`: means, covariances, precisions, dead flags), the ``S0`` of every iteration, the
    number of iterations run and, with ``return_posteriors``, the posteriors.  ``min_island`` > 0: the islands of the hard
    labels with fewer voxels take the class of their surroundings (``_edt.reassign_small``, 6 neighbours, unit spacing)
    and ``n_reassigned`` counts the voxels changed; the posteriors are not touched."""
    steps = NUMPY_STEPS if steps is None else steps
    y = np.asarray(y, np.float32)
    if y.ndim == 3:
        y = y[None]
    prior = np.asarray(prior, np.float32)
    classes = _classes(classes)
    if y.ndim != 4 or prior.ndim != 4 or prior.shape[1:] != y.shape[1:] or prior.shape[0] != len(classes):
        raise ValueError(f"segment_em needs y (C, Z, Y, X) and prior (K, Z, Y, X) on one grid, got {y.shape} and {prior.shape}")
    check_em_arguments(len(classes), y.shape[0], beta, prior_floor, var_floor, n_iter, tol)
    M = steps.effective_mask(y, mask)
    pi = steps.normalise_priors(prior, M, prior_floor)
    p, model, trace, it = run_em(pi, y, M, y.shape[0], steps, beta=beta, var_floor=var_floor, n_iter=n_iter, tol=tol)
    labels, changed = steps.hard_labels(p, classes, M), 0
    if check_min_island(min_island):
        from . import _edt

        labels, changed = _edt.reassign_small(np.asarray(labels), min_island)
    return SegResult(labels, model, trace, it, p if return_posteriors else None, changed)


def check_min_island(min_island):
    """``min_island`` as an int >= 0 (0: off)."""
    if isinstance(min_island, bool) or int(min_island) != min_island or int(min_island) < 0:
        raise ValueError(f"min_island must be an integer >= 0, got {min_island!r}")
    return int(min_island)


TISSUE_KEYS = ("labels", "classes", "channels", "sigma", "beta", "prior_floor", "var_floor", "n_iter", "tol", "min_island")


def tissue_arguments(tissue, template_shape, subject_shape):
    """The ``tissue=`` dict of ``atlas_labels`` checked: ``(labels int32 on the template's grid, classes, channels float32
    (C, Z, Y, X) on the subject's grid, sigma, the keywords of segment_em)``.  ``labels``, ``classes`` and ``channels`` are
    required; ``sigma`` defaults to 2 voxels."""
    t = dict(tissue)
    unknown = sorted(set(t) - set(TISSUE_KEYS))
    if unknown:
        raise ValueError(f"tissue: unknown key(s) {', '.join(unknown)}; it takes {', '.join(TISSUE_KEYS)}")
    for key in ("labels", "classes", "channels"):
        if key not in t:
            raise ValueError(f"tissue needs {key!r}")
    labels = np.asarray(t.pop("labels"))
    if labels.dtype.kind not in "iu" or labels.shape != tuple(template_shape):
        raise ValueError(f"tissue['labels'] must be an integer volume on the template's grid {tuple(template_shape)}")
    classes = _classes(t.pop("classes"))
    channels = np.asarray(t.pop("channels"), np.float32)
    if channels.ndim == 3:
        channels = channels[None]
    if channels.ndim != 4 or channels.shape[1:] != tuple(subject_shape) or not 1 <= channels.shape[0] <= MAX_CHANNELS:
        raise ValueError(f"tissue['channels'] must be 1 .. {MAX_CHANNELS} volumes on the subject's grid {tuple(subject_shape)}")
    sigma = t.pop("sigma", 2.0)
    _axis_taps(sigma)
    return labels.astype(np.int32), classes, channels, sigma, t


def tissue_result(propagated, prior, res):
    """The fourth value of ``atlas_labels(tissue=...)``."""
    return {"labels": res.labels, "propagated": propagated, "prior": prior, "model": res.model, "s0_trace": res.s0_trace,
            "n_iter": res.n_iter, "n_reassigned": res.n_reassigned}


def dice(a, b, classes):
    """Dice overlap of two label volumes per class value."""
    out = []
    for c in classes:
        x, y = np.asarray(a) == c, np.asarray(b) == c
        den = x.sum() + y.sum()
        out.append(2.0 * (x & y).sum() / den if den else 1.0)
    return np.array(out)
