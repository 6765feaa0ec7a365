"""Non-rigid alignment by a cubic B-spline free-form deformation (FFD) under Mattes mutual information, restated in
numpy: the executable statement of include/t2fit.h's t2fit_ffd_joint_hist_dev, t2fit_ffd_gradient_dev, t2fit_ffd_warp_dev
and t2fit_ffd_jacobian_dev, and the loop both the statement and the device path run.  The reference has no
non-rigid step (``build_jhu_ho_labels`` is flirt with 12 degrees of freedom); the model is Rueckert's FFD (1999) with
the lattice of :mod:`_bias` and the metric of :mod:`_register`.  Parity with elastix, NiftyReg or ANTs is not pinned.

**The transform.**  For a fixed voxel index ``x = (ix, iy, iz)`` the moving index coordinate is
``c(x) = A (x + d(x), 1)`` with ``d_k(x) = sum bz by bx phi_k[kz.., ky.., kx..]``, ``k = 0..2`` (0 is x): ``A`` the 3 x 4
index affine of :func:`_resample.index_affine`, ``phi`` a float64 ``(3, c, c, c)`` lattice of side ``c`` in (4, 5, 7, 11,
19), ``d`` in fixed-grid voxels.  First node and weights per axis are :func:`_bias.axis_weights`'s; the taps are added z,
then y, then x, each in tap order (:func:`_bias.field_eval`'s order), in float64; ``x + d`` goes through ``A`` in the
order of :func:`_resample._coords`: ``((A[k][0] px + A[k][1] py) + A[k][2] pz) + A[k][3]``.  A lattice of zeros (or
None) gives the coordinates of the affine path bit for bit.  Arrays are ``(Z, Y, X)``; every multiply and add rounds
once."""
from __future__ import annotations

import numpy as np

from . import _bias, _register, _resample

SIDES = _bias.SIDES                      # 4, 5, 7, 11, 19: a side c subdivides to 2 c - 3
ZCHUNK = 8                               # planes the statement handles at a time (memory only; no sum depends on it)
DEFAULT_SCHEDULE = ((4, 4), (2, 5), (1, 7))
# One sweep of the CPU statement on the recovery phantom of tests/ffd_cases.py is all these three rest on
DEFAULT_WEIGHT, DEFAULT_MAX_ITER, DEFAULT_MAX_STEP = 0.05, 20, 0.5


# ---- the lattice -----------------------------------------------------------------------------------------------------------
def check_lattice(phi, side=None):
    """float64 ``(3, c, c, c)``, finite, ``c`` one of :data:`SIDES`; None with ``side``: zeros."""
    if phi is None:
        phi = np.zeros((3,) + (int(SIDES[0] if side is None else side),) * 3)
    phi = np.ascontiguousarray(phi, np.float64)
    if phi.ndim != 4 or phi.shape[0] != 3 or phi.shape[1] not in SIDES or phi.shape[1:] != (phi.shape[1],) * 3:
        raise ValueError(f"the lattice is float64 (3, c, c, c) with c one of {SIDES}, got shape {phi.shape}")
    if not np.all(np.isfinite(phi)):
        raise ValueError("the lattice has a non-finite entry")
    return phi


def axis_tables(n, c):
    """Along an axis of ``n`` voxels under a lattice of side ``c``: the first node ``k[n]``, the weights ``b[n, 4]`` of
    :func:`_bias.axis_weights` and ``db[n, 4]``, their derivatives with respect to the voxel index: the derivative of the
    basis in ``tau`` (``-(om om) 0.5``, ``1.5 t2 - 2 tau``, ``(-1.5 t2 + tau) + 0.5``, ``t2 0.5``) times
    ``(c - 3) / (n - 1)`` (0 when ``n`` is 1)."""
    s = c - 3
    if n == 1:
        tau, scale = np.zeros(1), 0.0
    else:
        p = np.arange(n, dtype=np.float64) * s / (n - 1)
        tau = p - np.floor(p)
        tau[-1] = 1.0
        scale = float(s) / float(n - 1)
    k, b, _, _ = _bias.axis_weights(n, c)
    t2, om = tau * tau, 1.0 - tau
    db = np.stack([-((om * om) * 0.5), 1.5 * t2 - 2.0 * tau, (-1.5 * t2 + tau) + 0.5, t2 * 0.5], axis=-1) * scale
    return k, b, db


def _tables(shape, c):
    return [axis_tables(int(n), c) for n in shape]


def _taps(w, k, src, axis, sl=slice(None)):
    """``sum_j w[:, j] src[k + j]`` along ``axis`` of ``src``, added in tap order."""
    idx = [slice(None)] * src.ndim
    shape = [1] * src.ndim
    shape[axis] = -1
    out = None
    for j in range(4):
        idx[axis] = k[sl] + j
        term = w[sl, j].reshape(shape) * src[tuple(idx)]
        out = term if out is None else out + term
    return out


def _eval(lattice, tabs, z0, nzc, which=(0, 0, 0)):
    """One component's field on the planes ``z0 .. z0 + nzc``; ``which[a]`` 1 takes the derivative weights along axis
    ``a`` (z, y, x)."""
    (kz, bz, dz), (ky, by, dy), (kx, bx, dx) = tabs
    t1 = _taps((bz, dz)[which[0]], kz, lattice, 0, slice(z0, z0 + nzc))     # [nzc, c, c]
    t2 = _taps((by, dy)[which[1]], ky, t1, 1)                                 # [nzc, ny, c]
    return _taps((bx, dx)[which[2]], kx, t2, 2)                               # [nzc, ny, nx]


def displacement(phi, shape, z0=0, nzc=None):
    """``[d_x, d_y, d_z]`` float64 on the planes ``z0 .. z0 + nzc`` of a fixed grid of ``shape`` (module docstring)."""
    phi = check_lattice(phi)
    nzc = shape[0] - z0 if nzc is None else nzc
    tabs = _tables(shape, phi.shape[1])
    return [_eval(phi[k], tabs, z0, nzc) for k in range(3)]


def coords(A, phi, shape, z0=0, nzc=None):
    """``[c_x, c_y, c_z]`` of the fixed voxels of the planes ``z0 .. z0 + nzc``; ``phi`` None: the affine path itself."""
    a = np.asarray(A, np.float64).reshape(3, 4)
    nzc = shape[0] - z0 if nzc is None else nzc
    box = (nzc, shape[1], shape[2])
    if phi is None:
        return _resample._coords(a, box, (0, 0, z0))
    d = displacement(phi, shape, z0, nzc)
    p = [np.arange(shape[2], dtype=np.float64)[None, None, :] + d[0],
         np.arange(shape[1], dtype=np.float64)[None, :, None] + d[1],
         np.arange(z0, z0 + nzc, dtype=np.float64)[:, None, None] + d[2]]
    return [((a[k, 0] * p[0] + a[k, 1] * p[1]) + a[k, 2] * p[2]) + a[k, 3] for k in range(3)]


def subdivide(phi):
    """Cubic subdivision of every axis of a ``(3, c, c, c)`` lattice, side ``c -> 2 c - 3`` (up to 19); the field is
    unchanged up to rounding.  Host code."""
    out = check_lattice(phi)
    if 2 * out.shape[1] - 3 > SIDES[-1]:
        raise ValueError(f"a lattice side above {SIDES[-1]} is refused")
    for axis in (1, 2, 3):
        a = np.moveaxis(out, axis, 0)
        new = np.empty((2 * a.shape[0] - 3,) + a.shape[1:])
        new[0::2] = (a[:-1] + a[1:]) / 2.0
        new[1::2] = (a[:-2] + 6.0 * a[1:-1] + a[2:]) / 8.0
        out = np.moveaxis(new, 0, axis)
    return np.ascontiguousarray(out)


def to_side(phi, side):
    """``phi`` subdivided until its side is ``side``; ValueError when it cannot get there."""
    phi = check_lattice(phi)
    while phi.shape[1] < side:
        phi = subdivide(phi)
    if phi.shape[1] != side:
        raise ValueError(f"a lattice of side {phi.shape[1]} does not subdivide to side {side} (sides are {SIDES})")
    return phi


def next_level(phi, side, s_prev, s):
    """The lattice of a level of shrink factor ``s_prev`` carried to side ``side`` on a level of shrink factor ``s``:
    subdivided, then multiplied by ``s_prev / s`` (displacements are in voxels of the level)."""
    return to_side(phi, side) * (float(s_prev) / float(s))


# ---- the four per-voxel steps ------------------------------------------------------------------------------------------------
def _chunks(nz):
    return [(z0, min(ZCHUNK, nz - z0)) for z0 in range(0, nz, ZCHUNK)]


def joint_histogram(bins, moving, A, phi, n_f, n_m, lo_m, scale_m, fixed_mask=None, moving_mask=None):
    """:func:`_register.joint_histogram` with ``c(x)`` in place of ``A x``: same counting rule, same window, integer
    sums."""
    bins, fmask, moving, mmask, n_m = _register._mi_bins(bins, fixed_mask, moving, moving_mask, n_f, n_m)
    a = np.asarray(A, np.float64).reshape(3, 4)
    phi = None if phi is None else check_lattice(phi)
    zero = np.zeros(bins.shape, np.float32)
    hist = np.zeros(n_f * n_m, np.uint64)
    for z0, nzc in _chunks(bins.shape[0]):
        with np.errstate(all="ignore"):
            t = _register._terms(zero, fmask, moving, mmask, a, z0, nzc, coords(a, phi, bins.shape, z0, nzc))
        counted = t[0] != 0.0
        i0, w, _ = _register.parzen_window(t[2][counted], lo_m, scale_m, n_m)
        row = bins[z0:z0 + nzc][counted].astype(np.int64) * n_m
        for j in range(4):
            np.add.at(hist, row + i0 - 1 + j, np.floor(w[j] * _register.HIST_ONE + 0.5).astype(np.uint64))
    return hist.reshape(n_f, n_m)


def force(bins, table, moving, A, phi, n_m, lo_m, scale_m, fixed_mask=None, moving_mask=None):
    """float64 ``(3, Z, Y, X)``: ``f_j(x) = ((s g_0) A[0][j] + (s g_1) A[1][j]) + (s g_2) A[2][j]`` at every counted voxel
    (``s`` the ``c`` of :func:`_register.mi_gradient_sums`, ``g`` the interpolant's gradient at ``c(x)``), +0.0 at the
    others: ``d(-MI) / d d_j(x)`` with the counted set held fixed."""
    table = np.asarray(table, np.float64)
    if table.ndim != 2 or table.shape[1] != int(n_m):
        raise ValueError("table is float64 (n_f, n_m)")
    bins, fmask, moving, mmask, n_m = _register._mi_bins(bins, fixed_mask, moving, moving_mask, table.shape[0], n_m)
    a = np.asarray(A, np.float64).reshape(3, 4)
    phi = None if phi is None else check_lattice(phi)
    zero = np.zeros(bins.shape, np.float32)
    flat = table.ravel()
    out = np.zeros((3,) + bins.shape, np.float64)
    for z0, nzc in _chunks(bins.shape[0]):
        with np.errstate(all="ignore"):
            t = _register._terms(zero, fmask, moving, mmask, a, z0, nzc, coords(a, phi, bins.shape, z0, nzc))
            counted = t[0] != 0.0
            i0, _, dw = _register.parzen_window(np.where(counted, t[2], float(lo_m)), lo_m, scale_m, n_m)
            at = bins[z0:z0 + nzc].astype(np.int64) * n_m + i0 - 1
            s = np.zeros(counted.shape, np.float64)
            for j in range(4):
                s = s + flat[at + j] * dw[j]
            sg = [s * t[6 + 4 * k + 3] for k in range(3)]
            for j in range(3):
                out[j, z0:z0 + nzc] = np.where(counted, (sg[0] * a[0, j] + sg[1] * a[1, j]) + sg[2] * a[2, j], 0.0)
    return out


def contract(values, c):
    """``G[cz, cy, cx] = sum_z bz sum_y by sum_x bx values[z, y, x]``: x by :func:`_bias.row_tree` (the order of a wave),
    then y, then z in index order from +0.0.  A node outside a voxel's four gets +0.0 from it, not a product with a zero
    weight: a non-finite value cannot reach a node whose support it lies outside."""
    values = np.asarray(values, np.float64)
    nz, ny, nx = values.shape
    (kz, bz, _), (ky, by, _), (kx, bx, _) = _tables(values.shape, c)
    xs = np.zeros((nz, ny, c))
    with np.errstate(all="ignore"):
        for cx in range(c):
            d = cx - kx
            inside = (d >= 0) & (d < 4)
            w = bx[np.arange(nx), np.clip(d, 0, 3)]
            xs[:, :, cx] = _bias.row_tree(np.where(inside[None, None, :], w[None, None, :] * values, 0.0))
        ys = np.zeros((nz, c, c))
        for y in range(ny):
            for j in range(4):
                ys[:, ky[y] + j, :] = ys[:, ky[y] + j, :] + by[y, j] * xs[:, y, :]
        out = np.zeros((c, c, c))
        for z in range(nz):
            for j in range(4):
                out[kz[z] + j] = out[kz[z] + j] + bz[z, j] * ys[z]
    return out


def gradient(bins, table, moving, A, phi, n_m, lo_m, scale_m, fixed_mask=None, moving_mask=None, side=None):
    """float64 ``(3, c, c, c)``: the lattice gradient of ``-MI`` with the counted set held fixed, :func:`contract` of
    :func:`force`.  ``phi`` None: the gradient at the zero lattice of ``side``."""
    c = check_lattice(phi, side).shape[1]
    f = force(bins, table, moving, A, phi, n_m, lo_m, scale_m, fixed_mask, moving_mask)
    return np.stack([contract(f[j], c) for j in range(3)])


def warp(src, A, phi, out_shape, interp="linear", default=0.0):
    """``src`` sampled at ``c(x)`` on the fixed grid of ``out_shape``: the arithmetic of :func:`_resample.resample`
    (linear: float32; nearest: float32 or int32 with ``default`` outside)."""
    out_shape = tuple(int(v) for v in out_shape)
    phi = None if phi is None else check_lattice(phi)
    with np.errstate(all="ignore"):
        return _resample.resample(src, A, out_shape, interp, default, coords=coords(A, phi, out_shape))


def jacobian(phi, shape):
    """float64 ``det(I + dd/dx)`` at every voxel of ``shape`` from the analytic derivative weights (:func:`axis_tables`):
    ``(a00 (a11 a22 - a12 a21) - a01 (a10 a22 - a12 a20)) + a02 (a10 a21 - a11 a20)``, ``a[k][a] = [k == a] + dd_k/dx_a``."""
    phi = check_lattice(phi)
    shape = tuple(int(v) for v in shape)
    tabs = _tables(shape, phi.shape[1])
    det = np.empty(shape, np.float64)
    for z0, nzc in _chunks(shape[0]):
        # a[k][axis]: axis 0 is x (derivative weights along x: which = (0, 0, 1)), 1 is y, 2 is z
        a = [[_eval(phi[k], tabs, z0, nzc, w) for w in ((0, 0, 1), (0, 1, 0), (1, 0, 0))] for k in range(3)]
        for k in range(3):
            a[k][k] = 1.0 + a[k][k]
        det[z0:z0 + nzc] = ((a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]))
                            + a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]))
    return det


def min_jacobian(phi, mask):
    """``(min det, count of det <= 0)`` over the voxels of ``mask`` (0 / not 0); an empty mask gives ``(+inf, 0)``."""
    mask = np.asarray(mask) != 0
    if mask.ndim != 3:
        raise ValueError("mask is a (Z, Y, X) volume")
    det = jacobian(phi, mask.shape)[mask]
    return (float(det.min()) if det.size else float("inf")), int(np.count_nonzero(det <= 0.0))


# ---- regulariser (host, float64) -------------------------------------------------------------------------------------------
def regulariser(phi):
    """``(R, dR/dphi)``: the mean of the squared second differences ``phi[i - 1] - 2 phi[i] + phi[i + 1]`` of the three
    components along the three lattice axes.  Host code, shared by both paths."""
    phi = check_lattice(phi)
    total, count, g = 0.0, 0, np.zeros_like(phi)
    for axis in (1, 2, 3):
        p, gv = np.moveaxis(phi, axis, 0), np.moveaxis(g, axis, 0)
        d = (p[:-2] - 2.0 * p[1:-1]) + p[2:]
        total += float(np.sum(d * d))
        count += d.size
        gv[:-2] += 2.0 * d
        gv[1:-1] -= 4.0 * d
        gv[2:] += 2.0 * d
    return total / count, g / count


# ---- the loop --------------------------------------------------------------------------------------------------------------
class FFDRegistration:
    """``affine``: the :class:`_register.Registration` the deformation started from (``transform`` and ``parameters`` are
    its); ``lattice``: float64 ``(3, c, c, c)`` in voxels of the full-resolution fixed grid; ``iterations`` / ``stops``
    per entry of ``schedule``; ``cost``: ``-MI + weight R`` at the returned lattice on the last level; ``min_jacobian``
    and ``n_folded``: the smallest ``det(I + dd/dx)`` and the count of ``det <= 0`` inside the fixed mask at full
    resolution.  A folded result is reported, not refused."""

    def __init__(self, affine, lattice, schedule, iterations, stops, cost, min_jacobian, n_folded):  # noqa: A002
        self.affine, self.lattice, self.schedule = affine, lattice, tuple(schedule)
        self.iterations, self.stops, self.stop = tuple(iterations), tuple(stops), stops[-1]
        self.cost, self.min_jacobian, self.n_folded = float(cost), float(min_jacobian), int(n_folded)

    transform = property(lambda self: self.affine.transform)
    parameters = property(lambda self: self.affine.parameters)
    side = property(lambda self: self.lattice.shape[1])

    def __repr__(self):
        return (f"FFDRegistration(side={self.side}, cost={self.cost:.6f}, iterations={self.iterations}, stop={self.stop!r}, "
                f"min_jacobian={self.min_jacobian:.4f}, n_folded={self.n_folded})")


def check_schedule(schedule, fixed_shape, moving_shape):
    """((shrink, side), ..): shrink factors as :func:`_register.check_levels`, sides from :data:`SIDES`, never falling, each
    reachable from the one before by subdivision."""
    try:
        schedule = tuple((int(s), int(c)) for s, c in schedule)
    except (TypeError, ValueError):
        raise ValueError(f"schedule is a sequence of (shrink, side) pairs, got {schedule!r}") from None
    if not schedule:
        raise ValueError("schedule is empty")
    _register.check_levels([s for s, _ in schedule], fixed_shape, moving_shape)
    sides = [c for _, c in schedule]
    if any(c not in SIDES for c in sides) or any(b < a for a, b in zip(sides, sides[1:])):
        raise ValueError(f"lattice sides come from {SIDES} and never fall, got {tuple(sides)}")
    return schedule


def check_options(weight, max_iter, max_step):
    if not (np.isfinite(weight) and weight >= 0.0):
        raise ValueError(f"weight is finite and >= 0, got {weight!r}")
    if int(max_iter) < 0:
        raise ValueError(f"max_iter is >= 0, got {max_iter!r}")
    if not (np.isfinite(max_step) and max_step > 0.0):
        raise ValueError(f"max_step is finite and > 0 (voxels of the level), got {max_step!r}")
    return float(weight), int(max_iter), float(max_step)


class HostFFDPyramid(_register.HostAffinePyramid):
    """:class:`_register.HostAffinePyramid` and the four steps of the deformation; the device path has the same methods."""

    def hist(self, level, bins, n_f, n_m, lo_m, scale_m, A, phi):
        _, fmask, moving, mmask = level[:4]
        return joint_histogram(bins, moving, A, phi, n_f, n_m, lo_m, scale_m, fmask, mmask)

    def gradient(self, level, bins, table, n_m, lo_m, scale_m, A, phi):
        _, fmask, moving, mmask = level[:4]
        return gradient(bins, table, moving, A, phi, n_m, lo_m, scale_m, fmask, mmask)

    def warp(self, src, A, phi, out_shape, interp="linear", default=0.0):
        return warp(src, A, phi, out_shape, interp, default)

    def jacobian(self, phi, mask):
        return min_jacobian(phi, mask)


def optimize_ffd(pyramid, fixed_geom, moving_geom, affine, *, schedule=DEFAULT_SCHEDULE, bins=32, moving_bins=32,
                 weight=DEFAULT_WEIGHT, max_iter=DEFAULT_MAX_ITER, max_step=DEFAULT_MAX_STEP):
    """The regular-step descent of :func:`_register.optimize_affine` over the lattice, level by level.  Per entry
    ``(s, c)`` of ``schedule``: the level of shrink factor ``s`` and its index affine from ``affine.transform``; fixed bins
    and the moving range as 'mattes' sets them; the lattice of the level before subdivided to side ``c`` and multiplied by
    ``s_prev / s`` (displacements are in voxels of the level; the first level starts from zeros).  Per iteration: the joint
    histogram, ``-MI`` and the table, the lattice gradient, ``cost = -MI + weight R`` and ``g`` its gradient; ``norm`` the
    largest node-gradient norm; stop when ``norm < 1e-6`` ('gradient'); halve the step when ``g`` and the previous ``g``
    have a negative scalar product; stop when the step is below 1e-6 ('step'); move ``phi -= (step / norm) g``, so no node
    moves by more than ``step`` voxels; stop after ``max_iter`` moves ('iterations').  The first step of a level is
    ``max_step`` voxels of that level."""
    n_f, n_m = _register._check_bins(bins), _register._check_moving_bins(moving_bins)
    weight, max_iter, max_step = check_options(weight, max_iter, max_step)
    transform = np.asarray(affine.transform if hasattr(affine, "transform") else affine, np.float64)
    phi, s_prev, iterations, stops = None, None, [], []
    for s, side in schedule:
        level = pyramid.level(s)
        fg, mg = _register.level_geometry(fixed_geom, s), _register.level_geometry(moving_geom, s)
        a = _resample.index_affine(fg, mg, transform)
        level_bins = pyramid.bins(level, n_f)
        lo_m, scale_m = pyramid.moving_range(level, n_m)
        phi = np.zeros((3, side, side, side)) if phi is None else next_level(phi, side, s_prev, s)
        s_prev = s

        def evaluate(q):
            c, table = _register.mattes_metric(pyramid.hist(level, level_bins, n_f, n_m, lo_m, scale_m, a, q), n_f, n_m, scale_m)
            g = np.asarray(pyramid.gradient(level, level_bins, table, n_m, lo_m, scale_m, a, q), np.float64).reshape(q.shape)
            r, gr = regulariser(q)
            return c + weight * r, g + weight * gr

        step, prev, n_it, stop = max_step, None, 0, "iterations"
        while True:
            c, g = evaluate(phi)
            norm = float(np.sqrt(np.max(np.sum(g * g, axis=0))))
            if not norm >= _register.GRAD_TOL:
                stop = "gradient"
                break
            if prev is not None and float(np.sum(g * prev)) < 0.0:
                step *= _register.RELAX
            if step < _register.MIN_STEP:
                stop = "step"
                break
            if n_it >= max_iter:
                break
            phi = phi - (step / norm) * g
            prev, n_it = g, n_it + 1
        iterations.append(n_it)
        stops.append(stop)
    full = np.ascontiguousarray(phi * float(s_prev))
    min_det, folded = pyramid.jacobian(full, pyramid.full[1])
    return FFDRegistration(affine, full, schedule, iterations, stops, c, min_det, folded)


def register_ffd(fixed, moving, fixed_geom, moving_geom, *, affine, fixed_mask=None, moving_mask=None, schedule=DEFAULT_SCHEDULE,
                 bins=32, moving_bins=32, weight=DEFAULT_WEIGHT, max_iter=DEFAULT_MAX_ITER, max_step=DEFAULT_MAX_STEP):
    """Deform ``moving`` onto ``fixed`` from the affine result ``affine`` (a :class:`_register.Registration`, or anything
    with a 4 x 4 ``transform``: fixed point -> moving point): :func:`optimize_ffd`.  Masks None: ``build_mask`` of the
    volume.  The metric is Mattes mutual information whatever metric found ``affine``.  ``schedule`` whose last shrink
    factor is 1 (the default) ends on the full-resolution grid; otherwise the returned lattice is the last level's times
    its shrink factor, which is that level's deformation up to the half-voxel offset of a block mean's grid.  Returns an
    :class:`FFDRegistration`.  The statement of ``t2map.register.register_ffd``."""
    fixed, moving = np.asarray(fixed, np.float32), np.asarray(moving, np.float32)
    fmask = _register.build_mask(fixed) if fixed_mask is None else fixed_mask
    mmask = _register.build_mask(moving) if moving_mask is None else moving_mask
    pyramid = HostFFDPyramid(fixed, fmask, moving, mmask)
    fg, mg = _resample.as_geometry(fixed_geom, fixed.shape), _resample.as_geometry(moving_geom, moving.shape)
    schedule = check_schedule(schedule, fixed.shape, moving.shape)
    return optimize_ffd(pyramid, fg, mg, affine, schedule=schedule, bins=bins, moving_bins=moving_bins, weight=weight,
                        max_iter=max_iter, max_step=max_step)


def nonrigid_options(nonrigid):
    """The keywords of :func:`register_ffd` from ``atlas_labels(nonrigid=)``: True is the defaults, a dict overrides them."""
    if nonrigid is True:
        return {}
    allowed = ("schedule", "bins", "moving_bins", "weight", "max_iter", "max_step")
    if not isinstance(nonrigid, dict) or any(k not in allowed for k in nonrigid):
        raise ValueError(f"nonrigid is None, True or a dict with keys from {allowed}, got {nonrigid!r}")
    return dict(nonrigid)
