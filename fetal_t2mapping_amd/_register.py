"""Rigid registration of one volume onto another, restated in numpy: the executable statement of the definition in
include/t2fit.h (t2fit_register_sums_dev, t2fit_shrink_dev, t2fit_shrink_mask_dev) and the optimizer both the statement
and the device path run.  It builds the explicit recipe of the reference's ``registration_itk``
(utils/qmri_utils.py:167-221): correlation metric, fixed and moving masks from ``build_mask``, linear interpolator,
Euler 3-D transform, regular-step gradient descent (learning rate 1, 100 iterations, minimum step 1e-6, gradient
tolerance 1e-6), scales from the physical shift, and the 4 / 2 / 1 pyramid it has commented out -- deterministic where
ITK samples at random.  Parity with elastix (``registration_elastix``, what the reference actually calls) is unpinned.

Arrays are ``(Z, Y, X)``, x fastest; geometry is :class:`_resample.Geometry`'s.  Host code for tests and baselines, and
the host half (metric arithmetic, optimizer) of the product path; the sums over the voxels are the HIP kernel's there.

**The 43 sums.**  ``A`` is the index affine of :func:`_resample.index_affine` (fixed index -> continuous moving index).
A fixed voxel ``i = (ix, iy, iz)`` counts iff ``fixed_mask[i] != 0``, ``c = A (ix, iy, iz, 1)`` passes the inside test of
the resampler, and the moving mask at the nearest node ``floor(c + 0.5)`` (clamped) is not 0.  For a voxel that counts,
``f`` is the fixed sample, ``m`` the float64 trilinear interpolant of the moving volume (lower node clamped, upper node
replicated on the rim, x then y then z as ``lo + d (hi - lo)``, a zero weight returns ``lo``), and ``g_a = dm / dc_a`` the
difference of the two neighbours along axis ``a`` interpolated along the other two axes with the same weights; ``g_a`` is
0 where the interpolant is flat along ``a``: the upper neighbour is the clamped lower one, or ``c_a < 0`` (the lower
rim).  The sums, in this order::

    [0] N   [1] sum f   [2] sum m   [3] sum f f   [4] sum m m   [5] sum f m
    [6 + 4 (3 w + a) + j]  sum (w g_a) u_j      w in (1, f, m), a in (x, y, z), u = (ix, iy, iz, 1)
    [42] reserved, +0.0 (the count, 5 moments and 36 gradient sums are 42 numbers; the array has 43 slots)

Every product rounds once (``w g_a`` first, then ``u_j``; ``u_3 = 1`` is no multiplication); a voxel that does not
count contributes +0.0.  The volumes must be finite.

**The summation tree** (a function of the fixed volume's sizes alone).  The fixed volume is cut into bricks of
``BX x BY x BZ = 64 x 4 x 8`` voxels, padded with zeros.  In a brick, column ``(x, y)`` adds its 8 voxels in z order
starting from 0.0; the 64 columns of a row are added by halving (``v[:32] + v[32:]``, then 16, .. 1); the 4 rows by
halving.  That is the brick's slab.  The slabs, in ``(bz, by, bx)`` order, are reduced in passes: groups of 256
consecutive values (the last group padded with zeros) are each added by halving; passes repeat until one value is left
(at least one pass).

**The affine registration across contrasts** (``register_affine``: the correlation ratio over a binned fixed volume, 6 to
12 degrees of freedom; what the atlas-label stage of :mod:`_atlas` runs) is the last part of this module and builds on
everything above without changing it; so does **Mattes mutual information** (``metric="mattes"``: the cost elastix's
default rigid map minimises, which is what the reference's ``registration_elastix`` runs), stated after the correlation
ratio."""
from __future__ import annotations

import numpy as np

from . import _components, _morph, _resample

BX, BY, BZ = 64, 4, 8
FAN = 256
N_SUMS = 43
MIN_STEP, GRAD_TOL, RELAX, LEARNING_RATE = 1e-6, 1e-6, 0.5, 1.0
MIN_LEVEL_SIZE = 4  # a pyramid level keeps at least this many voxels per axis


def _halve(a):
    """Halving adds over the last axis (a power of two)."""
    while a.shape[-1] > 1:
        h = a.shape[-1] // 2
        a = a[..., :h] + a[..., h:]
    return a[..., 0]


def brick_counts(shape):
    """(bricks_z, bricks_y, bricks_x) of a fixed volume of ``shape`` (Z, Y, X)."""
    fz, fy, fx = (int(v) for v in shape)
    return -(-fz // BZ), -(-fy // BY), -(-fx // BX)


def pass_sizes(n_slabs):
    """Values per sum that enter each pass of the reduction: [n_slabs, ceil(n_slabs / 256), ..] down to the pass whose
    output is one value."""
    out = [int(n_slabs)]
    while out[-1] > FAN:
        out.append(-(-out[-1] // FAN))
    return out


def workspace_bytes(shape):
    """What t2fit_register_workspace_bytes returns: every pass's input, each rounded up to 256 bytes."""
    bz, by, bx = brick_counts(shape)
    return sum((N_SUMS * 8 * n + 255) // 256 * 256 for n in pass_sizes(bz * by * bx))


def _terms(fixed, fmask, moving, mmask, a, z0, nzc, coords=None):
    """float64 ``(43, nzc, fy, fx)``: what every voxel of the fixed planes ``z0 .. z0 + nzc`` adds to the sums.
    ``coords``: the moving coordinates ``(c_x, c_y, c_z)`` of those planes from the caller (:mod:`_ffd`), in place of
    ``A`` applied to the voxel index."""
    _, fy, fx = fixed.shape
    n = moving.shape[::-1]
    shape = (nzc, fy, fx)
    c = _resample._coords(a, shape, (0, 0, z0)) if coords is None else coords
    counted = fmask[z0:z0 + nzc] != 0
    for k in range(3):
        counted = counted & (c[k] >= -0.5) & (c[k] < n[k] - 0.5)
    near = [np.clip(np.floor(c[k] + 0.5), 0, n[k] - 1).astype(np.int64) for k in range(3)]
    counted = counted & (mmask[near[2], near[1], near[0]] != 0)
    b = [np.clip(np.floor(c[k]), 0, n[k] - 1) for k in range(3)]
    d = [np.maximum(c[k] - b[k], 0.0) for k in range(3)]
    lo = [b[k].astype(np.int64) for k in range(3)]
    hi = [np.minimum(lo[k] + 1, n[k] - 1) for k in range(3)]
    flat = [(hi[k] == lo[k]) | (c[k] < 0.0) for k in range(3)]
    v = moving.astype(np.float64)

    def lerp(p, q, w):
        return np.where(w == 0.0, p, p + w * (q - p))

    tap = {(z, y, x): v[(lo, hi)[z][2], (lo, hi)[y][1], (lo, hi)[x][0]] for z in (0, 1) for y in (0, 1) for x in (0, 1)}
    row = {(z, y): lerp(tap[z, y, 0], tap[z, y, 1], d[0]) for z in (0, 1) for y in (0, 1)}
    plane = [lerp(row[z, 0], row[z, 1], d[1]) for z in (0, 1)]
    m = lerp(plane[0], plane[1], d[2])
    gx = lerp(lerp(tap[0, 0, 1] - tap[0, 0, 0], tap[0, 1, 1] - tap[0, 1, 0], d[1]),
              lerp(tap[1, 0, 1] - tap[1, 0, 0], tap[1, 1, 1] - tap[1, 1, 0], d[1]), d[2])
    gy = lerp(row[0, 1] - row[0, 0], row[1, 1] - row[1, 0], d[2])
    gz = plane[1] - plane[0]
    g = [np.where(flat[k], 0.0, gk) for k, gk in enumerate((gx, gy, gz))]
    f = fixed[z0:z0 + nzc].astype(np.float64)
    u = [np.broadcast_to(np.arange(fx, dtype=np.float64)[None, None, :], shape),
         np.broadcast_to(np.arange(fy, dtype=np.float64)[None, :, None], shape),
         np.broadcast_to(np.arange(z0, z0 + nzc, dtype=np.float64)[:, None, None], shape)]
    out = np.zeros((N_SUMS,) + shape, np.float64)
    out[0], out[1], out[2], out[3], out[4], out[5] = 1.0, f, m, f * f, m * m, f * m
    for w, wv in enumerate((None, f, m)):
        for k in range(3):
            wg = g[k] if wv is None else wv * g[k]
            for j in range(4):
                out[6 + 4 * (3 * w + k) + j] = wg * u[j] if j < 3 else wg
    return np.where(counted[None], out, 0.0)


def _volumes(fixed, fixed_mask, moving, moving_mask):
    fixed, moving = np.asarray(fixed, np.float32), np.asarray(moving, np.float32)
    if fixed.ndim != 3 or moving.ndim != 3:
        raise ValueError("fixed and moving must be (Z, Y, X) volumes")
    fmask = np.ones(fixed.shape, np.uint8) if fixed_mask is None else (np.asarray(fixed_mask) != 0).astype(np.uint8)
    mmask = np.ones(moving.shape, np.uint8) if moving_mask is None else (np.asarray(moving_mask) != 0).astype(np.uint8)
    if fmask.shape != fixed.shape or mmask.shape != moving.shape:
        raise ValueError("a mask has the shape of its volume")
    return fixed, fmask, moving, mmask


def slabs(fixed, fixed_mask, moving, moving_mask, A):
    """float64 ``(43, n_slabs)``: the slab of every brick of the fixed volume, bricks in ``(bz, by, bx)`` order."""
    fixed, fmask, moving, mmask = _volumes(fixed, fixed_mask, moving, moving_mask)
    a = np.asarray(A, np.float64).reshape(3, 4)
    fz, fy, fx = fixed.shape
    nbz, nby, nbx = brick_counts(fixed.shape)
    out = np.zeros((N_SUMS, nbz, nby, nbx), np.float64)
    with np.errstate(all="ignore"):
        for bz in range(nbz):
            z0 = bz * BZ
            nzc = min(BZ, fz - z0)
            pad = np.zeros((N_SUMS, BZ, nby * BY, nbx * BX), np.float64)
            pad[:, :nzc, :fy, :fx] = _terms(fixed, fmask, moving, mmask, a, z0, nzc)
            acc = np.zeros(pad.shape[:1] + pad.shape[2:], np.float64)
            for k in range(BZ):
                acc = acc + pad[:, k]
            acc = _halve(acc.reshape(N_SUMS, nby, BY, nbx, BX))       # the 64 columns of a row
            out[:, bz] = _halve(np.moveaxis(acc, 2, -1))              # the 4 rows
    return out.reshape(N_SUMS, -1)


def reduce_slabs(v):
    """The passes of the tree over ``(43, n)`` values."""
    v = np.asarray(v, np.float64)
    while True:
        groups = -(-v.shape[1] // FAN)
        pad = np.zeros((v.shape[0], groups * FAN), np.float64)
        pad[:, :v.shape[1]] = v
        with np.errstate(all="ignore"):
            v = _halve(pad.reshape(v.shape[0], groups, FAN))
        if groups == 1:
            return v[:, 0]


def registration_sums(fixed, moving, A, fixed_mask=None, moving_mask=None):
    """The 43 float64 sums (module docstring) of ``moving`` sampled at ``A`` against ``fixed``; masks None: all ones."""
    return reduce_slabs(slabs(fixed, fixed_mask, moving, moving_mask, A))


# ---- metric: host arithmetic, shared by the statement and the device path --------------------------------------------
def metric(sums):
    """``(C, dC/dA [3, 4])`` from the 43 sums: ``C = -sfm^2 / (sff smm)`` with ``sfm = sum fm - sum f sum m / N`` (ITK's
    correlation metric), the derivative by the chain rule with N held constant.  ValueError when no voxel counts or a
    variance vanishes (no overlap, a constant volume): there is no metric there, and no transform is made up."""
    s = np.asarray(sums, np.float64)
    n = s[0]
    if not n >= 1.0:
        raise ValueError("the registration has no voxel to compare: the masks do not overlap under this transform")
    sf, sm, sff_, smm_, sfm_ = s[1:6]
    sfm, sff, smm = sfm_ - sf * sm / n, sff_ - sf * sf / n, smm_ - sm * sm / n
    if not (sff > 0.0 and smm > 0.0):
        raise ValueError("the registration metric is undefined: the fixed or the moving samples are constant")
    d1, df, dm = (s[6 + 12 * w:18 + 12 * w].reshape(3, 4) for w in range(3))
    dsfm = df - (sf / n) * d1
    dsmm = 2.0 * dm - 2.0 * (sm / n) * d1
    c = -(sfm * sfm) / (sff * smm)
    dc = -2.0 * sfm * dsfm / (sff * smm) + (sfm * sfm) * dsmm / (sff * smm * smm)
    return float(c), dc


# ---- transform: Euler angles about a centre ----------------------------------------------------------------------------
def _rotations(p):
    """R = Rz Rx Ry (ITK's Euler3DTransform order) and its derivatives with respect to (rx, ry, rz)."""
    cx, sx, cy, sy, cz, sz = np.cos(p[0]), np.sin(p[0]), np.cos(p[1]), np.sin(p[1]), np.cos(p[2]), np.sin(p[2])
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], np.float64)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], np.float64)
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], np.float64)
    dx = np.array([[0, 0, 0], [0, -sx, -cx], [0, cx, -sx]], np.float64)
    dy = np.array([[-sy, 0, cy], [0, 0, 0], [-cy, 0, -sy]], np.float64)
    dz = np.array([[-sz, -cz, 0], [cz, -sz, 0], [0, 0, 0]], np.float64)
    return rz @ rx @ ry, (rz @ dx @ ry, rz @ rx @ dy, dz @ rx @ ry)


def compose(p, centre):
    """4 x 4 (fixed point -> moving point, LPS millimetres) of ``p = (rx, ry, rz [rad], tx, ty, tz [mm])``:
    ``x' = R (x - centre) + centre + t``."""
    p, centre = np.asarray(p, np.float64), np.asarray(centre, np.float64)
    r, _ = _rotations(p)
    t = np.eye(4)
    t[:3, :3] = r
    t[:3, 3] = centre - r @ centre + p[3:]
    return t


def parameter_gradient(dc_da, p, centre, fixed_geom, moving_geom):
    """dC/dp from dC/dA: ``A = Mm^-1 [R Mf | R of + (centre - R centre + t) - om]`` is linear in R and t."""
    mf, of = _resample._index_to_point(fixed_geom)
    mm, _ = _resample._index_to_point(moving_geom)
    h = np.linalg.inv(mm).T @ np.asarray(dc_da, np.float64)
    d_r = h[:, :3] @ mf.T + np.outer(h[:, 3], of - np.asarray(centre, np.float64))
    _, dr = _rotations(np.asarray(p, np.float64))
    return np.array([np.sum(d_r * dr[0]), np.sum(d_r * dr[1]), np.sum(d_r * dr[2]), h[0, 3], h[1, 3], h[2, 3]])


def mask_centre_and_scales(fixed_mask, fixed_geom):
    """The rotation centre -- the centroid of the fixed mask, a physical point -- and the parameter scales: 1 for the
    translations; for the rotations the mean squared distance [mm^2] of the mask's voxels from the centre, which is what
    ITK's scales from the physical shift amount to for a rigid transform (a unit rotation shifts a voxel by its distance
    from the axis, a unit translation by 1; the scale is the mean squared shift)."""
    idx = np.argwhere(np.asarray(fixed_mask) != 0)[:, ::-1].astype(np.float64)  # (x, y, z)
    if len(idx) == 0:
        raise ValueError("the fixed mask is empty")
    m, o = _resample._index_to_point(fixed_geom)
    pts = idx @ m.T + o
    centre = pts.mean(axis=0)
    r2 = float(np.mean(np.sum((pts - centre) ** 2, axis=1)))
    return centre, np.array([r2, r2, r2, 1.0, 1.0, 1.0]) if r2 > 0.0 else np.ones(6)


# ---- pyramid ---------------------------------------------------------------------------------------------------------
def level_shape(shape, s):
    """(Z, Y, X) of a level of shrink factor ``s``: whole blocks only, the ragged edge is dropped."""
    return tuple(int(v) // int(s) for v in shape)


def level_geometry(geom, s, shape=None):
    """The grid of the block means: spacing ``s`` times as large, the origin at the centre of the first block."""
    g = _resample.as_geometry(geom, shape)
    m, o = _resample._index_to_point(g)
    origin = o + m @ np.full(3, (s - 1) / 2.0)
    return _resample.Geometry([v // s for v in g.GetSize()], [v * s for v in g.GetSpacing()], origin, g.GetDirection())


def shrink(vol, s):
    """Mean of the ``s^3`` blocks: a float64 sum in (dz, dy, dx) order from 0.0, divided by ``s^3``, one rounding to
    float32."""
    v = np.asarray(vol, np.float32).astype(np.float64)
    nz, ny, nx = level_shape(v.shape, s)
    acc = np.zeros((nz, ny, nx), np.float64)
    for dz in range(s):
        for dy in range(s):
            for dx in range(s):
                acc = acc + v[dz:nz * s:s, dy:ny * s:s, dx:nx * s:s]
    return (acc / float(s ** 3)).astype(np.float32)


def shrink_mask(mask, s):
    """1 where any voxel of the block is set."""
    m = np.asarray(mask) != 0
    nz, ny, nx = level_shape(m.shape, s)
    return m[:nz * s, :ny * s, :nx * s].reshape(nz, s, ny, s, nx, s).any(axis=(1, 3, 5)).astype(np.uint8)


def build_mask(vol, threshold=1.0, slice_axis=2, size=5, *, keep_largest=0, min_size=0, connectivity=1):
    """The reference's ``build_mask`` (utils/qmri_utils.py:223-252) with :mod:`_morph`, as ``_gpu_morph.build_mask``;
    ``min_size`` and ``keep_largest`` (off by default) clean the 3-D result with :mod:`_components`."""
    fp = [size, size, size]
    fp[slice_axis] = 1
    square = np.ones(fp, bool)
    m = _morph.fill_holes(np.asarray(vol, np.float32) > np.float32(threshold), slice_axis=slice_axis)
    m = _morph.erode(_morph.dilate(m, square), square).astype(np.uint8)
    if min_size:
        m = _components.remove_small(m, min_size, connectivity)
    if keep_largest:
        m = _components.keep_largest(m, keep_largest, connectivity)
    return m


def check_levels(levels, fixed_shape, moving_shape):
    levels = tuple(int(s) for s in levels)
    if not levels or any(s < 1 or s > 32 for s in levels):
        raise ValueError(f"levels are shrink factors in 1..32, got {levels!r}")
    for s in levels:
        if min(level_shape(fixed_shape, s) + level_shape(moving_shape, s)) < MIN_LEVEL_SIZE:
            raise ValueError(f"shrink factor {s} leaves fewer than {MIN_LEVEL_SIZE} voxels along an axis of "
                             f"{tuple(fixed_shape)} / {tuple(moving_shape)}")
    return levels


class HostPyramid:
    """The volumes and masks of every level, and their sums, in numpy.  The device path has the same two methods."""

    def __init__(self, fixed, fixed_mask, moving, moving_mask):
        self.full = _volumes(fixed, fixed_mask, moving, moving_mask)

    def level(self, s):
        fixed, fmask, moving, mmask = self.full
        if s == 1:
            return self.full
        return shrink(fixed, s), shrink_mask(fmask, s), shrink(moving, s), shrink_mask(mmask, s)

    def sums(self, level, A):
        fixed, fmask, moving, mmask = level
        return registration_sums(fixed, moving, A, fmask, mmask)


# ---- optimizer -------------------------------------------------------------------------------------------------------
class Registration:
    """``transform`` 4 x 4 (fixed point -> moving point, LPS millimetres: what ``recon.py --transforms`` reads),
    ``parameters`` (rx, ry, rz, tx, ty, tz) about ``centre``, ``metric`` at the returned parameters, ``iterations`` per
    level, ``stop``: why the last level ended ('gradient', 'step' or 'iterations'), ``stops``: every level's."""

    def __init__(self, transform, parameters, centre, metric, iterations, stops):  # noqa: A002
        self.transform, self.parameters, self.centre, self.metric = transform, parameters, centre, metric
        self.iterations, self.stops, self.stop = tuple(iterations), tuple(stops), stops[-1]

    def __repr__(self):
        return (f"Registration(parameters={np.array2string(self.parameters, precision=5)}, metric={self.metric:.6f}, "
                f"iterations={self.iterations}, stop={self.stop!r})")


def initial_step(s):
    """The first step [mm in scaled parameter space] of a level of shrink factor ``s``: ``registration_itk``'s learning
    rate 1 at full resolution, ``s`` times as long on a grid ``s`` times as coarse (a step of one voxel at every level)."""
    return LEARNING_RATE * float(s)


def optimize(pyramid, fixed_geom, moving_geom, centre, scales, *, levels=(4, 2, 1), max_iter=100, init=None):
    """Regular-step gradient descent over the levels.  Per iteration: the sums at ``A(p)``, ``C`` and ``dC/dp``, the scaled
    gradient ``g_i = (dC/dp_i) / scale_i``; stop when ``|g| < 1e-6`` ('gradient'); halve the step when ``g`` and the
    previous ``g`` have a negative scalar product; stop when the step is below 1e-6 ('step'); move
    ``p -= step g / |g|``; stop after ``max_iter`` moves ('iterations').  The parameters carry from level to level."""
    p = np.zeros(6) if init is None else np.array(init, np.float64)
    if p.shape != (6,) or not np.all(np.isfinite(p)):
        raise ValueError("init is (rx, ry, rz [rad], tx, ty, tz [mm]), finite")
    iterations, stops = [], []
    for s in levels:
        level = pyramid.level(s)
        fg, mg = level_geometry(fixed_geom, s), level_geometry(moving_geom, s)

        def evaluate(q):
            a = _resample.index_affine(fg, mg, compose(q, centre))
            c, dc = metric(pyramid.sums(level, a))
            return c, parameter_gradient(dc, q, centre, fg, mg) / scales

        step, prev, n_it, stop = initial_step(s), None, 0, "iterations"
        while True:
            c, g = evaluate(p)
            norm = float(np.sqrt(np.sum(g * g)))
            if norm < GRAD_TOL:
                stop = "gradient"
                break
            if prev is not None and float(np.sum(g * prev)) < 0.0:
                step *= RELAX
            if step < MIN_STEP:
                stop = "step"
                break
            if n_it >= max_iter:
                break
            p = p - (step / norm) * g
            prev, n_it = g, n_it + 1
        iterations.append(n_it)
        stops.append(stop)
    return Registration(compose(p, centre), p, np.asarray(centre, np.float64), c, iterations, stops)


def check_rigid_metric(metric):  # noqa: A002
    if metric not in ("corr", "mattes"):
        raise ValueError(f"metric is 'corr' or 'mattes', got {metric!r}")
    return metric


def rigid_from_affine(found):
    """The :class:`Registration` of :func:`register_rigid` (six parameters) from a 6-dof one of :func:`register_affine`."""
    p = found.parameters[:6].copy()
    return Registration(compose(p, found.centre), p, found.centre, found.metric, found.iterations, found.stops)


def rigid_init(init):
    """The 12 parameters :func:`register_affine` starts from, given the six of :func:`register_rigid` (or None)."""
    if init is None:
        return None
    p = np.array(init, np.float64)
    if p.shape != (6,) or not np.all(np.isfinite(p)):
        raise ValueError("init is (rx, ry, rz [rad], tx, ty, tz [mm]), finite")
    return np.concatenate([p, np.zeros(6)])


def register_rigid(fixed, moving, fixed_geom, moving_geom, *, fixed_mask=None, moving_mask=None, levels=(4, 2, 1),
                   max_iter=100, init=None, metric="corr", bins=32, moving_bins=32):  # noqa: A002
    """Register ``moving`` onto ``fixed`` (float32 ``(Z, Y, X)`` with their geometries); masks None: ``build_mask`` of
    the volume.  ``metric``: 'corr' (the squared correlation) or 'mattes' (Mattes mutual information, through
    :func:`register_affine` with 6 degrees of freedom, ``bins`` fixed and ``moving_bins`` moving bins).  Returns a
    :class:`Registration`.  The statement of ``t2map.register.register_rigid``."""
    fixed, moving = np.asarray(fixed, np.float32), np.asarray(moving, np.float32)
    fmask = build_mask(fixed) if fixed_mask is None else fixed_mask
    mmask = build_mask(moving) if moving_mask is None else moving_mask
    if check_rigid_metric(metric) == "mattes":
        return rigid_from_affine(register_affine(fixed, moving, fixed_geom, moving_geom, metric="mattes", bins=bins,
                                                 moving_bins=moving_bins, dof=6, fixed_mask=fmask, moving_mask=mmask, levels=levels,
                                                 max_iter=max_iter, init=rigid_init(init)))
    pyramid = HostPyramid(fixed, fmask, moving, mmask)
    fg, mg = _resample.as_geometry(fixed_geom, fixed.shape), _resample.as_geometry(moving_geom, moving.shape)
    levels = check_levels(levels, fixed.shape, moving.shape)
    centre, scales = mask_centre_and_scales(pyramid.full[1], fg)
    return optimize(pyramid, fg, mg, centre, scales, levels=levels, max_iter=max_iter, init=init)


def target_registration_error(found, true, mask, geom):
    """The largest distance [mm] between the images of the mask's voxels under two 4 x 4 transforms."""
    idx = np.argwhere(np.asarray(mask) != 0)[:, ::-1].astype(np.float64)
    m, o = _resample._index_to_point(_resample.as_geometry(geom, np.asarray(mask).shape))
    pts = idx @ m.T + o
    d = pts @ (np.asarray(found)[:3, :3] - np.asarray(true)[:3, :3]).T + (np.asarray(found)[:3, 3] - np.asarray(true)[:3, 3])
    return float(np.sqrt(np.max(np.sum(d * d, axis=1))))


# ---- correlation ratio: the cross-contrast metric of the affine registration ---------------------------------------------
# The statement of include/t2fit.h's t2fit_register_bin_dev, t2fit_register_binned_sums_dev and
# t2fit_register_sums_lut_dev.  The fixed volume is binned once per level; N_b and S_b are the count and the sum of the
# interpolated moving samples over the counted voxels of bin b, by the tree of the 43 sums; lut[b] = S_b / N_b; the 43
# sums with f = lut[bin] give, through metric(), C = CR - 1 and dC/dA with the voxel set held fixed (lut maximises the
# correlation over the functions constant on each bin, so its own derivative drops out).
MAX_BINS = 64
_correlation = metric  # (register_affine has a ``metric`` argument)


def _check_bins(n_bins):
    n_bins = int(n_bins)
    if not 1 <= n_bins <= MAX_BINS:
        raise ValueError(f"n_bins is in 1..{MAX_BINS}, got {n_bins}")
    return n_bins


def bin_range(fixed, fixed_mask, n_bins):
    """``(lo, scale)`` of a level: ``lo`` / ``hi`` the smallest / largest fixed sample inside the mask,
    ``scale = n_bins / (hi - lo)`` in float64, 0 when ``hi == lo``.  ValueError on an empty mask."""
    inside = np.asarray(fixed, np.float32)[np.asarray(fixed_mask) != 0]
    if inside.size == 0:
        raise ValueError("the fixed mask is empty")
    lo, hi = float(inside.min()), float(inside.max())
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError("the fixed volume is not finite inside its mask")
    return lo, (float(_check_bins(n_bins)) / (hi - lo) if hi > lo else 0.0)


def bin_volume(vol, lo, scale, n_bins):
    """uint8 ``clamp(floor((float64(vol) - lo) * scale), 0, n_bins - 1)``, each operation rounding once; NaN gives 0."""
    n_bins = _check_bins(n_bins)
    with np.errstate(all="ignore"):
        b = np.floor((np.asarray(vol, np.float32).astype(np.float64) - float(lo)) * float(scale))
        return np.where(b > 0.0, np.minimum(b, float(n_bins - 1)), 0.0).astype(np.uint8)


def _bins_and_masks(bins, fixed_mask, moving, moving_mask, n_bins):
    bins = np.minimum(np.asarray(bins, np.uint8), np.uint8(_check_bins(n_bins) - 1))
    if bins.ndim != 3:
        raise ValueError("bins is a (Z, Y, X) uint8 volume")
    _, fmask, moving, mmask = _volumes(np.zeros(bins.shape, np.float32), fixed_mask, moving, moving_mask)
    return bins, fmask, moving, mmask


def _tree(shape, n_rows, terms):
    """The summation tree over ``n_rows`` kinds of terms of a fixed volume of ``shape``; ``terms(z0, nzc)`` gives the
    float64 ``(n_rows, nzc, fy, fx)`` of the planes ``z0 .. z0 + nzc``."""
    fz, fy, fx = shape
    nbz, nby, nbx = brick_counts(shape)
    out = np.zeros((n_rows, nbz, nby, nbx), np.float64)
    with np.errstate(all="ignore"):
        for bz in range(nbz):
            z0 = bz * BZ
            nzc = min(BZ, fz - z0)
            t = terms(z0, nzc)
            for r0 in range(0, n_rows, 16):  # (rows in groups: the padded copy of a thin, long volume is large)
                r = min(16, n_rows - r0)
                pad = np.zeros((r, BZ, nby * BY, nbx * BX), np.float64)
                pad[:, :nzc, :fy, :fx] = t[r0:r0 + r]
                acc = np.zeros(pad.shape[:1] + pad.shape[2:], np.float64)
                for k in range(BZ):
                    acc = acc + pad[:, k]
                acc = _halve(acc.reshape(r, nby, BY, nbx, BX))
                out[r0:r0 + r, bz] = _halve(np.moveaxis(acc, 2, -1))
    return reduce_slabs(out.reshape(n_rows, -1))


def binned_sums(bins, moving, A, n_bins, fixed_mask=None, moving_mask=None):
    """float64 ``[2 n_bins]``: ``N_b`` then ``S_b``.  A counted voxel adds ``(1.0, m)`` to its own bin and +0.0 to every
    other; counting rule, ``m`` and tree as for the 43 sums.  A bin byte above ``n_bins - 1`` counts as ``n_bins - 1``."""
    bins, fmask, moving, mmask = _bins_and_masks(bins, fixed_mask, moving, moving_mask, n_bins)
    a = np.asarray(A, np.float64).reshape(3, 4)
    zero = np.zeros(bins.shape, np.float32)
    which = np.arange(n_bins, dtype=np.uint8)[:, None, None, None]

    def terms(z0, nzc):
        t = _terms(zero, fmask, moving, mmask, a, z0, nzc)
        own = bins[None, z0:z0 + nzc] == which
        return np.concatenate([np.where(own, t[0][None], 0.0), np.where(own, t[2][None], 0.0)])

    return _tree(bins.shape, 2 * n_bins, terms)


def lut_from_binned(binned):
    """``lut[b] = S_b / N_b`` where ``N_b > 0``, else 0.0."""
    b = np.asarray(binned, np.float64)
    n, s = b[:b.size // 2], b[b.size // 2:]
    with np.errstate(all="ignore"):
        return np.where(n > 0.0, s / np.where(n > 0.0, n, 1.0), 0.0)


def registration_sums_lut(bins, lut, moving, A, fixed_mask=None, moving_mask=None):
    """The 43 sums with ``f = lut[bins]``, a float64 that is not rounded to float32: the tree of
    :func:`registration_sums` over the same terms."""
    lut = np.asarray(lut, np.float64).ravel()
    bins, fmask, moving, mmask = _bins_and_masks(bins, fixed_mask, moving, moving_mask, lut.size)
    a = np.asarray(A, np.float64).reshape(3, 4)
    f = lut[bins]
    return _tree(bins.shape, N_SUMS, lambda z0, nzc: _terms(f, fmask, moving, mmask, a, z0, nzc))


def cr_metric(binned, sums_lut):
    """``(CR, dC/dA [3, 4])``: the correlation ratio ``1 + C`` of the moving samples given the binned fixed ones, and
    the derivative with the voxel set held fixed -- :func:`metric` of the 43 sums with ``f = lut[bin]``.  ``binned`` must
    be the ``N_b, S_b`` those sums' table came from (their counts must add up to the sums' N)."""
    b = np.asarray(binned, np.float64)
    if b.ndim != 1 or b.size % 2 or float(np.sum(b[:b.size // 2])) != float(np.asarray(sums_lut)[0]):
        raise ValueError("binned is [2 n_bins] and its counts add up to the N of sums_lut")
    c, dc = metric(sums_lut)
    return 1.0 + c, dc


# ---- Mattes mutual information: the cost elastix's default rigid map minimises -----------------------------------------
# The statement of include/t2fit.h's t2fit_register_joint_hist_dev and t2fit_register_mi_gradient_dev.  The fixed side
# is the uint8 bin volume above (a zero-order window); the moving sample m goes through a cubic B-spline Parzen window
# over n_m bins, two of them padding at each end (ITK's layout).  The joint histogram is made of integers (weights in
# units of 2^-30), so its sums are exact in any order; the gradient's 12 sums go through the tree of the 43.
MIN_MOVING_BINS = 5
N_MI_SUMS = 12
HIST_ONE = float(1 << 30)  # a weight of 1.0 in the histogram's units


def _check_moving_bins(n_m):
    n_m = int(n_m)
    if not MIN_MOVING_BINS <= n_m <= MAX_BINS:
        raise ValueError(f"moving_bins is in {MIN_MOVING_BINS}..{MAX_BINS}, got {n_m}")
    return n_m


def moving_bin_range(moving, moving_mask, n_m):
    """``(lo_m, scale_m)`` of a level: ``lo_m`` / ``hi_m`` the smallest / largest moving sample inside the moving mask,
    ``scale_m = (n_m - 4) / (hi_m - lo_m)`` in float64, 0 when they are equal.  ValueError on an empty mask."""
    inside = np.asarray(moving, np.float32)[np.asarray(moving_mask) != 0]
    if inside.size == 0:
        raise ValueError("the moving mask is empty")
    lo, hi = float(inside.min()), float(inside.max())
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError("the moving volume is not finite inside its mask")
    return lo, (float(_check_moving_bins(n_m) - 4) / (hi - lo) if hi > lo else 0.0)


def parzen_window(m, lo_m, scale_m, n_m):
    """``(i0, w [4], dw [4])`` of float64 moving samples ``m``: ``t = (m - lo_m) * scale_m + 2`` kept in ``[2, n_m - 2]``
    (anything else, a NaN too, becomes the nearer end: 2 for a NaN), ``i0 = min(floor(t), n_m - 3)``, ``u = t - i0``, and
    on the bins ``i0 - 1 .. i0 + 2`` the uniform cubic B-spline basis in ``u`` and its derivative with respect to ``t``,
    in the header's order of operations (``v = 1 - u``, ``u2 = u u``, ``u3 = u2 u``, ``v2 = v v``, ``v3 = v2 v``)."""
    with np.errstate(all="ignore"):
        t = (np.asarray(m, np.float64) - float(lo_m)) * float(scale_m) + 2.0
        t = np.where(t >= 2.0, t, 2.0)
        t = np.where(t <= float(n_m - 2), t, float(n_m - 2))
        base = np.minimum(np.floor(t), float(n_m - 3))
        u = t - base
        v = 1.0 - u
        u2, v2 = u * u, v * v
        u3, v3 = u2 * u, v2 * v
        w = [v3 / 6.0, ((3.0 * u3 - 6.0 * u2) + 4.0) / 6.0, (((-3.0 * u3 + 3.0 * u2) + 3.0 * u) + 1.0) / 6.0, u3 / 6.0]
        dw = [-(v2 * 0.5), 1.5 * u2 - 2.0 * u, (-1.5 * u2 + u) + 0.5, u2 * 0.5]
    return base.astype(np.int64), w, dw


def _mi_bins(bins, fixed_mask, moving, moving_mask, n_f, n_m):
    if bins is not None and np.asarray(bins).size > 1 << 32:
        raise ValueError("the fixed volume has more than 2^32 voxels: a histogram entry could pass 2^63")
    return _bins_and_masks(bins, fixed_mask, moving, moving_mask, n_f) + (_check_moving_bins(n_m),)


def joint_histogram(bins, moving, A, n_f, n_m, lo_m, scale_m, fixed_mask=None, moving_mask=None):
    """uint64 ``(n_f, n_m)``: a counted voxel of fixed bin ``b`` adds ``floor(w_j 2^30 + 0.5)`` to ``H[b][i0 - 1 + j]``,
    ``j = 0..3`` (:func:`parzen_window` of its interpolant ``m``).  Counting rule and ``m`` as for the 43 sums; integer
    sums, exact in any order."""
    bins, fmask, moving, mmask, n_m = _mi_bins(bins, fixed_mask, moving, moving_mask, n_f, n_m)
    a = np.asarray(A, np.float64).reshape(3, 4)
    zero = np.zeros(bins.shape, np.float32)
    hist = np.zeros(n_f * n_m, np.uint64)
    for z0 in range(0, bins.shape[0], BZ):
        nzc = min(BZ, bins.shape[0] - z0)
        with np.errstate(all="ignore"):
            t = _terms(zero, fmask, moving, mmask, a, z0, nzc)
        counted = t[0] != 0.0
        i0, w, _ = parzen_window(t[2][counted], lo_m, scale_m, n_m)
        row = bins[z0:z0 + nzc][counted].astype(np.int64) * n_m
        for j in range(4):
            np.add.at(hist, row + i0 - 1 + j, np.floor(w[j] * HIST_ONE + 0.5).astype(np.uint64))
    return hist.reshape(n_f, n_m)


def mattes_metric(hist, n_f, n_m, scale_m):
    """``(cost, table)`` from the joint histogram: with ``p = H / sum H`` and its marginals ``p_f``, ``p_m``, the cost is
    ``-MI = -sum_{p > 0} p log(p / (p_f p_m))`` and ``table[b][k] = -(scale_m 2^30 / sum H) log(p / p_m)`` where ``p > 0``,
    0 elsewhere: ``sum H 2^-30`` is the histogram's total in units of one voxel, and with the counted set held fixed (``p_f``
    constant, ``sum dp = 0``) ``d(-MI)/dt_v = sum_j table[b_v][i0 - 1 + j] w'_j(u_v)``.  Host arithmetic, shared by the
    statement and the device path.  ValueError when the histogram is empty: no voxel counts."""
    n_f, n_m = _check_bins(n_f), _check_moving_bins(n_m)
    h = np.asarray(hist)
    if h.shape != (n_f, n_m) or h.dtype != np.uint64:
        raise ValueError("hist is uint64 (n_f, n_m)")
    total = sum(int(v) for v in h.ravel().tolist())
    if total == 0:
        raise ValueError("the registration has no voxel to compare: the masks do not overlap under this transform")
    p = h.astype(np.float64) / float(total)
    pf, pm = p.sum(axis=1), p.sum(axis=0)
    some = p > 0.0
    with np.errstate(all="ignore"):
        mi = float(np.sum(np.where(some, p * np.log(np.where(some, p / (pf[:, None] * pm[None, :]), 1.0)), 0.0)))
        table = np.where(some, -(float(scale_m) * HIST_ONE / float(total)) * np.log(np.where(some, p / pm[None, :], 1.0)), 0.0)
    return -mi, np.ascontiguousarray(table, np.float64)


def mi_gradient_sums(bins, table, moving, A, n_m, lo_m, scale_m, fixed_mask=None, moving_mask=None):
    """float64 ``[12]``: ``[4 a + j] = sum (c g_a) u_j`` over the counted voxels, ``c = sum_j table[b][i0 - 1 + j] w'_j(u)``
    (the four products added in ``j`` order from 0.0), ``c g_a`` rounded first, then ``u_j`` (``u_3 = 1`` is no
    multiplication); a voxel that does not count adds +0.0; the tree of the 43 sums.  With :func:`mattes_metric`'s
    table this is ``d(-MI)/dA``."""
    table = np.asarray(table, np.float64)
    if table.ndim != 2 or table.shape[1] != int(n_m):
        raise ValueError("table is float64 (n_f, n_m)")
    n_f = table.shape[0]
    bins, fmask, moving, mmask, n_m = _mi_bins(bins, fixed_mask, moving, moving_mask, n_f, n_m)
    a = np.asarray(A, np.float64).reshape(3, 4)
    zero = np.zeros(bins.shape, np.float32)
    flat = table.ravel()

    def terms(z0, nzc):
        t = _terms(zero, fmask, moving, mmask, a, z0, nzc)
        counted = t[0] != 0.0
        i0, _, dw = parzen_window(np.where(counted, t[2], float(lo_m)), lo_m, scale_m, n_m)
        at = bins[z0:z0 + nzc].astype(np.int64) * n_m + i0 - 1
        c = np.zeros(counted.shape, np.float64)
        for j in range(4):
            c = c + flat[at + j] * dw[j]
        out = np.zeros((N_MI_SUMS,) + counted.shape, np.float64)
        for k in range(3):
            cg = c * t[6 + 4 * k + 3]                 # g_k: the "1 g_k 1" term of the 43
            for j in range(4):
                out[4 * k + j] = cg * _index(j, z0, counted.shape) if j < 3 else cg
        return np.where(counted[None], out, 0.0)

    return _tree(bins.shape, N_MI_SUMS, terms)


def _index(j, z0, shape):
    """``u_j`` (0: ix, 1: iy, 2: iz) of the planes ``z0 ..`` as float64, broadcast to ``shape`` (nzc, fy, fx)."""
    nzc, fy, fx = shape
    if j == 0:
        return np.broadcast_to(np.arange(fx, dtype=np.float64)[None, None, :], shape)
    if j == 1:
        return np.broadcast_to(np.arange(fy, dtype=np.float64)[None, :, None], shape)
    return np.broadcast_to(np.arange(z0, z0 + nzc, dtype=np.float64)[:, None, None], shape)


def mattes_cost_and_gradient(bins, moving, A, n_f, n_m, lo_m, scale_m, fixed_mask=None, moving_mask=None):
    """``(-MI, d(-MI)/dA [3, 4])`` at ``A``: :func:`joint_histogram`, :func:`mattes_metric`, :func:`mi_gradient_sums`."""
    cost, table = mattes_metric(joint_histogram(bins, moving, A, n_f, n_m, lo_m, scale_m, fixed_mask, moving_mask), n_f, n_m, scale_m)
    return cost, mi_gradient_sums(bins, table, moving, A, n_m, lo_m, scale_m, fixed_mask, moving_mask).reshape(3, 4)


# ---- affine transform: rotation, translation, log scales, shears ---------------------------------------------------------
N_AFFINE = 12
DOFS = (6, 7, 9, 12)


def _stretch(p):
    """K = [[e^s0, h01, h02], [0, e^s1, h12], [0, 0, e^s2]] and its derivatives with respect to p[6:12]."""
    e = np.exp(p[6:9])
    k = np.array([[e[0], p[9], p[10]], [0.0, e[1], p[11]], [0.0, 0.0, e[2]]], np.float64)
    dk = []
    for i in range(3):
        d = np.zeros((3, 3))
        d[i, i] = e[i]
        dk.append(d)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        d = np.zeros((3, 3))
        d[i, j] = 1.0
        dk.append(d)
    return k, dk


def compose_affine(p, centre):
    """4 x 4 (fixed point -> moving point, LPS millimetres) of ``p = (rx, ry, rz, tx, ty, tz, s0, s1, s2, h01, h02,
    h12)``: ``x' = R K (x - centre) + centre + t`` with R of :func:`compose` and K upper triangular, ``e^s`` on its
    diagonal."""
    p, centre = np.asarray(p, np.float64), np.asarray(centre, np.float64)
    r, _ = _rotations(p)
    k, _ = _stretch(p)
    t = np.eye(4)
    t[:3, :3] = r @ k
    t[:3, 3] = centre - t[:3, :3] @ centre + p[3:6]
    return t


def affine_parameter_gradient(dc_da, p, centre, fixed_geom, moving_geom):
    """dC/dp [12] from dC/dA: ``A = Mm^-1 [L Mf | L (of - centre) + centre + t - om]`` is linear in ``L = R K`` and t."""
    p = np.asarray(p, np.float64)
    mf, of = _resample._index_to_point(fixed_geom)
    mm, _ = _resample._index_to_point(moving_geom)
    h = np.linalg.inv(mm).T @ np.asarray(dc_da, np.float64)
    d_l = h[:, :3] @ mf.T + np.outer(h[:, 3], of - np.asarray(centre, np.float64))
    r, dr = _rotations(p)
    k, dk = _stretch(p)
    return np.array([np.sum(d_l * (d @ k)) for d in dr] + [h[0, 3], h[1, 3], h[2, 3]] + [np.sum(d_l * (r @ d)) for d in dk])


def affine_centre_and_scales(fixed_mask, fixed_geom):
    """The centre and the rotation / translation scales of :func:`mask_centre_and_scales`, and by the same rule (the mean
    squared shift of a mask point under a unit change) for ``s_a`` the mean square of component ``a`` of (mask point -
    centre), for ``h_ij`` that of component ``j``.  A vanishing scale is 1."""
    centre, rigid = mask_centre_and_scales(fixed_mask, fixed_geom)
    idx = np.argwhere(np.asarray(fixed_mask) != 0)[:, ::-1].astype(np.float64)
    m, o = _resample._index_to_point(fixed_geom)
    ms = np.mean((idx @ m.T + o - centre) ** 2, axis=0)
    scales = np.concatenate([rigid, ms, [ms[1], ms[2], ms[2]]])
    return centre, np.where(scales > 0.0, scales, 1.0)


def dof_basis(dof):
    """``[12, dof]``: the parameters are ``p = E q``.  6: rigid; 7: one scale, the three ``s`` tied; 9: three scales; 12."""
    if dof not in DOFS:
        raise ValueError(f"dof is one of {DOFS}, got {dof!r}")
    e = np.zeros((N_AFFINE, dof))
    e[:6, :6] = np.eye(6)
    if dof == 7:
        e[6:9, 6] = 1.0
    else:
        e[6:dof, 6:dof] = np.eye(dof - 6)
    return e


class HostAffinePyramid(HostPyramid):
    """:class:`HostPyramid` and the correlation ratio's two steps; the device path has the same methods."""

    def bins(self, level, n_bins):
        fixed, fmask = level[0], level[1]
        lo, scale = bin_range(fixed, fmask, n_bins)
        return bin_volume(fixed, lo, scale, n_bins)

    def cr_sums(self, level, bins, n_bins, A):
        _, fmask, moving, mmask = level[:4]
        binned = binned_sums(bins, moving, A, n_bins, fmask, mmask)
        return binned, registration_sums_lut(bins, lut_from_binned(binned), moving, A, fmask, mmask)

    def moving_range(self, level, n_m):
        return moving_bin_range(level[2], level[3], n_m)

    def joint_hist(self, level, bins, n_f, n_m, lo_m, scale_m, A):
        _, fmask, moving, mmask = level[:4]
        return joint_histogram(bins, moving, A, n_f, n_m, lo_m, scale_m, fmask, mmask)

    def mi_sums(self, level, bins, table, n_m, lo_m, scale_m, A):
        _, fmask, moving, mmask = level[:4]
        return mi_gradient_sums(bins, table, moving, A, n_m, lo_m, scale_m, fmask, mmask)


def optimize_affine(pyramid, fixed_geom, moving_geom, centre, scales, *, metric="cr", bins=32, dof=12, levels=(4, 2, 1),  # noqa: A002
                    max_iter=100, init=None, moving_bins=32):
    """The regular-step descent of :func:`optimize` over ``q`` with ``p = E q`` (:func:`dof_basis`): the gradient is
    ``E^T dC/dp``, a tied parameter's scale the sum of its members'.  ``metric``: 'cr' (each level's bins come from that
    level's fixed volume inside its mask), 'ncc' (the 43 sums as they are) or 'mattes' (Mattes mutual information: the
    fixed bins of 'cr' and ``moving_bins`` cubic B-spline bins over each level's moving samples inside its mask).
    ``init``: 12 parameters."""
    if metric not in ("cr", "ncc", "mattes"):
        raise ValueError(f"metric is 'cr', 'ncc' or 'mattes', got {metric!r}")
    n_bins = _check_bins(bins)
    n_m = _check_moving_bins(moving_bins)
    e = dof_basis(dof)
    p0 = np.zeros(N_AFFINE) if init is None else np.array(init, np.float64)
    if p0.shape != (N_AFFINE,) or not np.all(np.isfinite(p0)):
        raise ValueError("init is (rx, ry, rz, tx, ty, tz, s0, s1, s2, h01, h02, h12), finite")
    q_scales = e.T @ np.asarray(scales, np.float64)
    q = np.zeros(dof)
    iterations, stops = [], []
    for s in levels:
        level = pyramid.level(s)
        fg, mg = level_geometry(fixed_geom, s), level_geometry(moving_geom, s)
        level_bins = pyramid.bins(level, n_bins) if metric != "ncc" else None
        lo_m, scale_m = pyramid.moving_range(level, n_m) if metric == "mattes" else (0.0, 0.0)

        def evaluate(q):
            p = p0 + e @ q
            a = _resample.index_affine(fg, mg, compose_affine(p, centre))
            if metric == "mattes":
                c, table = mattes_metric(pyramid.joint_hist(level, level_bins, n_bins, n_m, lo_m, scale_m, a), n_bins, n_m, scale_m)
                dc = np.asarray(pyramid.mi_sums(level, level_bins, table, n_m, lo_m, scale_m, a), np.float64).reshape(3, 4)
            else:
                c, dc = cr_metric(*pyramid.cr_sums(level, level_bins, n_bins, a)) if metric == "cr" else _correlation(
                    pyramid.sums(level, a))
            return c, (e.T @ affine_parameter_gradient(dc, p, centre, fg, mg)) / q_scales

        step, prev, n_it, stop = initial_step(s), None, 0, "iterations"
        while True:
            c, g = evaluate(q)
            norm = float(np.sqrt(np.sum(g * g)))
            if norm < GRAD_TOL:
                stop = "gradient"
                break
            if prev is not None and float(np.sum(g * prev)) < 0.0:
                step *= RELAX
            if step < MIN_STEP:
                stop = "step"
                break
            if n_it >= max_iter:
                break
            q = q - (step / norm) * g
            prev, n_it = g, n_it + 1
        iterations.append(n_it)
        stops.append(stop)
    p = p0 + e @ q
    return Registration(compose_affine(p, centre), p, np.asarray(centre, np.float64), c, iterations, stops)


def mask_centroid(mask, geom):
    """The physical centroid of a mask's voxels."""
    idx = np.argwhere(np.asarray(mask) != 0)[:, ::-1].astype(np.float64)
    if len(idx) == 0:
        raise ValueError("the mask is empty")
    m, o = _resample._index_to_point(geom)
    return (idx @ m.T + o).mean(axis=0)


def affine_init(init, fixed_mask, fixed_geom, moving_mask, moving_geom):
    """None: zeros; 'centroids': the translation that takes the fixed mask's centroid onto the moving mask's (a template
    and a subject do not share a frame); else 12 parameters."""
    if init is None:
        return np.zeros(N_AFFINE)
    if isinstance(init, str):
        if init != "centroids":
            raise ValueError(f"init is None, 'centroids' or 12 parameters, got {init!r}")
        p = np.zeros(N_AFFINE)
        p[3:6] = mask_centroid(moving_mask, moving_geom) - mask_centroid(fixed_mask, fixed_geom)
        return p
    return np.array(init, np.float64)


def register_affine(fixed, moving, fixed_geom, moving_geom, *, metric="cr", bins=32, dof=12, fixed_mask=None,  # noqa: A002
                    moving_mask=None, levels=(4, 2, 1), max_iter=100, init=None, moving_bins=32):
    """Register ``moving`` onto ``fixed`` with up to 12 degrees of freedom and the correlation ratio ('cr', for volumes
    of different contrast), the squared correlation ('ncc') or Mattes mutual information ('mattes', ``bins`` fixed and
    ``moving_bins`` moving bins).  Masks None: ``build_mask`` of the volume.  Returns a
    :class:`Registration` whose ``parameters`` are the 12 of :func:`compose_affine`.  The statement of
    ``t2map.register.register_affine``."""
    fixed, moving = np.asarray(fixed, np.float32), np.asarray(moving, np.float32)
    fmask = build_mask(fixed) if fixed_mask is None else fixed_mask
    mmask = build_mask(moving) if moving_mask is None else moving_mask
    pyramid = HostAffinePyramid(fixed, fmask, moving, mmask)
    fg, mg = _resample.as_geometry(fixed_geom, fixed.shape), _resample.as_geometry(moving_geom, moving.shape)
    levels = check_levels(levels, fixed.shape, moving.shape)
    centre, scales = affine_centre_and_scales(pyramid.full[1], fg)
    p0 = affine_init(init, pyramid.full[1], fg, pyramid.full[3], mg)
    return optimize_affine(pyramid, fg, mg, centre, scales, metric=metric, bins=bins, dof=dof, levels=levels,
                           max_iter=max_iter, init=p0, moving_bins=moving_bins)
