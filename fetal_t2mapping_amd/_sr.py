"""Super-resolution reconstruction of thick-slice stacks, restated in numpy: the executable statement of the
definition in include/t2fit.h (t2fit_sr_plan_host, t2fit_sr_forward_dev, t2fit_sr_adjoint_dev).  Each thick slice is
modelled as the slice-profile average of the 1 mm volume x; the reconstruction inverts that model per echo,

    minimise  1/2 sum_s ||A_s x - y_s||^2  +  weight * TV(x)        (TV: isotropic, forward differences, as _tv.py)

by proximal gradient from the averaged merge: ``x <- prox(x - tau sum_s A_s^T (A_s x - y_s))``.  The prox of
``tau * weight * TV`` is :func:`_tv.denoise_tv` with ``dims=3``, whose ``weight`` w stands for exactly one times TV (its
fixed point minimises ``1/2 ||u - f||^2 + w TV(u)``: substitute p = w q in the update of :func:`_tv.update` and Chambolle's
iteration for lambda = w appears), so it is called with ``w = tau * weight``.

Arrays are ``(Z, Y, X)`` or ``(n, Z, Y, X)``, x fastest.  ``B`` (3 x 4, from :func:`_resample.index_affine`) maps an
integer index v of the high-resolution grid H to the continuous stack index ``u = coord(B, v)``; the weight of the pair
(stack sample j, voxel v) is ``(tri(u_x - j_x) * tri(u_y - j_y)) * prof(u_z - j_z)`` and BOTH directions compute it from
that u, so the matrix and its transpose hold the same bits.  Sums are float64, one rounding per operation in the order
written, candidates in ascending (z, y, x); a candidate of weight 0 is skipped, so the result does not depend on the
candidate boxes, which only have to cover the support.  Host code for tests and baselines: the product path is the HIP
kernel.

A stack acquired slice by slice from a moving subject has a rigid pose per slice: :func:`forward_slices`,
:func:`adjoint_slices` and ``reconstruct_sr(slice_transforms=...)`` take an affine per slice (``(lz, 3, 4)``, from
:func:`slice_affines`), sample ``j`` forming its weights from ``u = coord(B[j_z], v)``; the statement of
t2fit_sr_slice_forward_dev / t2fit_sr_slice_adjoint_dev.

Bad slices (drop-outs, stripes, misplaced slices) are weighted down by ``reconstruct_sr(robust=...)``: every iteration
multiplies its residuals by a weight per slice and a Huber weight per sample (:func:`robust_step`, the statement of
t2fit_sr_robust_dev: only +, x, /, sqrt and comparisons, the slice sums in the device's tree lane by lane)."""
from __future__ import annotations

import numpy as np

from . import _resample, _tv

BOX, BSPLINE3 = 0, 1
PROFILES = {"box": BOX, "bspline3": BSPLINE3}
MAX_STACKS = 6
BSPLINE3_FWHM = 1.4447034489287527  # full width at half maximum of the cubic B-spline: 2 x, x^3 / 2 - x^2 + 1 / 3 = 0
DEFAULT_WEIGHT, DEFAULT_N_ITER, DEFAULT_PROX_ITER = 16.0, 8, 5  # the sweep they come from


def _profile_id(profile):
    if profile in PROFILES:
        return PROFILES[profile]
    if profile in (BOX, BSPLINE3) and not isinstance(profile, str):
        return int(profile)
    raise ValueError(f"profile must be one of {sorted(PROFILES)}, got {profile!r}")


def profile_params(profile, rel_thickness):
    """``(par, half_width)`` in slice-index units of a profile whose thickness is ``rel_thickness`` slice spacings: box
    ``par = h = rel / 2``, support ``-h <= d < h``; bspline3 ``par = a = rel / BSPLINE3_FWHM``, ``prof(d) = beta3(|d| / a)``,
    support ``|d| < 2 a``."""
    rel = float(rel_thickness)
    if not (rel > 0.0 and np.isfinite(rel)):
        raise ValueError(f"the slice thickness must be finite and > 0, got {rel_thickness!r}")
    if _profile_id(profile) == BOX:
        return rel / 2.0, rel / 2.0
    a = rel / BSPLINE3_FWHM
    return a, 2.0 * a


def tri(d):
    return np.maximum(0.0, 1.0 - np.abs(d))


def prof(d, profile, par):
    if profile == BOX:
        return np.where((d >= -par) & (d < par), 1.0, 0.0)
    t = np.abs(d) / par
    q = 2.0 - t
    inner = (2.0 / 3.0 - t * t) + 0.5 * ((t * t) * t)
    outer = ((q * q) * q) / 6.0
    return np.where(t < 1.0, inner, np.where(t < 2.0, outer, 0.0))


def pair_weight(ux, uy, uz, jx, jy, jz, profile, par):
    """``w(j, v)`` from the stack coordinate u of v and the sample index j (float64 arrays that broadcast)."""
    return (tri(ux - jx) * tri(uy - jy)) * prof(uz - jz, profile, par)


def _coord(a, k, ix, iy, iz):
    return ((a[k, 0] * ix + a[k, 1] * iy) + a[k, 2] * iz) + a[k, 3]


def _grid(start, shape):
    """Index grids ix, iy, iz (float64, broadcastable to ``shape`` (Z, Y, X)) of the box at ``start`` (x, y, z)."""
    iz = np.arange(start[2], start[2] + shape[0], dtype=np.float64)[:, None, None]
    iy = np.arange(start[1], start[1] + shape[1], dtype=np.float64)[None, :, None]
    ix = np.arange(start[0], start[0] + shape[2], dtype=np.float64)[None, None, :]
    return ix, iy, iz


def plan_box(B, half):
    """The host half of the forward operator (t2fit_sr_plan_host, same arithmetic): the inverse ``Binv`` (3 x 4, stack
    index -> continuous H index) and integer radii (x, y, z) such that every voxel v with a non-zero weight for sample j
    lies within ``radius`` of ``floor(coord(Binv, j) + 0.5)`` on each axis.  ``half`` (x, y, z): half-widths of the support
    in stack-index units.  ``radius_a = ceil(sum_b |Binv[a, b]| half_b) + 1``: the sum bounds the support around the exact
    preimage, 1/2 goes to the rounding of the centre, the rest to the inverse's own rounding."""
    b = np.asarray(B, np.float64).reshape(3, 4)
    half = np.asarray(half, np.float64).reshape(3)
    if not (np.all(np.isfinite(b)) and np.all(np.isfinite(half)) and np.all(half > 0)):
        raise ValueError("B must be finite and the half-widths finite and > 0")
    m = b[:, :3]
    c = np.empty((3, 3), np.float64)  # cofactors
    c[0, 0] = m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]
    c[0, 1] = m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2]
    c[0, 2] = m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]
    c[1, 0] = m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2]
    c[1, 1] = m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0]
    c[1, 2] = m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1]
    c[2, 0] = m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]
    c[2, 1] = m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]
    c[2, 2] = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    det = (m[0, 0] * c[0, 0] + m[0, 1] * c[0, 1]) + m[0, 2] * c[0, 2]
    if not (np.isfinite(det) and det != 0.0):
        raise ValueError("B is singular")
    inv = np.empty((3, 4), np.float64)
    radius = []
    for a in range(3):
        for k in range(3):
            inv[a, k] = c[k, a] / det
        inv[a, 3] = -((inv[a, 0] * b[0, 3] + inv[a, 1] * b[1, 3]) + inv[a, 2] * b[2, 3])
        reach = (abs(inv[a, 0]) * half[0] + abs(inv[a, 1]) * half[1]) + abs(inv[a, 2]) * half[2]
        if not (np.isfinite(reach) and reach < 2.0 ** 20):
            raise ValueError("B is singular")
        radius.append(int(np.ceil(reach)) + 1)
    return inv, tuple(radius)


def _volumes(x):
    x = np.asarray(x)
    if x.ndim not in (3, 4):
        raise ValueError("a volume is (Z, Y, X) or (n, Z, Y, X)")
    return x.reshape((-1,) + x.shape[-3:]), x.ndim == 3


def forward(x, B, lr_shape, profile="box", rel_thickness=1.0, *, y=None, mask=None, hr_shape=None, start=(0, 0, 0),
            shape=None, out_dtype=np.float32, box=None):
    """``(out, N)`` of one stack: ``N[j] = sum_v w(j, v)`` (float64) and ``out[j] = (sum_v w x[v]) / N[j]``, minus ``y[j]``
    when ``y`` is given; 0 where the sample does not count (``N[j] <= 0`` or its ``mask`` is 0).  ``x = None`` (then give
    ``hr_shape``): the weights only, ``out`` is None.  ``start`` (x, y, z) and ``shape`` (Z, Y, X): the box of samples to
    evaluate (``y`` and ``mask`` still cover the whole stack), by default all of ``lr_shape``.  ``box``: ``(Binv, radius)``
    to walk instead of :func:`plan_box`'s."""
    pid = _profile_id(profile)
    par, hw = profile_params(pid, rel_thickness)
    b = np.asarray(B, np.float64).reshape(3, 4)
    if x is not None:
        xv, single = _volumes(x)
        hr_shape = xv.shape[-3:]
    else:
        xv, single = None, True
    hz, hy, hx = (int(v) for v in hr_shape)
    lr_shape = tuple(int(v) for v in lr_shape)
    shape = lr_shape if shape is None else tuple(int(v) for v in shape)
    binv, radius = plan_box(b, (1.0, 1.0, hw)) if box is None else box
    jx, jy, jz = _grid(start, shape)
    k = [np.broadcast_to(np.floor(_coord(binv, a, jx, jy, jz) + 0.5), shape) for a in range(3)]
    n_sum = np.zeros(shape, np.float64)
    acc = None if xv is None else np.zeros((len(xv),) + shape, np.float64)
    for dz in range(-radius[2], radius[2] + 1):
        vz = k[2] + dz
        in_z = (vz >= 0) & (vz <= hz - 1)
        if not in_z.any():
            continue
        for dy in range(-radius[1], radius[1] + 1):
            vy = k[1] + dy
            in_zy = in_z & (vy >= 0) & (vy <= hy - 1)
            if not in_zy.any():
                continue
            for dx in range(-radius[0], radius[0] + 1):
                vx = k[0] + dx
                inside = in_zy & (vx >= 0) & (vx <= hx - 1)
                if not inside.any():
                    continue
                w = pair_weight(_coord(b, 0, vx, vy, vz), _coord(b, 1, vx, vy, vz), _coord(b, 2, vx, vy, vz), jx, jy, jz, pid, par)
                use = inside & (w > 0.0)
                if not use.any():
                    continue
                n_sum = np.where(use, n_sum + w, n_sum)
                if acc is not None:
                    iz, iy, ix = (np.clip(v, 0, n - 1).astype(np.int64) for v, n in ((vz, hz), (vy, hy), (vx, hx)))
                    with np.errstate(all="ignore"):
                        acc = np.where(use, acc + w * xv[:, iz, iy, ix].astype(np.float64), acc)
    if acc is None:
        return None, n_sum
    sub = tuple(slice(s, s + n) for s, n in zip(start[::-1], shape))
    counts = n_sum > 0.0
    if mask is not None:
        counts &= np.asarray(mask).reshape(lr_shape)[sub] != 0
    with np.errstate(all="ignore"):
        out = acc / np.where(counts, n_sum, 1.0)
        if y is not None:
            out = out - np.asarray(y).reshape((-1,) + lr_shape)[(slice(None),) + sub].astype(np.float64)
        out = np.where(counts, out, 0.0).astype(out_dtype)
    return (out[0] if single else out), n_sum


def adjoint(r, N, B, profile, rel_thickness, hr_shape, *, masks=None, x=None, tau=0.0, start=(0, 0, 0), shape=None,
            out_dtype=np.float32):
    """``sum_s A_s^T r_s`` on the grid ``hr_shape``: lists over the stacks of residuals ``r[s]`` (``(lz, ly, lx)`` or
    ``(n, lz, ly, lx)``), normalisers ``N[s]`` (float64, from :func:`forward`), affines, profiles and thicknesses (a scalar
    profile / thickness serves all).  One float64 accumulator per voxel runs over the stacks in order and, within a stack,
    over its candidate samples in ascending (z, y, x): ``acc += (w * r[j]) / N[j]`` for the samples that count.  With ``x``:
    ``x - tau * acc``.  ``start`` / ``shape``: the box of voxels to evaluate."""
    n_s = len(r)
    if not 1 <= n_s <= MAX_STACKS:
        raise ValueError(f"between 1 and {MAX_STACKS} stacks, got {n_s}")
    profiles = [profile] * n_s if isinstance(profile, (str, int)) else list(profile)
    rels = [rel_thickness] * n_s if np.ndim(rel_thickness) == 0 else list(rel_thickness)
    masks = [None] * n_s if masks is None else list(masks)
    hr_shape = tuple(int(v) for v in hr_shape)
    shape = hr_shape if shape is None else tuple(int(v) for v in shape)
    rv = [_volumes(v) for v in r]
    single = rv[0][1]
    n_vol = len(rv[0][0])
    vx, vy, vz = _grid(start, shape)
    acc = np.zeros((n_vol,) + shape, np.float64)
    for s in range(n_s):
        rs = rv[s][0]
        lz, ly, lx = rs.shape[-3:]
        pid = _profile_id(profiles[s])
        par, hw = profile_params(pid, rels[s])
        b = np.asarray(B[s], np.float64).reshape(3, 4)
        ns = np.asarray(N[s], np.float64).reshape(lz, ly, lx)
        ms = None if masks[s] is None else np.asarray(masks[s]).reshape(lz, ly, lx) != 0
        u = [np.broadcast_to(_coord(b, a, vx, vy, vz), shape) for a in range(3)]
        f = [np.floor(u[0]), np.floor(u[1]), np.floor(u[2] - hw)]
        for cz in range(int(np.floor(2.0 * hw)) + 3):
            jz = f[2] + cz
            in_z = (jz >= 0) & (jz <= lz - 1)
            if not in_z.any():
                continue
            for cy in (0, 1):
                jy = f[1] + cy
                in_zy = in_z & (jy >= 0) & (jy <= ly - 1)
                for cx in (0, 1):
                    jx = f[0] + cx
                    inside = in_zy & (jx >= 0) & (jx <= lx - 1)
                    if not inside.any():
                        continue
                    w = pair_weight(u[0], u[1], u[2], jx, jy, jz, pid, par)
                    iz, iy, ix = (np.clip(v, 0, n - 1).astype(np.int64) for v, n in ((jz, lz), (jy, ly), (jx, lx)))
                    nj = ns[iz, iy, ix]
                    use = inside & (w > 0.0) & (nj > 0.0)
                    if ms is not None:
                        use &= ms[iz, iy, ix]
                    if not use.any():
                        continue
                    with np.errstate(all="ignore"):
                        acc = np.where(use, acc + (w * rs[:, iz, iy, ix].astype(np.float64)) / np.where(use, nj, 1.0), acc)
    if x is not None:
        sub = tuple(slice(s, s + n) for s, n in zip(start[::-1], shape))
        xs = np.asarray(x).reshape((-1,) + hr_shape)[(slice(None),) + sub].astype(np.float64)
        with np.errstate(all="ignore"):
            acc = xs - float(tau) * acc
    out = acc.astype(out_dtype)
    return out[0] if single else out


# ---- a rigid pose per slice ----------------------------------------------------------------------------------------------
def slice_affines(hi, geom, slice_transforms):
    """``(lz, 3, 4)``: ``B[k] = index_affine(hi, geom, slice_transforms[k])``, the index affine of slice k of the stack
    ``geom`` whose pose is ``slice_transforms[k]`` (4 x 4, fixed point -> stack point)."""
    g = _resample.as_geometry(geom)
    t = np.asarray(slice_transforms, np.float64)
    lz = int(g.GetSize()[2])
    if t.shape != (lz, 4, 4):
        raise ValueError(f"slice transforms must be (lz, 4, 4) = ({lz}, 4, 4), got shape {t.shape}")
    if not np.all(np.isfinite(t)):
        raise ValueError("slice transforms must be finite")
    return np.stack([_resample.index_affine(hi, g, t[k]) for k in range(lz)])


def compose_slice_transforms(stack_transform, motion, geom):
    """``(lz, 4, 4)`` fixed point -> stack point: the stack's transform (4 x 4 or None) followed, for slice k, by the rigid
    motion ``motion[k] = (rx, ry, rz [rad], tx, ty, tz [mm])`` in the convention of :func:`_register.compose`, applied about
    the physical centre of slice k of ``geom``."""
    from . import _register

    g = _resample.as_geometry(geom)
    nx, ny, lz = (int(v) for v in g.GetSize())
    motion = np.asarray(motion, np.float64)
    if motion.shape != (lz, 6) or not np.all(np.isfinite(motion)):
        raise ValueError(f"motion must be finite (lz, 6) = ({lz}, 6), got shape {motion.shape}")
    base = np.eye(4) if stack_transform is None else np.asarray(stack_transform, np.float64)
    if base.shape != (4, 4) or not np.all(np.isfinite(base)):
        raise ValueError("the stack transform must be a finite 4 x 4 matrix")
    m, o = _resample._index_to_point(g)
    out = np.empty((lz, 4, 4), np.float64)
    for k in range(lz):
        centre = o + m @ np.array([(nx - 1) / 2.0, (ny - 1) / 2.0, float(k)])
        out[k] = _register.compose(motion[k], centre) @ base
    return out


def _slice_affine_list(B, lz):
    b = np.asarray(B, np.float64)
    if b.shape != (lz, 3, 4):
        raise ValueError(f"one 3 x 4 affine per slice: expected shape ({lz}, 3, 4), got {b.shape}")
    return b


def forward_slices(x, B, lr_shape, profile="box", rel_thickness=1.0, *, y=None, mask=None, hr_shape=None, start=(0, 0, 0),
                   shape=None, out_dtype=np.float32):
    """:func:`forward` with an affine per slice, ``B`` ``(lz, 3, 4)``: sample ``j`` takes its weights from ``B[j_z]`` and
    walks the box of :func:`plan_box` of that affine (here every slice walks the largest of the radii: the box only has to
    cover the support).  The terms of a sample and their order are those of :func:`forward` with its slice's affine, so
    equal affines give its bits."""
    pid = _profile_id(profile)
    par, hw = profile_params(pid, rel_thickness)
    lr_shape = tuple(int(v) for v in lr_shape)
    bs = _slice_affine_list(B, lr_shape[0])
    if x is not None:
        xv, single = _volumes(x)
        hr_shape = xv.shape[-3:]
    else:
        xv, single = None, True
    hz, hy, hx = (int(v) for v in hr_shape)
    shape = lr_shape if shape is None else tuple(int(v) for v in shape)
    ks = range(int(start[2]), int(start[2]) + shape[0])
    plans = [plan_box(bs[k], (1.0, 1.0, hw)) for k in ks]
    radius = [max(p[1][a] for p in plans) for a in range(3)]
    b = np.stack([bs[k] for k in ks])[:, :, :, None, None]  # [slice of the box][row][column], broadcast over (y, x)
    binv = np.stack([p[0] for p in plans])[:, :, :, None, None]
    co = lambda m, a, ix, iy, iz: ((m[:, a, 0] * ix + m[:, a, 1] * iy) + m[:, a, 2] * iz) + m[:, a, 3]
    jx, jy, jz = _grid(start, shape)
    k = [np.broadcast_to(np.floor(co(binv, a, jx, jy, jz) + 0.5), shape) for a in range(3)]
    n_sum = np.zeros(shape, np.float64)
    acc = None if xv is None else np.zeros((len(xv),) + shape, np.float64)
    for dz in range(-radius[2], radius[2] + 1):
        vz = k[2] + dz
        in_z = (vz >= 0) & (vz <= hz - 1)
        if not in_z.any():
            continue
        for dy in range(-radius[1], radius[1] + 1):
            vy = k[1] + dy
            in_zy = in_z & (vy >= 0) & (vy <= hy - 1)
            if not in_zy.any():
                continue
            for dx in range(-radius[0], radius[0] + 1):
                vx = k[0] + dx
                inside = in_zy & (vx >= 0) & (vx <= hx - 1)
                if not inside.any():
                    continue
                w = pair_weight(co(b, 0, vx, vy, vz), co(b, 1, vx, vy, vz), co(b, 2, vx, vy, vz), jx, jy, jz, pid, par)
                use = inside & (w > 0.0)
                if not use.any():
                    continue
                n_sum = np.where(use, n_sum + w, n_sum)
                if acc is not None:
                    iz, iy, ix = (np.clip(v, 0, n - 1).astype(np.int64) for v, n in ((vz, hz), (vy, hy), (vx, hx)))
                    with np.errstate(all="ignore"):
                        acc = np.where(use, acc + w * xv[:, iz, iy, ix].astype(np.float64), acc)
    if acc is None:
        return None, n_sum
    sub = tuple(slice(s, s + n) for s, n in zip(start[::-1], shape))
    counts = n_sum > 0.0
    if mask is not None:
        counts &= np.asarray(mask).reshape(lr_shape)[sub] != 0
    with np.errstate(all="ignore"):
        out = acc / np.where(counts, n_sum, 1.0)
        if y is not None:
            out = out - np.asarray(y).reshape((-1,) + lr_shape)[(slice(None),) + sub].astype(np.float64)
        out = np.where(counts, out, 0.0).astype(out_dtype)
    return (out[0] if single else out), n_sum


def adjoint_slices(r, N, B, profile, rel_thickness, hr_shape, *, masks=None, x=None, tau=0.0, start=(0, 0, 0), shape=None,
                   out_dtype=np.float32):
    """:func:`adjoint` with an affine per slice, ``B[s]`` ``(lz_s, 3, 4)``.  One float64 accumulator per voxel runs over the
    stacks in order, within a stack over ALL slices in ascending index k (not position in space), within a slice over the
    2 x 2 in-plane candidates ``(floor(u_y) + cy, floor(u_x) + cx)`` in ascending (cy, cx) with ``u = coord(B[s][k], v)``:
    ``acc += (w * r[j]) / N[j]`` for the samples that count and have ``w > 0``.  Equal affines give :func:`adjoint`'s bits:
    the non-zero terms and their order are the same."""
    n_s = len(r)
    if not 1 <= n_s <= MAX_STACKS:
        raise ValueError(f"between 1 and {MAX_STACKS} stacks, got {n_s}")
    profiles = [profile] * n_s if isinstance(profile, (str, int)) else list(profile)
    rels = [rel_thickness] * n_s if np.ndim(rel_thickness) == 0 else list(rel_thickness)
    masks = [None] * n_s if masks is None else list(masks)
    hr_shape = tuple(int(v) for v in hr_shape)
    shape = hr_shape if shape is None else tuple(int(v) for v in shape)
    rv = [_volumes(v) for v in r]
    single = rv[0][1]
    n_vol = len(rv[0][0])
    vx, vy, vz = _grid(start, shape)
    acc = np.zeros((n_vol,) + shape, np.float64)
    for s in range(n_s):
        rs = rv[s][0]
        lz, ly, lx = rs.shape[-3:]
        pid = _profile_id(profiles[s])
        par, _ = profile_params(pid, rels[s])
        bs = _slice_affine_list(B[s], lz)
        ns = np.asarray(N[s], np.float64).reshape(lz, ly, lx)
        ms = None if masks[s] is None else np.asarray(masks[s]).reshape(lz, ly, lx) != 0
        for k in range(lz):
            with np.errstate(all="ignore"):
                reached = prof(np.broadcast_to(_coord(bs[k], 2, vx, vy, vz), shape) - float(k), pid, par) > 0.0
            if not reached.any():
                continue  # every pair of this slice has weight 0
            # the box of voxels the profile reaches: outside it every weight is 0 and the accumulator stays as it is
            box = tuple(slice(int(np.argmax(m)), len(m) - int(np.argmax(m[::-1]))) for m in
                        (reached.any(axis=(1, 2)), reached.any(axis=(0, 2)), reached.any(axis=(0, 1))))
            gx, gy, gz = vx[:, :, box[2]], vy[:, box[1], :], vz[box[0], :, :]
            sub_shape = tuple(b.stop - b.start for b in box)
            part = acc[(slice(None),) + box]
            with np.errstate(all="ignore"):
                u = [np.broadcast_to(_coord(bs[k], a, gx, gy, gz), sub_shape) for a in range(3)]
                f = [np.floor(u[0]), np.floor(u[1])]
            for cy in (0, 1):
                jy = f[1] + cy
                in_y = (jy >= 0) & (jy <= ly - 1)
                for cx in (0, 1):
                    jx = f[0] + cx
                    inside = in_y & (jx >= 0) & (jx <= lx - 1)
                    if not inside.any():
                        continue
                    with np.errstate(all="ignore"):
                        w = pair_weight(u[0], u[1], u[2], jx, jy, float(k), pid, par)
                        iy, ix = (np.clip(np.where(inside, v, 0), 0, n - 1).astype(np.int64) for v, n in ((jy, ly), (jx, lx)))
                    nj = ns[k, iy, ix]
                    use = inside & (w > 0.0) & (nj > 0.0)
                    if ms is not None:
                        use &= ms[k, iy, ix]
                    if not use.any():
                        continue
                    with np.errstate(all="ignore"):
                        part = np.where(use, part + (w * rs[:, k, iy, ix].astype(np.float64)) / np.where(use, nj, 1.0), part)
            acc[(slice(None),) + box] = part
    if x is not None:
        sub = tuple(slice(s, s + n) for s, n in zip(start[::-1], shape))
        xs = np.asarray(x).reshape((-1,) + hr_shape)[(slice(None),) + sub].astype(np.float64)
        with np.errstate(all="ignore"):
            acc = xs - float(tau) * acc
    out = acc.astype(out_dtype)
    return out[0] if single else out


def check_slice_transforms(slice_transforms, order, lr_shapes):
    """``{stack name: (lz, 4, 4) float64}`` after the refusals: unknown names, wrong shapes, non-finite entries."""
    unknown = [k for k in slice_transforms if k not in order]
    if unknown:
        raise ValueError(f"slice transforms are given per stack {list(order)}, got {unknown}")
    out = {}
    for o, t in slice_transforms.items():
        t = np.asarray(t, np.float64)
        lz = int(lr_shapes[list(order).index(o)][0])
        if t.shape != (lz, 4, 4):
            raise ValueError(f"slice transforms of stack {o!r} must be (lz, 4, 4) = ({lz}, 4, 4), got shape {t.shape}")
        if not np.all(np.isfinite(t)):
            raise ValueError(f"slice transforms of stack {o!r} have a non-finite entry")
        out[o] = t
    return out


def slice_plan(order, hi, geoms, B, lr_shapes, slice_transforms):
    """The affines of every slice of every stack, a list over ``order`` of ``(lz, 3, 4)``: from the stack's entry of
    ``slice_transforms`` where it has one, else the stack's own affine ``B[s]`` on every slice."""
    st = check_slice_transforms(slice_transforms, order, lr_shapes)
    return [slice_affines(hi, _resample.as_geometry(geoms[o]), st[o]) if o in st
            else np.repeat(np.asarray(B[s], np.float64).reshape(1, 3, 4), int(lr_shapes[s][0]), axis=0)
            for s, o in enumerate(order)]


def counted(N, mask=None):
    """1.0 where a sample counts, else 0.0 (float32): the residual whose adjoint is ``A^T 1``."""
    c = np.asarray(N) > 0.0
    if mask is not None:
        c &= np.asarray(mask).reshape(c.shape) != 0
    return c.astype(np.float32)


def step_size(column_max):
    """``tau = 1 / sum_s max_v (A_s^T 1)[v]``: the rows of A_s sum to 1, so ``||A_s||^2 <= ||A_s||_1 ||A_s||_inf`` is at
    most the largest column sum.  The sum runs over the stacks in order, in float64."""
    total = 0.0
    for m in column_max:
        total = total + float(m)
    if not (total > 0.0 and np.isfinite(total)):
        raise ValueError("no stack sample counts on this grid: nothing to reconstruct from")
    return 1.0 / total


def sr_plan(geoms, fixed="ax", res=1.0, transforms=None, thickness=None):
    """``(order, H, B list, rel_thickness list)``: the fixed stack first, then the others as ``geoms`` lists them; ``H`` the
    fixed stack's isotropic grid; ``B[s] = index_affine(H, G_s, T_s)``; the thickness of each stack in units of its slice
    spacing (``thickness``: mm, a number for all stacks or {name: mm}; default the slice spacing itself)."""
    if fixed not in geoms:
        raise ValueError(f"the fixed stack {fixed!r} is not among {list(geoms)}")
    order = [fixed] + [o for o in geoms if o != fixed]
    if not 1 <= len(order) <= MAX_STACKS:
        raise ValueError(f"between 1 and {MAX_STACKS} stacks, got {len(order)}")
    transforms = transforms or {}
    unknown = [k for k in transforms if k not in order[1:]]
    if unknown:
        raise ValueError(f"transforms are given per moving stack {order[1:]}, got {unknown}")
    lo = [_resample.as_geometry(geoms[o]) for o in order]
    hi = _resample.isotropic_geometry(lo[0], res)
    b = [_resample.index_affine(hi, g, transforms.get(o)) for o, g in zip(order, lo)]
    rel = []
    for o, g in zip(order, lo):
        t = thickness.get(o) if isinstance(thickness, dict) else thickness
        t = g.GetSpacing()[2] if t is None else float(t)
        if not (t > 0.0 and np.isfinite(t)):
            raise ValueError(f"the slice thickness must be finite and > 0, got {t!r} for {o!r}")
        rel.append(t / g.GetSpacing()[2])
    return order, hi, b, rel


def initial_volume(stacks, geoms, order, hi, res, transforms):
    """``x_0``: the averaged merge when the stacks are exactly ax, cor and sag, else the fixed stack's own linear resample."""
    if sorted(order) == sorted(_resample.ORIENTATIONS):
        return _resample.reconstruct(stacks, geoms, order[0], res, transforms)[0]
    g = _resample.as_geometry(geoms[order[0]], np.asarray(stacks[order[0]]).shape[-3:])
    return _resample.resample(np.asarray(stacks[order[0]], np.float32), _resample.index_affine(hi, g), hi.shape)


# ---- outlier weighting: a weight per slice and a Huber weight per sample ------------------------------------------------
ROBUST_DEFAULTS = {"slice_threshold": 1.5, "huber": 2.5, "min_count": 16, "sigma_floor": 0.0}  # the sweep
ROBUST_MAX_SLICES = 4096
ROBUST_LANES, ROBUST_WAVE = 256, 64


def robust_params(robust):
    """None for ``None`` / ``False``, the defaults for ``True``, a checked copy of the defaults updated by a dict."""
    if robust is None or robust is False:
        return None
    p = dict(ROBUST_DEFAULTS)
    if robust is not True:
        if not isinstance(robust, dict):
            raise ValueError(f"robust is None, True or a dict of {sorted(ROBUST_DEFAULTS)}, got {robust!r}")
        unknown = [k for k in robust if k not in p]
        if unknown:
            raise ValueError(f"robust takes {sorted(ROBUST_DEFAULTS)}, got {unknown}")
        p.update(robust)
    for k in ("slice_threshold", "huber"):
        p[k] = float(p[k])
        if not (p[k] > 0.0 and np.isfinite(p[k])):
            raise ValueError(f"robust {k} must be finite and > 0, got {p[k]!r}")
    p["sigma_floor"] = float(p["sigma_floor"])
    if not (p["sigma_floor"] >= 0.0 and np.isfinite(p["sigma_floor"])):
        raise ValueError(f"robust sigma_floor must be finite and >= 0, got {p['sigma_floor']!r}")
    if int(p["min_count"]) != p["min_count"] or int(p["min_count"]) < 1:
        raise ValueError(f"robust min_count must be an integer >= 1, got {p['min_count']!r}")
    p["min_count"] = int(p["min_count"])
    return p


def _robust_counted(rv, N, mask):
    """Which samples of ``rv`` ``(n, lz, ly, lx)`` are counted: ``N > 0``, the mask byte set, the residual finite."""
    c = np.asarray(N, np.float64).reshape(rv.shape[-3:]) > 0.0
    if mask is not None:
        c &= np.asarray(mask).reshape(c.shape) != 0
    return c[None] & np.isfinite(rv)


def robust_slice_sums(r, N, mask=None):
    """``(n, lz, 2)`` float64: per echo and slice the number ``c`` of counted samples and ``q2 = sum (double)r (double)r``
    over them, in the device's tree, lane by lane: lane ``t`` of 256 adds the samples ``i = t, t + 256, ...`` of the
    slice's ``ly lx`` in ascending ``i``; each wave of 64 lanes adds by the xor butterfly 32, 16, .., 1; the four waves meet
    as ``((w0 + w1) + w2) + w3``."""
    rv = _volumes(r)[0]
    n_vol, lz, ly, lx = rv.shape
    plane = ly * lx
    rows = -(-plane // ROBUST_LANES)
    pad = ((0, 0), (0, 0), (0, rows * ROBUST_LANES - plane))
    ok = np.pad(_robust_counted(rv, N, mask).reshape(n_vol, lz, plane), pad).reshape(n_vol, lz, rows, ROBUST_LANES)
    d = np.pad(rv.astype(np.float64).reshape(n_vol, lz, plane), pad).reshape(n_vol, lz, rows, ROBUST_LANES)
    c = np.zeros((n_vol, lz, ROBUST_LANES), np.float64)
    q2 = np.zeros((n_vol, lz, ROBUST_LANES), np.float64)
    with np.errstate(all="ignore"):
        for i in range(rows):
            q2 = np.where(ok[:, :, i], q2 + d[:, :, i] * d[:, :, i], q2)
            c = np.where(ok[:, :, i], c + 1.0, c)
    lane = np.arange(ROBUST_LANES)
    out = []
    for v in (c, q2):
        for s in (32, 16, 8, 4, 2, 1):
            v = v + v[..., lane ^ s]
        w = v[..., ::ROBUST_WAVE]
        out.append(((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3])
    return np.stack(out, axis=-1)


def robust_scale(sums, params=None):
    """``(weights (n, n_slices), sigma2 (n,))`` from the sums of every slice of every stack, ``(n, n_slices, 2)``, listed
    stack-major and ascending in slice index.  Per echo: slice k is eligible when ``c >= min_count``, then ``m_k = q2 / c``;
    with ``v`` the sorted eligible ``m``, ``sigma2 = max(0.5 (v[(n - 1) // 2] + v[n // 2]), sigma_floor^2)``; no eligible
    slice or ``sigma2`` not > 0: robustness is off (weights 1, ``sigma2`` reported 0).  ``q_k = 1`` if the slice is not
    eligible or ``m_k <= t^2 sigma2``, else ``(t^2 sigma2) / m_k``."""
    p = robust_params(True if params is None else params)
    sums = np.asarray(sums, np.float64)
    n_vol, n_slices = sums.shape[:2]
    if n_slices > ROBUST_MAX_SLICES:
        raise ValueError(f"at most {ROBUST_MAX_SLICES} slices in total, got {n_slices}")
    tt, floor2 = p["slice_threshold"] * p["slice_threshold"], p["sigma_floor"] * p["sigma_floor"]
    weights, sigma2 = np.ones((n_vol, n_slices), np.float64), np.zeros(n_vol, np.float64)
    for e in range(n_vol):
        c, q2 = sums[e, :, 0], sums[e, :, 1]
        eligible = c >= float(p["min_count"])
        m = np.where(eligible, q2 / np.where(eligible, c, 1.0), -1.0)
        v = np.sort(m[eligible])
        n = len(v)
        if n == 0:
            continue
        s2 = 0.5 * (v[(n - 1) // 2] + v[n // 2])
        s2 = s2 if s2 > floor2 else floor2
        if not s2 > 0.0:
            continue
        sigma2[e] = s2
        limit = tt * s2
        down = eligible & ~(m <= limit)
        weights[e] = np.where(down, limit / np.where(down, m, 1.0), 1.0)
    return weights, sigma2


def robust_apply(r, N, mask, weights, sigma2, params=None):
    """The weighted residual of one stack: ``weights`` ``(n, lz)`` are its slices' ``q``, ``sigma2`` ``(n,)``.  A counted
    sample becomes ``(float)((q_k w_j) (double)r_j)`` with ``w_j = 1`` if ``|r_j| <= delta`` else ``delta / |r_j|``,
    ``delta = huber sqrt(sigma2)``; a sample that is not counted becomes +0.0; an echo with ``sigma2 = 0`` stays as it is."""
    p = robust_params(True if params is None else params)
    rv = _volumes(r)[0]
    ok = _robust_counted(rv, N, mask)
    s2 = np.asarray(sigma2, np.float64).reshape(-1, 1, 1, 1)
    q = np.asarray(weights, np.float64).reshape(rv.shape[0], rv.shape[1], 1, 1)
    with np.errstate(all="ignore"):
        delta = p["huber"] * np.sqrt(s2)
        d = rv.astype(np.float64)
        ad = np.abs(d)
        inside = ad <= delta
        w = np.where(inside, 1.0, delta / np.where(inside, 1.0, ad))
        out = np.where(ok, (q * w) * d, 0.0).astype(rv.dtype)
    out = np.where(s2 > 0.0, out, rv)
    return out.reshape(np.shape(r))


def robust_step(r, N, masks=None, params=None):
    """``(weighted r, slice weights, sigma2, sums)`` of all stacks: lists over the stacks of residuals and normalisers.
    ``slice weights``: one ``(n, lz_s)`` array per stack; ``sums``: ``(n, n_slices, 2)`` over all slices, stack-major."""
    p = robust_params(True if params is None else params)
    n_s = len(r)
    if not 1 <= n_s <= MAX_STACKS or len(N) != n_s:
        raise ValueError(f"between 1 and {MAX_STACKS} stacks with one N each, got {n_s}")
    masks = [None] * n_s if masks is None else list(masks)
    sums = np.concatenate([robust_slice_sums(r[s], N[s], masks[s]) for s in range(n_s)], axis=1)
    weights, sigma2 = robust_scale(sums, p)
    edges = np.cumsum([0] + [_volumes(v)[0].shape[1] for v in r])
    per_stack = [weights[:, edges[s]:edges[s + 1]].copy() for s in range(n_s)]
    out = [robust_apply(r[s], N[s], masks[s], per_stack[s], sigma2, p) for s in range(n_s)]
    return out, per_stack, sigma2, sums


def _reweigh(r, N, masks, robust, info):
    """The residuals after :func:`robust_step` when ``robust`` asks for it; ``info`` (a dict or None) takes the tables."""
    p = robust_params(robust)
    if p is None:
        return r
    r, weights, sigma2, sums = robust_step(r, N, masks, p)
    if info is not None:
        info.update(slice_weights=weights, sigma2=sigma2, robust_sums=sums)
    return r


def _prox_joint(z, w, prox_iter, out_dtype):
    """The prox of ``w`` times the vector-valued TV across the echoes of ``z`` ``(n, Z, Y, X)``: the joint denoiser in 3-D,
    one problem, ``eps = 0``, ``prox_iter`` iterations (with one echo, the per-echo prox)."""
    if np.dtype(out_dtype) == np.float32:
        return _tv.denoise_tv_joint(z, w, eps=0.0, max_iter=prox_iter, dims=3, precision="f32")[0]
    return _tv.tv_joint_problem(z, w, 0.0, prox_iter, np.float64)[0]


def iterate(x, y, N, B, profile, rels, tau, weight, prox_iter, masks=None, out_dtype=np.float32, robust=None, info=None,
            tv="channel"):
    """One proximal-gradient step on ``x`` ``(n, Z, Y, X)``: residuals of every stack, the update ``z``, the TV prox
    (``tv``: ``"channel"``, every echo on its own, or ``"joint"``, one gradient norm per voxel across the echoes).
    ``robust`` (None, True or a dict of :data:`ROBUST_DEFAULTS`): the residuals pass through :func:`robust_step` first;
    ``info``: a dict that then receives ``slice_weights``, ``sigma2`` and ``robust_sums``."""
    r = [forward(x, B[s], y[s].shape[-3:], profile, rels[s], y=y[s], mask=None if masks is None else masks[s],
                 out_dtype=out_dtype)[0] for s in range(len(y))]
    r = _reweigh(r, N, masks, robust, info)
    z = adjoint(r, N, B, profile, rels, x.shape[-3:], masks=masks, x=x, tau=tau, out_dtype=out_dtype)
    if not weight > 0.0:
        return z
    if tv == "joint":
        return _prox_joint(z, tau * weight, prox_iter, out_dtype)
    if np.dtype(out_dtype) == np.float32:
        return _tv.denoise_tv(z, tau * weight, eps=0.0, max_iter=prox_iter, dims=3, precision="f32")[0]
    return np.stack([_tv.tv_problem(v, tau * weight, 0.0, prox_iter, np.float64)[0] for v in z])


def iterate_slices(x, y, N, B, profile, rels, tau, weight, prox_iter, masks=None, out_dtype=np.float32, robust=None,
                   info=None, tv="channel"):
    """:func:`iterate` on the slice operators: ``B[s]`` is ``(lz_s, 3, 4)``."""
    r = [forward_slices(x, B[s], y[s].shape[-3:], profile, rels[s], y=y[s], mask=None if masks is None else masks[s],
                        out_dtype=out_dtype)[0] for s in range(len(y))]
    r = _reweigh(r, N, masks, robust, info)
    z = adjoint_slices(r, N, B, profile, rels, x.shape[-3:], masks=masks, x=x, tau=tau, out_dtype=out_dtype)
    if not weight > 0.0:
        return z
    if tv == "joint":
        return _prox_joint(z, tau * weight, prox_iter, out_dtype)
    if np.dtype(out_dtype) == np.float32:
        return _tv.denoise_tv(z, tau * weight, eps=0.0, max_iter=prox_iter, dims=3, precision="f32")[0]
    return np.stack([_tv.tv_problem(v, tau * weight, 0.0, prox_iter, np.float64)[0] for v in z])


def reconstruct_sr(stacks, geoms, *, fixed="ax", res=1.0, transforms=None, thickness=None, profile="box",
                   weight=DEFAULT_WEIGHT, n_iter=DEFAULT_N_ITER, prox_iter=DEFAULT_PROX_ITER, stack_masks=None, x0=None,
                   return_info=False, out_dtype=np.float32, slice_transforms=None, robust=None, tv="channel"):
    """The whole reconstruction on the host, argument for argument ``t2map.reconstruct_sr``.  ``tv``: ``"channel"`` (the
    prox of every echo on its own) or ``"joint"`` (vector-valued TV across the echoes: :func:`_tv.denoise_tv_joint` with
    ``w = tau * weight``, ``eps = 0``, ``prox_iter`` iterations; with one echo it equals ``"channel"``).  Returns ``(x, Geometry of H)``
    and with ``return_info`` also ``{"tau", "N", "column_max"}``.  ``slice_transforms``: ``{stack name: (lz, 4, 4)}``, a pose
    per slice (fixed point -> stack point) in place of the stack's transform; the fixed stack may have an entry, stacks
    without one carry their stack transform on every slice.  Then N, tau and the loop run on :func:`forward_slices` and
    :func:`adjoint_slices`; ``x0`` stays the merge.  None: the stack-wise operators.  ``robust`` (None, True for
    :data:`ROBUST_DEFAULTS`, or a dict of them): every iteration reweighs its residuals by :func:`robust_step`; the info then
    also holds ``"slice_weights"`` (one ``(n_vol, lz)`` array per stack) and ``"sigma2"`` (``(n_vol,)``) of the last
    iteration (None when there was none)."""
    if not (float(weight) >= 0.0 and np.isfinite(weight)) or int(n_iter) < 0 or int(prox_iter) < 1:
        raise ValueError("weight must be finite and >= 0, n_iter >= 0, prox_iter >= 1")
    if tv not in ("channel", "joint"):
        raise ValueError(f"tv must be 'channel' or 'joint', got {tv!r}")
    how = {"tv": "joint"} if tv == "joint" else {}
    robust = robust_params(robust)
    pid = _profile_id(profile)
    names = [o for o in geoms if o in stacks]
    shapes = {o: np.asarray(stacks[o]).shape for o in names}
    geoms = {o: _resample.as_geometry(geoms[o], shapes[o][-3:]) for o in names}
    order, hi, B, rels = sr_plan(geoms, fixed, res, transforms, thickness)
    y = [_volumes(np.asarray(stacks[o], np.float32))[0] for o in order]
    if len({len(v) for v in y}) != 1:
        raise ValueError(f"the stacks differ in their number of echoes: {shapes}")
    masks = None if stack_masks is None else [stack_masks.get(o) for o in order]
    fwd, adj, step = forward, adjoint, iterate
    if slice_transforms is not None:
        B = slice_plan(order, hi, geoms, B, [v.shape[-3:] for v in y], slice_transforms)
        fwd, adj, step = forward_slices, adjoint_slices, iterate_slices
    N = [fwd(None, B[s], y[s].shape[-3:], pid, rels[s], hr_shape=hi.shape)[1] for s in range(len(y))]
    col = [adj([counted(N[s], None if masks is None else masks[s])], [N[s]], [B[s]], pid, [rels[s]], hi.shape,
               masks=None if masks is None else [masks[s]], out_dtype=out_dtype) for s in range(len(y))]
    col_max = [v.max() for v in col]
    tau = step_size(col_max)
    x = initial_volume(stacks, geoms, order, hi, res, transforms) if x0 is None else np.asarray(x0)
    x = x.reshape((-1,) + hi.shape).astype(out_dtype)
    if len(x) != len(y[0]):
        raise ValueError("x0 does not have the stacks' number of echoes")
    last = {"slice_weights": None, "sigma2": None}
    for _ in range(int(n_iter)):
        if robust is None:
            x = step(x, y, N, B, pid, rels, tau, float(weight), int(prox_iter), masks, out_dtype, **how)
        else:
            x = step(x, y, N, B, pid, rels, tau, float(weight), int(prox_iter), masks, out_dtype, robust=robust, info=last,
                     **how)
    if np.asarray(stacks[order[0]]).ndim == 3:
        x = x[0]
    if return_info:
        info = {"tau": tau, "N": N, "column_max": col_max}
        if robust is not None:
            info.update(last)
        return x, hi, info
    return x, hi
