"""Marchenko-Pastur PCA denoising and noise maps across the echoes (Veraart et al., NeuroImage 2016; MRtrix's
``dwidenoise``), stated in numpy.  This is the definition of include/t2fit.h's ``t2fit_mppca_dev``: the device equals it bit
for bit.  Only + - * / sqrt abs and comparisons occur, all in float64, one rounding per operation, nothing fused, every sum
in the order written here.

Over a window of ``N = (2r+1)^dims`` voxels the ``M`` echoes form an ``M x N`` matrix of low rank plus noise.  Per centre
(a voxel whose whole window lies inside the volume): the Gram matrix ``G = X X^T`` (:func:`gram`), its eigen-decomposition
by cyclic Jacobi (:func:`jacobi`), the ascending order (:func:`order`), the noise level and the number of noise components
by the Marchenko-Pastur law (:func:`rank_sigma`), the projector onto the kept components (:func:`projector`).  Per voxel:
the mean of the projectors of all processed centres whose window holds it, applied to the voxel's own decay
(:func:`aggregate`), and the sigma / rank of the nearest centre (:func:`clamp_map`).

The noise is treated as Gaussian: at low SNR the Rician floor of magnitude data biases sigma low."""
import numpy as np

MAX_TE = 16  # T2FIT_MPPCA_MAX_TE
MAX_RADIUS = 4
MAX_SWEEPS = 16


def check(shape, radius, dims, estimator):
    """The refusals of ``t2fit_mppca_dev`` on the sizes; returns ``(M, nz, ny, nx, N)``."""
    if len(shape) != 4:
        raise ValueError(f"mppca needs a te-major (M, Z, Y, X) stack, got shape {tuple(shape)}")
    m, nz, ny, nx = (int(v) for v in shape)
    if dims not in (2, 3):
        raise ValueError(f"dims must be 2 or 3, got {dims!r}")
    if not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"radius must be 1..{MAX_RADIUS}, got {radius!r}")
    if estimator not in (1, 2):
        raise ValueError(f"estimator must be 1 or 2, got {estimator!r}")
    if not 2 <= m <= MAX_TE:
        raise ValueError(f"mppca needs 2..{MAX_TE} echoes (T2FIT_MPPCA_MAX_TE), got {m}")
    w = 2 * radius + 1
    n = w ** dims
    if n <= m:
        raise ValueError(f"the window of {n} voxels must hold more voxels than there are echoes ({m}): raise the radius")
    if nz < 1 or min(ny, nx) < w or (dims == 3 and nz < w):
        raise ValueError(f"every windowed axis must be at least {w} long, got (Z, Y, X) = {(nz, ny, nx)} with dims = {dims}")
    return m, nz, ny, nx, n


def _box(a, r, axis):
    """Sum of the ``2r+1`` neighbours along ``axis`` in increasing offset from 0.0, at the positions that have them all."""
    n = a.shape[axis] - 2 * r
    acc = np.zeros(a.shape[:axis] + (n,) + a.shape[axis + 1:])
    for k in range(2 * r + 1):
        acc = acc + np.take(a, range(k, k + n), axis=axis)
    return acc


def window_sum(a, r, dims):
    """The separable ordered window sum over the last ``dims`` axes of ``a`` ``(..., Z, Y, X)`` float64, at the centres:
    along x in increasing offset from 0.0, those sums along y, those along z for ``dims = 3``."""
    a = _box(_box(np.asarray(a, np.float64), r, a.ndim - 1), r, a.ndim - 2)
    return _box(a, r, a.ndim - 3) if dims == 3 else a


def pairs(m):
    """The upper triangle row by row: ``(i, j)`` with ``i <= j``."""
    return [(i, j) for i in range(m) for j in range(i, m)]


def gram(x, r, dims):
    """``(centres.., M, M)`` float64: ``G_ij = sum over the window of x_i x_j``, samples cast to float64 first."""
    x = np.asarray(x, np.float32).astype(np.float64)
    m = x.shape[0]
    g = None
    for i, j in pairs(m):
        s = window_sum(x[i] * x[j], r, dims)
        if g is None:
            g = np.zeros(s.shape + (m, m))
        g[..., i, j] = s
        g[..., j, i] = s
    return g


def jacobi(g, max_sweeps=MAX_SWEEPS):
    """Cyclic Jacobi on a batch ``(n, M, M)`` of symmetric matrices.  Returns ``(w, V, sweeps)``: the diagonal left, the
    accumulated rotations (columns are the eigenvectors) and the sweeps every matrix ran."""
    a = np.array(g, np.float64)
    n, m = a.shape[0], a.shape[1]
    v = np.zeros((n, m, m))
    v[:, range(m), range(m)] = 1.0
    sweeps = np.zeros(n, np.int32)
    pq = [(p, q) for p in range(m) for q in range(p + 1, m)]
    with np.errstate(all="ignore"):
        for _ in range(max_sweeps):
            off = np.zeros(n)
            for p, q in pq:
                off = off + a[:, p, q] * a[:, p, q]
            active = off != 0.0
            if not active.any():
                break
            sweeps += active
            for p, q in pq:
                app, aqq, apq = a[:, p, p], a[:, q, q], a[:, p, q]
                gg = np.abs(apq)
                small = active & (np.abs(app) + gg == np.abs(app)) & (np.abs(aqq) + gg == np.abs(aqq))
                a[small, p, q] = 0.0
                a[small, q, p] = 0.0
                idx = np.flatnonzero(active & (a[:, p, q] != 0.0))
                if idx.size == 0:
                    continue
                app, aqq, apq = a[idx, p, p], a[idx, q, q], a[idx, p, q]
                theta = (aqq - app) / (2.0 * apq)
                t = np.where(theta < 0.0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                ap, aq = a[idx, :, p], a[idx, :, q]
                new_p = c[:, None] * ap - s[:, None] * aq
                new_q = s[:, None] * ap + c[:, None] * aq
                a[idx, :, p] = new_p
                a[idx, p, :] = new_p
                a[idx, :, q] = new_q
                a[idx, q, :] = new_q
                a[idx, p, p] = app - t * apq
                a[idx, q, q] = aqq + t * apq
                a[idx, p, q] = 0.0
                a[idx, q, p] = 0.0
                vp, vq = v[idx, :, p], v[idx, :, q]
                v[idx, :, p] = c[:, None] * vp - s[:, None] * vq
                v[idx, :, q] = s[:, None] * vp + c[:, None] * vq
    return a[:, range(m), range(m)].copy(), v, sweeps


def order(w):
    """Position of every eigenvalue in the ascending order, ties by index: a rank by counting."""
    w = np.asarray(w)
    m = w.shape[-1]
    pos = np.zeros(w.shape, np.int32)
    for i in range(m):
        for j in range(m):
            if j != i:
                pos[..., i] += (w[..., j] < w[..., i]) | ((w[..., j] == w[..., i]) & (j < i))
    return pos


def rank_sigma(s, n_window, estimator=2):
    """``dwidenoise``'s estimator on the ascending eigenvalues ``s`` ``(n, M)``: ``(cut, sigma^2)``; the ``cut`` smallest
    components are noise."""
    s = np.asarray(s, np.float64)
    n, m = s.shape
    q = float(n_window)
    lam_r = np.maximum(s[:, 0], 0.0) / q
    clam, cut, sigsq = np.zeros(n), np.zeros(n, np.int32), np.zeros(n)
    for p in range(m):
        lam = np.maximum(s[:, p], 0.0) / q
        clam = clam + lam
        gam = float(p + 1) / (float(n_window - (m - p - 1)) if estimator == 2 else q)
        a = clam / float(p + 1)
        b = (lam - lam_r) / (4.0 * np.sqrt(gam))
        hit = b < a
        sigsq = np.where(hit, a, sigsq)
        cut = np.where(hit, p + 1, cut).astype(np.int32)
    return cut, sigsq


def projector(v, pos, cut):
    """``(n, M, M)``: the sum of ``v_j v_j^T`` over the components at the ascending positions ``cut .. M-1``, added in
    ascending position from 0.0."""
    n, m = pos.shape
    proj = np.zeros((n, m, m))
    col = np.argsort(pos, axis=1)  # col[:, k]: the column at position k (pos is a permutation)
    for k in range(m):
        vec = np.take_along_axis(v, col[:, None, k:k + 1], axis=2)[:, :, 0]
        proj = proj + np.where((k >= cut)[:, None, None], vec[:, :, None] * vec[:, None, :], 0.0)
    return proj


def centre_shape(nz, ny, nx, r, dims):
    return (nz - 2 * r if dims == 3 else nz, ny - 2 * r, nx - 2 * r)


def clamp_map(field, shape, r, dims):
    """A per-centre field as a per-voxel map: the value at the centre ``clamp(v, r, n-1-r)`` per windowed axis."""
    nz, ny, nx = shape
    iz = np.clip(np.arange(nz), r, nz - 1 - r) - r if dims == 3 else np.arange(nz)
    iy = np.clip(np.arange(ny), r, ny - 1 - r) - r
    ix = np.clip(np.arange(nx), r, nx - 1 - r) - r
    return field[np.ix_(iz, iy, ix)]


def aggregate(x, proj, done, r, dims):
    """Step 6: ``x`` float32 ``(M, Z, Y, X)``, ``proj`` ``(cz, cy, cx, M, M)`` with zeros at unprocessed centres, ``done`` their
    flags.  Returns the float32 output and ``cnt``."""
    x = np.asarray(x, np.float32)
    m = x.shape[0]
    pad = [(2 * r, 2 * r) if dims == 3 else (0, 0), (2 * r, 2 * r), (2 * r, 2 * r)]
    cnt = window_sum(np.pad(done.astype(np.float64), pad), r, dims)
    pbar = {}
    for i, j in pairs(m):
        pbar[i, j] = pbar[j, i] = window_sum(np.pad(proj[..., i, j], pad), r, dims)
    out = np.array(x)
    x64 = x.astype(np.float64)
    has = cnt > 0.0
    with np.errstate(all="ignore"):
        for i in range(m):
            acc = np.zeros(x.shape[1:])
            for j in range(m):
                acc = acc + pbar[i, j] * x64[j]
            out[i] = np.where(has, (acc / cnt).astype(np.float32), x[i])
    return out, cnt.astype(np.int32)


def mppca_parts(x, radius=2, dims=2, estimator=2, mask=None):
    """Every stage of the definition on ``x`` float32 ``(M, Z, Y, X)``: a dict of the per-centre fields (``G``, ``eig``
    ascending, ``cut``, ``sigsq``, ``sweeps``, ``done``, ``P``) and the per-voxel results (``out``, ``sigma``, ``rank``, ``cnt``)."""
    x = np.ascontiguousarray(x, np.float32)
    m, nz, ny, nx, n_window = check(x.shape, radius, dims, estimator)
    r = radius
    cs = centre_shape(nz, ny, nx, r, dims)
    if mask is None:
        at = np.ones(cs, bool)
    else:
        mask = np.asarray(mask)
        if mask.shape != (nz, ny, nx):
            raise ValueError("mask shape does not match the volume")
        at = (mask != 0)[r if dims == 3 else 0:(nz - r) if dims == 3 else nz, r:ny - r, r:nx - r]
    with np.errstate(all="ignore"):
        g = gram(x, r, dims)
    done = at & np.isfinite(g).all(axis=(-1, -2))
    sel = np.flatnonzero(done.reshape(-1))
    w, v, sweeps = jacobi(g.reshape(-1, m, m)[sel])
    pos = order(w)
    s = np.empty_like(w)
    np.put_along_axis(s, pos.astype(np.int64), w, axis=1)
    cut, sigsq = rank_sigma(s, n_window, estimator)
    n_c = int(np.prod(cs))
    proj = np.zeros((n_c, m, m))
    proj[sel] = projector(v, pos, cut)
    sig_c, rank_c = np.zeros(n_c, np.float32), np.zeros(n_c, np.uint8)
    sig_c[sel] = np.sqrt(sigsq).astype(np.float32)
    rank_c[sel] = (m - cut).astype(np.uint8)
    out, cnt = aggregate(x, proj.reshape(cs + (m, m)), done, r, dims)
    full = lambda a, fill, dt: _scatter(a, sel, n_c, fill, dt).reshape(cs + a.shape[1:])
    return {"G": g, "eig": full(s, np.nan, np.float64), "cut": full(cut, 0, np.int32), "sigsq": full(sigsq, 0.0, np.float64),
            "sweeps": full(sweeps, 0, np.int32), "done": done, "P": proj.reshape(cs + (m, m)), "out": out, "cnt": cnt,
            "sigma": np.ascontiguousarray(clamp_map(sig_c.reshape(cs), (nz, ny, nx), r, dims)),
            "rank": np.ascontiguousarray(clamp_map(rank_c.reshape(cs), (nz, ny, nx), r, dims))}


def _scatter(a, sel, n, fill, dtype):
    res = np.full((n,) + a.shape[1:], fill, dtype)
    res[sel] = a
    return res


def mppca(x, radius=2, dims=2, estimator=2, mask=None):
    """``(out float32 (M, Z, Y, X), sigma float32 (Z, Y, X), rank uint8 (Z, Y, X))``."""
    parts = mppca_parts(x, radius, dims, estimator, mask)
    return parts["out"], parts["sigma"], parts["rank"]
