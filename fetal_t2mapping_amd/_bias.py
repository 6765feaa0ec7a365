"""N4 bias-field correction stated in numpy (include/t2fit.h holds the same definition in words).

Stands for the reference's ``run_biasfield_correction`` / ``run_biasfield_correction2`` (utils/qmri_utils.py:254-357),
which call ``sitk.N4BiasFieldCorrectionImageFilter``.  Written from the N4 paper (Tustison 2010), the multilevel
B-spline paper (Lee, Wolberg and Shin 1997) and ITK's documentation; parity with ITK is unpinned.

Every per-voxel volume is float32 in memory; all arithmetic is float64 with one rounding at the store, every multiply and
add rounding once (no fused multiply-add).  The steps the device repeats per voxel are functions here (``log_image``,
``minmax``, ``histogram``, ``fit_weights``, ``fit_delta``, ``field_eval``, ``convergence_sums``, ``apply_field``); the
sharpening table, the lattice refinement, the convergence figure and the loop are host code that the device path runs
unchanged (:func:`n4_loop` over a steps object: :class:`HostSteps` here, ``_gpu_bias.DeviceSteps`` there).
"""
import math

import numpy as np

LANES = 64          # terms l, l + 64, .. of a row go to lane l
FAN = 256           # a pass of the tree over the rows adds groups of 256 by halving
FIX = 1 << 24       # the histogram is fixed point: a voxel weighs 2^24
BINS = 200
MAX_BINS = 1024
SIDES = (4, 5, 7, 11, 19)   # lattice side per level: 4, then 2 c - 3
DEFAULT_ITER = (50, 50, 50, 50)


# ---- 1. log image --------------------------------------------------------------------------------------------------------
def as_volume(vol, what="volume"):
    v = np.ascontiguousarray(vol, np.float32)
    if v.ndim != 3:
        raise ValueError(f"{what} must be 3-D (z, y, x), got shape {v.shape}")
    return v


def log_image(vol, mask=None):
    """``M = mask and vol > 0`` (uint8) and ``u0 = float32(log(float64(vol)))`` in M, +0.0 elsewhere."""
    v = as_volume(vol)
    m = v > 0
    if mask is not None:
        if np.shape(mask) != v.shape:
            raise ValueError("the mask has the shape of the volume")
        m &= np.asarray(mask) != 0
    u0 = np.zeros(v.shape, np.float32)
    u0[m] = np.log(v[m].astype(np.float64)).astype(np.float32)
    return u0, m.astype(np.uint8)


def minmax(u, m):
    """(lo, hi) of ``u`` over M as float32; (+inf, -inf) when M is empty."""
    sel = np.asarray(u, np.float32)[np.asarray(m) != 0]
    if sel.size == 0:
        return np.float32(np.inf), np.float32(-np.inf)
    return sel.min(), sel.max()


# ---- 2. sharpening -------------------------------------------------------------------------------------------------------
def slope_of(lo, hi, bins=BINS):
    lo, hi = float(lo), float(hi)
    if not hi > lo:
        raise ValueError("N4: the log image is flat (or empty) inside the mask: there is no histogram to sharpen")
    return (hi - lo) / (bins - 1)


def bin_coords(u, lo, slope, bins=BINS):
    """``c = clamp((float64(u) - lo) / slope, 0, B - 1)``, ``i = min(floor(c), B - 2)``, ``t = c - i``."""
    c = (np.asarray(u).astype(np.float64) - float(lo)) / float(slope)
    c = np.minimum(np.maximum(c, 0.0), bins - 1.0)
    i = np.minimum(np.floor(c), bins - 2.0)
    return i.astype(np.int64), c - i


def histogram(u, m, lo, slope, bins=BINS):
    """uint64 ``[bins]``: every voxel of M adds ``2^24 - w`` to bin ``i`` and ``w = floor(t 2^24 + 0.5)`` to bin ``i + 1``."""
    i, t = bin_coords(np.asarray(u)[np.asarray(m) != 0], lo, slope, bins)
    w = np.floor(t * FIX + 0.5).astype(np.uint64)
    hist = np.zeros(bins, np.uint64)
    np.add.at(hist, i, np.uint64(FIX) - w)
    np.add.at(hist, i + 1, w)
    return hist


def padded_size(bins):
    return 1 << (int(math.ceil(math.log2(bins))) + 1)


def sharpen_table(hist, lo, slope, fwhm, noise=0.01, fft=np.fft.fft, ifft=np.fft.ifft):
    """``E[b]``: the expected true log intensity of bin ``b`` after the histogram is deconvolved (Wiener, ``noise``) by a
    Gaussian of full width ``fwhm`` (in log intensity).  Host code, shared by both paths."""
    hist = np.asarray(hist)
    bins = hist.size
    lo, slope, fwhm = float(lo), float(slope), float(fwhm)
    if not (fwhm > 0.0 and noise > 0.0):
        raise ValueError("N4: fwhm and noise must be > 0")
    p = padded_size(bins)
    o = (p - bins) // 2
    v = np.zeros(p)
    v[o:o + bins] = hist.astype(np.float64) / FIX
    width = fwhm / slope
    e = 4.0 * math.log(2.0) / (width * width)
    s = 2.0 * math.sqrt(math.log(2.0) / math.pi) / width
    f = np.zeros(p)
    f[0] = s
    n = np.arange(1, p // 2 + 1)
    g = s * np.exp(-(n * n) * e)
    f[n] = g
    f[p - n] = g
    ff = fft(f)
    wiener = np.conj(ff) / (np.conj(ff) * ff + noise)
    u = np.maximum(np.real(ifft(fft(v) * np.real(wiener))), 0.0)
    x = lo + (np.arange(p) - o) * slope
    num = np.real(ifft(fft(x * u) * ff))
    den = np.real(ifft(fft(u) * ff))
    table = np.zeros(p)
    np.divide(num, den, out=table, where=den != 0.0)
    return np.ascontiguousarray(table[o:o + bins])


def residual(u, m, table, lo=0.0, slope=1.0):
    """float64 ``u - (E[i] (1 - t) + E[i + 1] t)`` in M, +0.0 elsewhere; ``table`` None: ``u`` itself."""
    ud = np.asarray(u).astype(np.float64)
    if table is not None:
        table = np.asarray(table, np.float64)
        i, t = bin_coords(u, lo, slope, table.size)
        ud = ud - (table[i] * (1.0 - t) + table[i + 1] * t)
    return np.where(np.asarray(m) != 0, ud, 0.0)


# ---- 3. fit --------------------------------------------------------------------------------------------------------------
def bspline(tau):
    """The four uniform cubic B-spline weights, ``[..., 4]``, in the order of operations the kernels use."""
    t2 = tau * tau
    t3 = t2 * tau
    om = 1.0 - tau
    return np.stack([((om * om) * om) / 6.0, ((3.0 * t3 - 6.0 * t2) + 4.0) / 6.0,
                     (((-3.0 * t3 + 3.0 * t2) + 3.0 * tau) + 1.0) / 6.0, t3 / 6.0], axis=-1)


def axis_weights(n, c):
    """Along an axis of ``n`` voxels under a lattice of side ``c``: the first node ``k[n]`` and, at nodes ``k .. k + 3``,
    the weights ``b[n, 4]``, ``a = b^3 / S`` and ``q = b^2`` with ``S = ((b0^2 + b1^2) + b2^2) + b3^2``."""
    s = c - 3
    if n == 1:
        k, tau = np.zeros(1), np.zeros(1)
    else:
        p = np.arange(n, dtype=np.float64) * s / (n - 1)
        k = np.floor(p)
        tau = p - k
        k[-1], tau[-1] = s - 1, 1.0
    b = bspline(tau)
    q = b * b
    ssq = ((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3]
    return k.astype(np.int64), b, (q * b) / ssq[:, None], q


def dense(k, w, c):
    """``[n, c]``: the four weights at their nodes, every other weight 0."""
    out = np.zeros((len(k), c))
    out[np.arange(len(k))[:, None], k[:, None] + np.arange(4)] = w
    return out


def row_tree(terms):
    """The sum along the last axis in the order of a wave: zero-padded to a multiple of 64, lane ``l`` adds terms
    ``l, l + 64, ..`` in order from +0.0, then the 64 lanes halve (32, 16, .. 1)."""
    terms = np.asarray(terms, np.float64)
    nx = terms.shape[-1]
    groups = -(-nx // LANES)
    p = np.zeros(terms.shape[:-1] + (groups * LANES,))
    p[..., :nx] = terms
    p = p.reshape(terms.shape[:-1] + (groups, LANES))
    acc = np.zeros(terms.shape[:-1] + (LANES,))
    for j in range(groups):
        acc = acc + p[..., j, :]
    h = LANES // 2
    while h >= 1:
        acc = acc[..., :h] + acc[..., h:2 * h]
        h //= 2
    return acc[..., 0]


def tree256(values):
    """Passes of 256-to-1 halving groups (the last group padded with zeros) until one value is left; at least one pass."""
    v = np.asarray(values, np.float64).ravel()
    while True:
        groups = max(-(-v.size // FAN), 1)
        p = np.zeros(groups * FAN)
        p[:v.size] = v
        p = p.reshape(groups, FAN)
        h = FAN // 2
        while h >= 1:
            p = p[:, :h] + p[:, h:2 * h]
            h //= 2
        v = p[:, 0]
        if groups == 1:
            return float(v[0])


def contract(values, wz, wy, wx):
    """``out[cz, cy, cx] = sum_z wz[z, cz] sum_y wy[y, cy] sum_x wx[x, cx] values[z, y, x]``: x by :func:`row_tree`, then y,
    then z in index order from +0.0; the weights are dense ``[n, c]``."""
    c = wx.shape[1]
    nz, ny, _ = values.shape
    xs = np.stack([row_tree(values * wx[:, cx]) for cx in range(c)], axis=-1)  # [nz, ny, c]
    ys = np.zeros((nz, c, c))
    for y in range(ny):
        ys = ys + wy[y][None, :, None] * xs[:, y, None, :]
    out = np.zeros((c, c, c))
    for z in range(nz):
        out = out + wz[z][:, None, None] * ys[z][None, :, :]
    return out


def _dense_axes(shape, c, which):
    return [dense(k, (b, a, q)[which], c) for k, b, a, q in (axis_weights(n, c) for n in shape)]


def fit_weights(m, c):
    """``omega[cz, cy, cx] = sum over M of qz qy qx``: depends on M and the level only."""
    m = np.asarray(m) != 0
    return contract(m.astype(np.float64), *_dense_axes(m.shape, c, 2))


def fit_delta(u, m, c, table=None, lo=0.0, slope=1.0):
    """``delta[cz, cy, cx] = sum over M of az ay ax r`` with the residual ``r`` of :func:`residual`."""
    r = residual(u, m, table, lo, slope)
    return contract(r, *_dense_axes(r.shape, c, 1))


def lattice_update(lattice, delta, omega):
    inc = np.zeros_like(delta)
    np.divide(delta, omega, out=inc, where=omega != 0.0)
    return lattice + inc


# ---- 4. field ------------------------------------------------------------------------------------------------------------
def field_eval(lattice, shape, store=np.float32):
    """float32 field at every voxel of ``shape``: z, then y, then x, four taps each, added in tap order (``store``: the
    type of the one rounding at the end)."""
    lattice = np.asarray(lattice, np.float64)
    c = lattice.shape[0]
    (kz, bz, _, _), (ky, by, _, _), (kx, bx, _, _) = (axis_weights(n, c) for n in shape)
    t1 = bz[:, 0, None, None] * lattice[kz]
    for j in range(1, 4):
        t1 = t1 + bz[:, j, None, None] * lattice[kz + j]          # [nz, c, c]
    t2 = by[None, :, 0, None] * t1[:, ky, :]
    for j in range(1, 4):
        t2 = t2 + by[None, :, j, None] * t1[:, ky + j, :]          # [nz, ny, c]
    f = bx[None, None, :, 0] * t2[:, :, kx]
    for j in range(1, 4):
        f = f + bx[None, None, :, j] * t2[:, :, kx + j]
    return f.astype(store)


# ---- 5. convergence ------------------------------------------------------------------------------------------------------
def convergence_terms(field_new, field_old, m):
    d = np.expm1(np.asarray(field_new).astype(np.float64) - np.asarray(field_old).astype(np.float64))
    return np.where(np.asarray(m) != 0, d, 0.0)


def convergence_sums(field_new, field_old, m):
    """(sum d, sum d^2) of ``d = expm1(field_new - field_old)`` over M: rows by :func:`row_tree`, the rows in (z, y)
    order by :func:`tree256`."""
    d = convergence_terms(field_new, field_old, m)
    return tree256(row_tree(d)), tree256(row_tree(d * d))


def convergence(sum_d, sum_dd, n):
    """The coefficient of variation of ``exp`` of the field's change, N4's stopping figure.  Host code."""
    if n < 2:
        return 0.0
    var = (sum_dd - sum_d * sum_d / n) / (n - 1)
    return math.sqrt(max(var, 0.0)) / (1.0 + sum_d / n)


def next_u(u0, field, m):
    u = (np.asarray(u0).astype(np.float64) - np.asarray(field).astype(np.float64)).astype(np.float32)
    return np.where(np.asarray(m) != 0, u, np.float32(0.0))


# ---- 6. next level -------------------------------------------------------------------------------------------------------
def refine(lattice):
    """Cubic subdivision of every axis, side ``c -> 2 c - 3``; the field is unchanged.  Host code."""
    out = np.asarray(lattice, np.float64)
    if 2 * out.shape[0] - 3 > SIDES[-1]:
        raise ValueError(f"N4: a lattice side above {SIDES[-1]} is refused (at most {len(SIDES)} levels)")
    for axis in range(3):
        a = np.moveaxis(out, axis, 0)
        new = np.empty((2 * a.shape[0] - 3,) + a.shape[1:])
        new[0::2] = (a[:-1] + a[1:]) / 2.0
        new[1::2] = (a[:-2] + 6.0 * a[1:-1] + a[2:]) / 8.0
        out = np.moveaxis(new, 0, axis)
    return np.ascontiguousarray(out)


# ---- 7. output -----------------------------------------------------------------------------------------------------------
def apply_field(vol, log_field, scale=1.0):
    """``float32(float64(vol) / exp(float64(log_field)) * scale)`` at every voxel."""
    v, f = as_volume(vol), as_volume(log_field, "log_field")
    if v.shape != f.shape:
        raise ValueError("the field has the shape of the volume")
    return (v.astype(np.float64) / np.exp(f.astype(np.float64)) * float(scale)).astype(np.float32)


# ---- the loop ------------------------------------------------------------------------------------------------------------
class N4Result:
    """``corrected`` float32 volume, ``log_field`` float32 (the estimated log bias at every voxel), ``lattice`` float64
    ``[c, c, c]`` of the last level, ``iterations`` per level, ``convergence``: every iteration's figure, per level."""

    def __init__(self, corrected, log_field, lattice, iterations, convergence):  # noqa: A002
        self.corrected, self.log_field, self.lattice = corrected, log_field, lattice
        self.iterations, self.convergence = tuple(iterations), tuple(tuple(c) for c in convergence)

    def __repr__(self):
        return f"N4Result(iterations={self.iterations}, last convergence={[c[-1] for c in self.convergence if c]})"


def check_options(fwhm, max_iter, threshold, bins, noise, scale):
    max_iter = tuple(int(i) for i in np.atleast_1d(max_iter))
    if not 1 <= len(max_iter) <= len(SIDES) or any(i < 0 for i in max_iter):
        raise ValueError(f"N4: max_iter holds 1..{len(SIDES)} non-negative counts (a lattice side above {SIDES[-1]} is "
                         f"refused), got {max_iter!r}")
    bins = int(bins)
    if not 2 <= bins <= MAX_BINS:
        raise ValueError(f"N4: bins is outside 2..{MAX_BINS}")
    if not (float(fwhm) > 0.0 and float(noise) > 0.0 and math.isfinite(float(scale)) and float(threshold) >= 0.0):
        raise ValueError("N4: fwhm and noise must be > 0, threshold >= 0 and scale finite")
    return max_iter, bins


class HostSteps:
    """The per-voxel steps in numpy; the device path has the same methods."""

    def __init__(self, vol, mask, log=None):
        self.vol = as_volume(vol)
        if not np.all(np.isfinite(self.vol)):
            raise ValueError("N4: the volume must be finite")
        self.u0, self.m = log_image(self.vol, mask) if log is None else log
        self.u = self.u0.copy()
        self.field = np.zeros(self.vol.shape, np.float32)

    def range(self):  # noqa: A003
        return minmax(self.u, self.m)

    def set_level(self, lattice):
        self.lat = np.array(lattice, np.float64)
        self.omega = fit_weights(self.m, self.lat.shape[0])

    def histogram(self, lo, slope, bins):
        return histogram(self.u, self.m, lo, slope, bins)

    def fit(self, table, lo, slope):
        delta = fit_delta(self.u, self.m, self.lat.shape[0], table, lo, slope)
        self.lat = lattice_update(self.lat, delta, self.omega)

    def eval_field(self):
        new = field_eval(self.lat, self.vol.shape)
        sums = convergence_sums(new, self.field, self.m)
        self.field, self.u = new, next_u(self.u0, new, self.m)
        return sums + self.range()

    def lattice(self):
        return self.lat

    def finish(self, scale):
        return apply_field(self.vol, self.field, scale), self.field


def n4_loop(steps, *, fwhm=0.15, max_iter=DEFAULT_ITER, threshold=1e-3, bins=BINS, noise=0.01, scale=1.0):
    """Levels of: range, histogram, table, fit, field, convergence, until ``conv <= threshold`` or the level's budget."""
    max_iter, bins = check_options(fwhm, max_iter, threshold, bins, noise, scale)
    lo, hi = steps.range()
    lattice = np.zeros((SIDES[0],) * 3)
    iterations, history = [], []
    for level, budget in enumerate(max_iter):
        if level:
            lattice = refine(lattice)
        steps.set_level(lattice)
        figures = []
        while len(figures) < budget:
            slope = slope_of(lo, hi, bins)
            hist = steps.histogram(float(lo), slope, bins)
            table = sharpen_table(hist, lo, slope, fwhm, noise)
            steps.fit(table, float(lo), slope)
            sum_d, sum_dd, lo, hi = steps.eval_field()
            figures.append(convergence(sum_d, sum_dd, int(hist.sum(dtype=np.uint64)) >> 24))
            if figures[-1] <= threshold:
                break
        lattice = np.array(steps.lattice(), np.float64)
        iterations.append(len(figures))
        history.append(figures)
    corrected, field = steps.finish(float(scale))
    return N4Result(corrected, field, lattice, iterations, history)


def n4_correct(volume, mask=None, *, fwhm=0.15, max_iter=DEFAULT_ITER, threshold=1e-3, bins=BINS, noise=0.01, scale=1.0,
               log=None):
    """The whole correction on the host.  ``mask`` None: ``_register.build_mask`` of the volume.  ``log``: a
    ``(u0, M)`` pair to use in place of :func:`log_image` (the tests hand in the device's own log image)."""
    if mask is None and log is None:
        from ._register import build_mask

        mask = build_mask(as_volume(volume))
    return n4_loop(HostSteps(volume, mask, log), fwhm=fwhm, max_iter=max_iter, threshold=threshold, bins=bins, noise=noise,
                   scale=scale)
