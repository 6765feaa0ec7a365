"""Inputs and references shared by test_unring_host.py and test_unring_gpu.py: the band-limited phantoms, an independent
float64 reference of the unringing (numpy.fft for the filter, the Fourier phase ramp for the shifts; it shares no code with
fetal_t2mapping_amd/_unring.py), the error bounds of the float32 chains, and the near-tie rows on which a float64 evaluation
of the same tables picks another shift than the float32 chain.  Everything is built once and read-only."""
import functools

import numpy as np

from fetal_t2mapping_amd import _unring

U32 = 2.0 ** -24  # the unit roundoff of float32


# ---- phantoms ---------------------------------------------------------------------------------------------------------

def _fine_shapes(ny, nx, up):
    """Two nested shapes on the (ny up, nx up) grid at sub-voxel offsets: an ellipse of 100 and, inside it, a disc that
    steps up by 150; coordinates in coarse voxels."""
    y = (np.arange(ny * up) + 0.5) / up
    x = (np.arange(nx * up) + 0.5) / up
    yy, xx = np.meshgrid(y, x, indexing="ij")
    cy, cx = 0.5 * ny + 0.31, 0.5 * nx - 0.43
    img = np.zeros((ny * up, nx * up))
    img[((yy - cy) / (0.36 * ny)) ** 2 + ((xx - cx) / (0.30 * nx)) ** 2 < 1.0] = 100.0
    r = 0.15 * min(ny, nx)
    img[(yy - cy + 1.27) ** 2 + (xx - cx - 0.81) ** 2 < r * r] = 250.0
    return img


def band_limit(fine, ny, nx):
    """The (ny, nx) image whose DFT is the central block of the fine image's DFT: what a truncated k-space acquires."""
    f = np.fft.fftshift(np.fft.fft2(fine))
    fy, fx = fine.shape
    y0, x0 = fy // 2 - ny // 2, fx // 2 - nx // 2
    crop = np.fft.ifftshift(f[y0:y0 + ny, x0:x0 + nx])
    return np.real(np.fft.ifft2(crop)) * (ny * nx) / (fy * fx)


@functools.lru_cache(maxsize=None)
def phantom(ny=48, nx=48, up=8, noise=0.0, seed=0):
    """``(image float32 (ny, nx), truth float64 (ny, nx), flat bool (ny, nx))``: the nested shapes band-limited from the `up`
    times finer grid (plus Gaussian noise); the truth is the fine image averaged over each voxel; `flat` marks the voxels
    whose 5 x 5 neighbourhood of the truth is constant."""
    fine = _fine_shapes(ny, nx, up)
    img = band_limit(fine, ny, nx)
    if noise:
        img = img + noise * np.random.default_rng(seed).standard_normal(img.shape)
    truth = fine.reshape(ny, up, nx, up).mean(axis=(1, 3))
    lo, hi = truth.copy(), truth.copy()
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            s = np.roll(np.roll(truth, dy, 0), dx, 1)
            lo, hi = np.minimum(lo, s), np.maximum(hi, s)
    img = img.astype(np.float32)
    img.setflags(write=False)
    return img, truth, hi == lo


@functools.lru_cache(maxsize=None)
def blob(ny=48, nx=48):
    """A smooth Gaussian blob of height 100 (sigma a sixth of the field of view: it has nothing near the band limit)."""
    yy, xx = np.meshgrid(np.arange(ny) - 0.5 * ny + 0.3, np.arange(nx) - 0.5 * nx - 0.2, indexing="ij")
    b = (100.0 * np.exp(-0.5 * ((yy / (ny / 6.0)) ** 2 + (xx / (nx / 6.0)) ** 2))).astype(np.float32)
    b.setflags(write=False)
    return b


NOISY_SIZES = ((48, 48), (33, 40), (24, 65))


def noisy_phantom(ny, nx):
    """The phantom with noise of standard deviation 1: no two shifts tie exactly."""
    return phantom(ny, nx, 8, 1.0, 7 + ny)[0]


def random_slices(s, ny, nx, seed):
    """Smooth structure, edges and noise: float32 (s, ny, nx)."""
    rng = np.random.default_rng(seed)
    x = 40.0 * rng.standard_normal((s, ny, nx))
    x[:, ny // 3:, nx // 4: nx // 4 + max(3, nx // 3)] += 300.0
    x[:, : ny // 2, : nx // 5] += 120.0
    return x.astype(np.float32)


# ---- the float64 reference --------------------------------------------------------------------------------------------

def ref_split(x):
    """float64 (I1, I2) of slices (S, ny, nx): the 2-D circular filtering by G = cy / (cx + cy) through numpy.fft."""
    x = np.asarray(x, np.float64)
    ny, nx = x.shape[-2:]
    cx = 1.0 + np.cos(2.0 * np.pi * np.fft.fftfreq(nx))[None, :]
    cy = 1.0 + np.cos(2.0 * np.pi * np.fft.fftfreq(ny))[:, None]
    den = cx + cy
    g = np.where(np.abs(den) < 1e-12, 0.5, cy / np.where(np.abs(den) < 1e-12, 1.0, den))
    i1 = np.real(np.fft.ifft2(np.fft.fft2(x, axes=(-2, -1)) * g, axes=(-2, -1)))
    return i1, x - i1


def ref_shifted(rows, K):
    """float64 (2K+1, R, n): the band-limited interpolant of every row at l + s_j, by the phase ramp exp(2 pi i k s / n) (the
    Nyquist term of an even n keeps its real part, cos(pi s))."""
    rows = np.asarray(rows, np.float64)
    n = rows.shape[-1]
    s = np.concatenate([[0.0], np.arange(1, K + 1) / (2 * K + 1.0), -np.arange(1, K + 1) / (2 * K + 1.0)])
    k = np.fft.fftfreq(n) * n
    f = np.fft.fft(rows, axis=-1)
    out = []
    for sj in s:
        ramp = np.exp(2j * np.pi * k * sj / n)
        if n % 2 == 0:
            ramp[n // 2] = np.cos(np.pi * sj)
        out.append(np.real(np.fft.ifft(f * ramp, axis=-1)))
    out[0] = rows.copy()
    return np.stack(out)


def ref_select(y, K, min_w, max_w):
    """``(out, shift, tv, tv_all)`` from the shifted rows y (2K+1, R, n), in the dtype of y: the rule of the method."""
    nj, rows, n = y.shape
    idx = np.arange(n)
    tv_all = np.empty_like(y)
    for j in range(nj):
        d = np.abs(y[j] - y[j][:, (idx - 1) % n])
        tvl, tvr = np.zeros_like(d), np.zeros_like(d)
        for t in range(min_w, max_w + 1):
            tvl += d[:, (idx - t) % n]
            tvr += d[:, (idx + t + 1) % n]
        tv_all[j] = np.minimum(tvl, tvr)
    shift = np.zeros((rows, n), np.int64)
    best = tv_all[0].copy()
    for j in range(1, nj):
        better = tv_all[j] < best
        shift[better], best[better] = j, tv_all[j][better]
    out = y[0].copy()
    for j in range(1, nj):
        sj = (j if j <= K else K - j) / (2 * K + 1.0)
        nb = y[j][:, (idx - 1) % n] if sj > 0 else y[j][:, (idx + 1) % n]
        val = y[j] * (1.0 - abs(sj)) + nb * abs(sj)
        out = np.where(shift == j, val, out)
    return out, shift, best, tv_all


def ref_rows(rows, K, min_w, max_w):
    return ref_select(ref_shifted(rows, K), K, min_w, max_w)[:3]


def ref_unring(x, K=20, min_w=1, max_w=3):
    """float64 (S, ny, nx): the whole method."""
    i1, i2 = ref_split(x)
    s, ny, nx = i1.shape
    ox = ref_rows(i1.reshape(-1, nx), K, min_w, max_w)[0].reshape(s, ny, nx)
    oy = ref_rows(i2.transpose(0, 2, 1).reshape(-1, ny), K, min_w, max_w)[0].reshape(s, nx, ny).transpose(0, 2, 1)
    return ox + oy


# ---- bounds -----------------------------------------------------------------------------------------------------------

def split_bound(x):
    """A bound on the Frobenius norm (and so on every element) of statement - reference for I1 of one slice.  A float32 fma
    chain of length L with table entries rounded once errs, per element, by at most (L + 2) u sum_k |t_k| |d_k|, which is at most
    (L + 2) u sqrt(L) |d|_2 (|t| <= 1, Cauchy-Schwarz); over the M rows of a column, in the 2-norm, sqrt(M L) (L + 2) u |d|_2.
    The exact stage has the gain sqrt(n) in that norm, the filter at most 1 and the later exact stages pass relative errors
    on unchanged, so the relative errors of the four stages add (first order; 1 % is kept for the higher orders, the two
    roundings of the filter product and the final 1 / (nx ny) being folded into G):
      row DFT (M 2nx, L nx): sqrt(2 nx) (nx + 2) u;   column DFT and its inverse (M 2ny, L 2ny): 2 sqrt(ny) (2ny + 2) u each;
      inverse row DFT (M nx, L 2nx): sqrt(2 nx) (2nx + 2) u;   the filter product: 2 u."""
    ny, nx = x.shape[-2:]
    rel = np.sqrt(2.0 * nx) * (nx + 2) + 2 * 2.0 * np.sqrt(ny) * (2 * ny + 2) + np.sqrt(2.0 * nx) * (2 * nx + 2) + 2.0
    return 1.01 * rel * U32 * float(np.linalg.norm(np.asarray(x, np.float64)))


def shifted_bound(rows):
    """Per row, a bound on |Y_j[l] statement - reference| for every j and l: the chain of length n errs by at most
    (n + 2) u sum_m |h| |x| <= (n + 2) u |h_j|_2 |x|_2, and |h_j|_2 <= 1 (h_j is a row of a unitary shift; for an even n and
    s != 0 it is below 1)."""
    rows = np.asarray(rows, np.float64)
    n = rows.shape[-1]
    return 1.01 * (n + 2) * U32 * np.linalg.norm(rows, axis=-1)


def tv_bound(rows, min_w, max_w, tv):
    """(R, 1), a bound on |winning tv statement - reference|: |min_j a_j - min_j b_j| <= max_j |a_j - b_j|; a tv is a sum of
    W = max_w - min_w + 1 terms |Y[i] - Y[i-1]|, each off by at most 2 eps_Y plus its own rounding, and W - 1 additions."""
    w = max_w - min_w + 1
    return (2.0 * w * shifted_bound(rows) + (w + 2) * U32 * np.max(np.abs(tv), axis=-1) * 1.01)[:, None]


def value_bound(rows, out):
    """(R, 1): the output of an agreed shift is a convex combination of two samples of Y_j (eps_Y) plus three roundings."""
    return (shifted_bound(rows) + 4 * U32 * np.max(np.abs(out), axis=-1))[:, None]


# ---- near ties ----------------------------------------------------------------------------------------------------------

def select_f64_tables(rows, h, K, min_w, max_w):
    """The shift a float64 evaluation of the same float32 tables and rows picks: (R, n) int64."""
    hc = _unring.circulant(np.asarray(h, np.float32)).astype(np.float64)
    y = np.einsum("jlm,rm->jrl", hc, np.asarray(rows, np.float64))
    y[0] = np.asarray(rows, np.float64)
    return ref_select(y, K, min_w, max_w)[1]


def _tv_row_f64(row, hc64, K, min_w, max_w):
    """float64 (2K+1, n): the tv of every shift along one float32 row, from the float32 taps evaluated in float64."""
    y = np.einsum("jlm,m->jl", hc64, row.astype(np.float64))
    y[0] = row
    return ref_select(y[:, None, :], K, min_w, max_w)[3][:, 0, :]


def _tie_rows(row, pos, hc64, K, min_w, max_w):
    """Two copies of `row` that differ in one float32 step of the sample next to `pos`, between which the best and the
    second-best shift at `pos` (of the float64 evaluation) change places; None when moving that sample by up to 16 does
    not make them tie."""
    p = (pos + 1) % row.size
    tv = _tv_row_f64(row, hc64, K, min_w, max_w)[:, pos]
    j1, j2 = np.argsort(tv, kind="stable")[:2]

    def gap(v):
        r = row.copy()
        r[p] = v
        t = _tv_row_f64(r, hc64, K, min_w, max_w)[:, pos]
        return t[j2] - t[j1]

    lo = np.float32(row[p])
    hi = None
    for step in (0.25, -0.25, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 4.0, -4.0, 8.0, -8.0, 16.0, -16.0):
        if gap(np.float32(lo + step)) < 0:
            hi = np.float32(lo + step)
            break
    if hi is None:
        return None
    while True:  # bisection over the float32 values between lo (gap > 0) and hi (gap < 0)
        mid = np.float32(0.5 * (float(lo) + float(hi)))
        if mid == lo or mid == hi:
            break
        if gap(mid) < 0:
            hi = mid
        else:
            lo = mid
    out = []
    for v in (lo, hi):
        r = row.copy()
        r[p] = v
        out.append(r)
    return out


@functools.lru_cache(maxsize=None)
def near_tie_case():
    """Rows of length 40 (K 20, window 1 .. 3) on which the float32 chain picks another shift than a float64 evaluation of the
    same tables on at least 10 samples.  The phantoms do not yield them (best and second-best tv lie 0.05 .. 0.1 apart, the
    chains err by 1e-4), and scaling a row scales every tv alike, so the ties are built: one sample of a row of the noisy
    33 x 40 phantom's I1 is moved, by bisection over the float32 values, to where the best and the second-best shift of a
    neighbouring position change places; on the two rows either side of that point the two tv differ by about one float32
    step of the moved sample, far less than the chain's error.  A device kernel with another summation order fails here.
    Returns (rows float32 (R, 40), tables, shift of the statement (R, 40), number of differing samples)."""
    ny, nx, K = 33, 40, 20
    t = _unring.Tables(ny, nx, K)
    base = _unring.split(noisy_phantom(ny, nx)[None], t)[0][0]
    hc64 = _unring.circulant(t.hx).astype(np.float64)
    rows = []
    for r in range(ny):
        for pos in (6, 17, 29):
            pair = _tie_rows(base[r].copy(), pos, hc64, K, 1, 3)
            if pair is not None:
                rows += pair
    rows = np.stack(rows)
    shift32 = _unring.unring_rows(rows, t.hx, t.ab, 1, 3)[1].astype(np.int64)
    shift64 = select_f64_tables(rows, t.hx, K, 1, 3)
    differ = int(np.sum(shift32 != shift64))
    assert differ >= 10, f"only {differ} samples where the float64 evaluation picks another shift: the case does not bite"
    rows.setflags(write=False)
    shift32.setflags(write=False)
    return rows, t, shift32, differ
