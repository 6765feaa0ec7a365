"""Cases of the MP-PCA denoiser, shared by tests/test_mppca_host.py and tests/test_mppca_gpu.py: the decaying picture the
tests run on, an INDEPENDENT reference written patch by patch with plain loops and np.linalg.eigh (it shares nothing with
fetal_t2mapping_amd/_mppca.py: no box sums, no Jacobi, no batched arrays), a hand-written window sum, and the device
tests' table."""
import functools
import math

import numpy as np

from fetal_t2mapping_amd import _mppca

MAX_TE = 16  # T2FIT_MPPCA_MAX_TE
SIGMA = 20.0


def picture(shape, seed, sigma=SIGMA):
    """``(M, nz, ny, nx)`` float32: two compartments (k 900 / T2 200 ms left, k 600 / T2 70 ms right, the boundary slanted so
    that it crosses windows at every offset) and a third (T2 400 ms) in the lower rows, echoes 40 ms apart, under Rician
    noise.  Windows inside one compartment have rank 1, windows across a boundary rank 2 (asserted where it matters)."""
    rng = np.random.default_rng(seed)
    m, nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    right = 2 * x + y + z >= nx + ny // 2
    k = np.where(right, 600.0, 900.0)
    t2 = np.where(right, 70.0, 200.0)
    low = 3 * y >= 2 * ny
    k, t2 = np.where(low, 750.0, k), np.where(low, 400.0, t2)
    te = 40.0 * (1.0 + np.arange(m))
    clean = k[None] * np.exp(-te[:, None, None, None] / t2[None])
    a = np.hypot(clean + rng.normal(scale=sigma, size=clean.shape), rng.normal(scale=sigma, size=clean.shape))
    return a.astype(np.float32)


# ---- the independent reference ---------------------------------------------------------------------------------------------------
def ref_rank_sigma(w, n_window, estimator):
    """dwidenoise's loop on one ascending spectrum, scalar by scalar: ``(cut, sigma^2, margin)``; ``margin`` is the smallest
    ``|b - a| / a`` over the steps past the first (at the first b = 0 exactly): how far the decision is from a tie."""
    m = len(w)
    q = float(n_window)
    lam_r = max(float(w[0]), 0.0) / q
    clam, cut, sigsq, margin = 0.0, 0, 0.0, math.inf
    for p in range(m):
        lam = max(float(w[p]), 0.0) / q
        clam += lam
        gam = (p + 1) / (q - (m - p - 1)) if estimator == 2 else (p + 1) / q
        a = clam / (p + 1)
        b = (lam - lam_r) / (4.0 * math.sqrt(gam))
        if b < a:
            sigsq, cut = a, p + 1
        if p > 0 and a > 0.0:
            margin = min(margin, abs(b - a) / a)
    return cut, sigsq, margin


def ref_mppca(x, radius, dims, estimator=2, mask=None):
    """The definition, one patch at a time: X (M x N) of the window, eigh of X X^T, the estimator, the projector of the kept
    eigenvectors added to every voxel of the window; then every voxel's mean projector applied to its own samples.
    Returns ``{'eig' (centres, M), 'cut', 'sigsq', 'done' (centre arrays), 'out' float64, 'sigma', 'rank', 'cnt', 'margin'}``."""
    x = np.asarray(x, np.float32).astype(np.float64)
    m, nz, ny, nx = x.shape
    r, rz = radius, radius if dims == 3 else 0
    cs = (nz - 2 * rz, ny - 2 * r, nx - 2 * r)
    eig, cut_c, sig_c = np.full(cs + (m,), np.nan), np.zeros(cs, np.int32), np.zeros(cs)
    done = np.zeros(cs, bool)
    psum, cnt = np.zeros((nz, ny, nx, m, m)), np.zeros((nz, ny, nx), np.int32)
    n_window = (2 * r + 1) ** dims
    margin = math.inf
    for iz in range(cs[0]):
        for iy in range(cs[1]):
            for ix in range(cs[2]):
                vz, vy, vx = iz + rz, iy + r, ix + r
                if mask is not None and not mask[vz, vy, vx]:
                    continue
                win = (slice(vz - rz, vz + rz + 1), slice(vy - r, vy + r + 1), slice(vx - r, vx + r + 1))
                mat = x[(slice(None),) + win].reshape(m, -1)
                assert mat.shape[1] == n_window
                with np.errstate(all="ignore"):
                    g = mat @ mat.T
                if not np.isfinite(g).all():
                    continue
                w, v = np.linalg.eigh(g)
                cut, sigsq, gap = ref_rank_sigma(w, n_window, estimator)
                margin = min(margin, gap)
                keep = v[:, cut:]
                psum[win] += keep @ keep.T
                cnt[win] += 1
                done[iz, iy, ix], eig[iz, iy, ix], cut_c[iz, iy, ix], sig_c[iz, iy, ix] = True, w, cut, sigsq
    out = np.array(x)
    for v in zip(*np.nonzero(cnt)):
        out[(slice(None),) + v] = (psum[v] / cnt[v]) @ x[(slice(None),) + v]
    cz = np.clip(np.arange(nz), rz, nz - 1 - rz) - rz
    cy = np.clip(np.arange(ny), r, ny - 1 - r) - r
    cx = np.clip(np.arange(nx), r, nx - 1 - r) - r
    pick = np.ix_(cz, cy, cx)
    return {"eig": eig, "cut": cut_c, "sigsq": sig_c, "done": done, "out": out, "cnt": cnt, "margin": margin,
            "sigma": np.sqrt(sig_c)[pick] * done[pick], "rank": ((m - cut_c) * done)[pick].astype(np.uint8)}


def loop_window_sum(a, r, dims):
    """The ordered window sum written as a triple loop per centre: x innermost from 0.0, then y, then z."""
    a = np.asarray(a, np.float64)
    nz, ny, nx = a.shape
    rz = r if dims == 3 else 0
    out = np.zeros((nz - 2 * rz, ny - 2 * r, nx - 2 * r))
    for iz in range(out.shape[0]):
        for iy in range(out.shape[1]):
            for ix in range(out.shape[2]):
                sz = 0.0
                for dz in range(2 * rz + 1):
                    sy = 0.0
                    for dy in range(2 * r + 1):
                        sx = 0.0
                        for dx in range(2 * r + 1):
                            sx = sx + float(a[iz + dz, iy + dy, ix + dx])
                        sy = sy + sx
                    sz = sz + sy
                out[iz, iy, ix] = sz
    return out


# (shape, dims, radius, seed) of the statement-against-reference cases.  The seeds are fixed ones for which the statement
# and the reference pick the same rank at every centre (a centre whose b - a is within rounding of 0 could go either way
# between Jacobi's and LAPACK's eigenvalues; none of these cases has one: the smallest |b - a| / a, 'margin', is asserted)
REF_CASES = [((6, 1, 14, 16), 2, 2, 11), ((3, 2, 9, 10), 2, 1, 12), ((4, 5, 7, 8), 3, 1, 13), ((8, 1, 12, 12), 2, 2, 14),
             ((2, 1, 7, 7), 2, 1, 15)]
# .. and the echo counts in between and above: 5 and 7 (device kernels of their own), 9, 12 and 16 (the generic ones)
REF_CASES += [((m, 3, 6, 8), 3, 1, 100 + m) for m in (5, 7, 9, 12, 16)]


@functools.lru_cache(maxsize=None)
def ref_input(shape, seed):
    a = picture(shape, seed)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def ref_case(shape, dims, radius, seed, estimator=2):
    return ref_mppca(ref_input(shape, seed), radius, dims, estimator)


# ---- the device tests' table -------------------------------------------------------------------------------------------------------
# (M, Z, Y, X, dims, r)
GPU_CASES = [(3, 3, 3, 3, 3, 1),       # one centre
             (2, 1, 5, 5, 2, 2),       # one centre, two echoes
             (6, 4, 37, 70, 2, 2),     # ragged, more than one wave per row
             (8, 2, 19, 33, 2, 1),     # the widest register-resident kernel, N = 9 just above M
             (8, 9, 11, 67, 3, 1),
             (8, 7, 21, 35, 3, 2),
             (16, 5, 9, 13, 3, 1),     # the generic kernel at the documented maximum
             (3, 2, 64, 128, 2, 3)]    # tile-aligned
BOTH_ESTIMATORS = [(6, 4, 37, 70, 2, 2), (8, 9, 11, 67, 3, 1)]
# Every echo count: the device compiles its two kernels once per M = 2 .. 8 and once more for 9 .. 16.  The centres of each
# case (544, 280 and 80) fill more than one wave and end in a ragged one.
EVERY_M = ([(m, 2, 6, 70, 2, 1) for m in range(2, 9)] + [(m, 4, 6, 37, 3, 1) for m in range(9, MAX_TE + 1)]
           + [(12, 2, 9, 12, 2, 2), (16, 2, 9, 12, 2, 2)])


@functools.lru_cache(maxsize=None)
def gpu_stack(case):
    a = picture(case[:4], seed=sum(case) * 7919 + case[0])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def gpu_want(case, estimator=2):
    """The statement's ``(out, sigma, rank)`` of a device case, computed once."""
    res = _mppca.mppca(gpu_stack(case), case[5], case[4], estimator)
    for a in res:
        a.setflags(write=False)
    return res


def holes_mask(shape, seed=3):
    """A mask with a border of zeros and holes inside (about one voxel in five)."""
    rng = np.random.default_rng(seed)
    m = (rng.random(shape) > 0.2).astype(np.uint8)
    m[:, :2], m[:, -1:], m[:, :, :1], m[:, :, -3:] = 0, 0, 0, 0
    return m
