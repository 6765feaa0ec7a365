"""Cases of the vector-valued (joint) TV denoiser, shared by tests/test_tvj_host.py and tests/test_tvj_gpu.py: an
INDEPENDENT reference written voxel by voxel with scalar operations of the working precision (no slice tables, no numpy
array arithmetic: it shares nothing with fetal_t2mapping_amd/_tv.py), mutations of the statement the reference must notice,
the shapes of the device tests, and the multi-echo phantom of the benefit test."""
import contextlib
import functools
import itertools
import math

import numpy as np

from fetal_t2mapping_amd import _tv

DTYPE = {"f32": np.float32, "f64": np.float64}
WEIGHT = 25.0


def field(shape, seed, sigma=20.0):
    """``(C, nz, ny, nx)`` float32: steps along every axis shared by the channels (a common edge set), a decaying level
    per channel, and noise: all values in the hundreds, so float32 rounding matters at every voxel."""
    rng = np.random.default_rng(seed)
    c, nz, ny, nx = shape
    ch, z, y, x = np.meshgrid(np.arange(c), np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    clean = (300.0 + 600.0 * (2 * x >= nx) + 400.0 * (2 * y >= ny) + 200.0 * (z % 2)) * np.exp(-0.25 * ch)
    return (clean + rng.normal(scale=sigma, size=shape)).astype(np.float32)


# ---- the independent reference -------------------------------------------------------------------------------------------------
def ref_joint(f, weight, max_iter, dtype):
    """The definition of include/t2fit.h for one joint problem ``f`` ``(C, Y, X)`` or ``(C, Z, Y, X)``, ``max_iter``
    iterations (no stop rule): every number a scalar of ``dtype``, every operation one scalar operation in the order the
    header writes it.  Returns ``(out, E)`` of the last iteration; the two sums of E are exact (math.fsum) float64 sums."""
    T = np.dtype(dtype).type
    f = np.asarray(f)
    chans, sp = f.shape[0], f.shape[1:]
    n = len(sp)
    tau, tw, one = T(1.0 / (2.0 * n)), T((1.0 / (2.0 * n)) / float(weight)), T(1.0)
    vox = list(itertools.product(*[range(s) for s in sp]))

    def shifted(x, a, by):
        return tuple(v + by if b == a else v for b, v in enumerate(x))

    p = {(c, a, x): T(0.0) for c in range(chans) for a in range(n) for x in vox}
    out, e = {}, 0.0
    with np.errstate(all="ignore"):
        for i in range(max_iter):
            d = {}
            for c in range(chans):
                for x in vox:
                    if i == 0:
                        d[c, x] = T(0.0)
                        continue
                    s = p[c, 0, x] + p[c, 1, x]
                    if n == 3:
                        s = s + p[c, 2, x]
                    v = -s
                    for a in range(n):
                        if x[a] > 0:
                            v = v + p[c, a, shifted(x, a, -1)]
                    d[c, x] = v
            out = {(c, x): T(f[(c,) + x]) + d[c, x] for c in range(chans) for x in vox}
            g = {(c, a, x): (out[c, shifted(x, a, 1)] - out[c, x]) if x[a] + 1 < sp[a] else T(0.0)
                 for c in range(chans) for a in range(n) for x in vox}
            nrm = {}
            for x in vox:
                s = None
                for c in range(chans):
                    sq = g[c, 0, x] * g[c, 0, x] + g[c, 1, x] * g[c, 1, x]
                    if n == 3:
                        sq = sq + g[c, 2, x] * g[c, 2, x]
                    s = sq if c == 0 else s + sq
                nrm[x] = np.sqrt(s)
            e = (math.fsum(float(v * v) for v in d.values()) + float(weight) * math.fsum(float(v) for v in nrm.values())) \
                / (chans * len(vox))
            for c in range(chans):
                for x in vox:
                    den = one + tw * nrm[x]
                    for a in range(n):
                        p[c, a, x] = (p[c, a, x] - tau * g[c, a, x]) / den
    res = np.empty(f.shape, T)
    for (c, x), v in out.items():
        res[(c,) + x] = v
    return res, e


# (C, spatial shape) of the reference's cases; the largest are (3, 4, 5) and (3, 3, 4, 5)
REF_CASES = [(1, (4, 5)), (2, (3, 4)), (3, (4, 5)), (3, (1, 5)), (1, (3, 4, 5)), (2, (2, 3, 4)), (3, (3, 4, 5)), (3, (2, 1, 3))]
REF_ITERS = 4
E_RTOL = 1e-13  # the statement sums E's terms with np.sum (pairwise float64), the reference exactly: a few 1e-16 apart


@functools.lru_cache(maxsize=None)
def ref_input(chans, sp):
    a = field((chans, 1) + sp if len(sp) == 2 else (chans,) + sp, seed=1000 * chans + sum(sp))
    a = a[:, 0] if len(sp) == 2 else a
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def ref_case(chans, sp, precision):
    return ref_joint(ref_input(chans, sp), WEIGHT, REF_ITERS, DTYPE[precision])


def statement_matches_reference(chans, sp, precision):
    """True when the statement's out is bit-equal to the reference's and its E within E_RTOL, n_iter = REF_ITERS - 1."""
    want, want_e = ref_case(chans, sp, precision)
    got, n_iter, e = _tv.tv_joint_problem(ref_input(chans, sp), WEIGHT, 0.0, REF_ITERS, DTYPE[precision])
    assert got.dtype == want.dtype and got.shape == want.shape and n_iter == REF_ITERS - 1
    return got.tobytes() == want.tobytes() and abs(e - want_e) <= E_RTOL * want_e


# ---- mutations of the statement ------------------------------------------------------------------------------------------------
_update, _joint_norm, _joint_energy = _tv.update, _tv.joint_norm, _tv.joint_energy


def _update_per_channel_norm(p, g, nrm, tau, tw):
    sq = g[0] * g[0] + g[1] * g[1]
    if len(g) == 3:
        sq = sq + g[2] * g[2]
    return _update(p, g, np.sqrt(sq), tau, tw)


def _joint_norm_descending(g):
    return _joint_norm(g[::-1])


def _joint_energy_over_spatial_count(d, nrm, weight):
    return _joint_energy(d, nrm, weight) * len(d)


# name: (attribute of _tv, the wrong variant)
MUTATIONS = {"per_channel_norm_in_the_update": ("update", _update_per_channel_norm),
             "s_summed_in_descending_channel_order": ("joint_norm", _joint_norm_descending),
             "energy_divided_by_the_spatial_count": ("joint_energy", _joint_energy_over_spatial_count)}


@contextlib.contextmanager
def mutated(name):
    attr, fn = MUTATIONS[name]
    saved = getattr(_tv, attr)
    setattr(_tv, attr, fn)
    try:
        yield
    finally:
        setattr(_tv, attr, saved)


# ---- the device tests' shapes ---------------------------------------------------------------------------------------------------
MAX_CHAN = 64  # T2FIT_TV_JOINT_MAX_CHAN
# (C, nz, ny, nx): what the entry is for.  Tiles are 32 x 64 (2-D) and 4 x 8 x 64 (3-D); 128-bit accesses when nx % 4 == 0.
GPU_SHAPES = [(3, 5, 33, 65),          # ragged in every axis, element-wise path, two tiles in y and x
              (2, 9, 9, 68),           # vector path, the x halo inside the tile row, three z tiles in 3-D
              (1, 3, 8, 64),           # C = 1: also against the scalar kernel
              (8, 2, 32, 64),          # exact tiles
              (16, 1, 5, 4),           # 16 channels
              (MAX_CHAN, 1, 3, 4),     # the documented maximum
              (3, 1, 1, 7),            # 1-wide axes
              (3, 4, 1, 1)]
GPU_ITERS = (1, 2, 7)


@functools.lru_cache(maxsize=None)
def gpu_stack(shape):
    a = field(shape, seed=sum(shape) * 7919 + shape[0])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def gpu_want(shape, dims, precision, max_iter):
    """The statement's (out, n_iter, energy) of a device case at eps = 0, computed once."""
    return _tv.denoise_tv_joint(gpu_stack(shape), WEIGHT, 0.0, max_iter, dims, precision)


# ---- the multi-echo phantom of the benefit test ----------------------------------------------------------------------------------
PH_TE = np.array([80.0, 114.0, 150.0, 202.0, 250.0, 299.0])
PH_SIGMA, PH_SEED, PH_ITERS = 25.0, 0, 100
PH_WEIGHTS = (0.5, 1.0, 2.0, 3.0)  # in units of PH_SIGMA


@functools.lru_cache(maxsize=None)
def phantom():
    """``(noisy (6, 64, 64) float32, true T2 (64, 64))``: piecewise constant, background k 700 / T2 120, a disc of radius 20
    at k 900 / T2 200, a small disc of radius 8 at k 600 / T2 80, a strip of T2 300; Rician noise of sigma 25, seed 0."""
    y, x = np.meshgrid(np.arange(64.0), np.arange(64.0), indexing="ij")
    k, t2 = np.full((64, 64), 700.0), np.full((64, 64), 120.0)
    big = (y - 28) ** 2 + (x - 28) ** 2 < 20.0 ** 2
    k[big], t2[big] = 900.0, 200.0
    small = (y - 53) ** 2 + (x - 53) ** 2 < 8.0 ** 2
    k[small], t2[small] = 600.0, 80.0
    t2[:, 58:62] = np.where(small[:, 58:62], t2[:, 58:62], 300.0)
    clean = k[None] * np.exp(-PH_TE[:, None, None] / t2[None])
    rng = np.random.default_rng(PH_SEED)
    noisy = np.hypot(clean + rng.normal(scale=PH_SIGMA, size=clean.shape), rng.normal(scale=PH_SIGMA, size=clean.shape))
    noisy = noisy.astype(np.float32)
    for a in (noisy, t2):
        a.setflags(write=False)
    return noisy, t2


def loglin_t2(stack):
    """Unweighted log-linear least-squares T2 per voxel, clipped to 10 .. 2000 ms."""
    logs = np.log(np.maximum(np.asarray(stack, np.float64), 1e-6))
    te = PH_TE - PH_TE.mean()
    slope = np.tensordot(te, logs - logs.mean(axis=0), axes=(0, 0)) / np.sum(te * te)
    with np.errstate(divide="ignore"):
        t2 = np.where(slope < 0, -1.0 / np.minimum(slope, -1e-300), 2000.0)
    return np.clip(t2, 10.0, 2000.0)


def t2_rmse(stack):
    return float(np.sqrt(np.mean((loglin_t2(stack) - phantom()[1]) ** 2)))


@functools.lru_cache(maxsize=None)
def benefit_tables():
    """``(none, {c: per-echo RMSE}, {c: joint RMSE})`` over PH_WEIGHTS, on the float32 statement."""
    noisy, _ = phantom()
    per, joint = {}, {}
    for c in PH_WEIGHTS:
        w = c * PH_SIGMA
        per[c] = t2_rmse(np.stack([_tv.tv_problem(f, w, 0.0, PH_ITERS, np.float32)[0] for f in noisy]))
        joint[c] = t2_rmse(_tv.tv_joint_problem(noisy, w, 0.0, PH_ITERS, np.float32)[0])
    return t2_rmse(noisy), per, joint
