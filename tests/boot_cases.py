"""Crafted inputs of the parametric bootstrap whose drop-outs are known without a device (tests/test_bootstrap_host.py
checks the layout, tests/test_bootstrap_edges_gpu.py runs it).  Pure numpy: nothing here loads the library.

The refit is the closed-form ``loglin`` solver with two echoes and ``noise="gaussian"``.  By csrc/t2fit_loglin.h a replica
counts exactly when both of its samples are > 0 and finite (with two positive samples sxx > 0 always holds, and slope and intercept
are finite), and the samples are ``S + s n1`` of :func:`fetal_t2mapping_amd._philox.replica`: the number of counted
replicas of a voxel is known in float64.  The table's k bounds are widened to (1e-3, 1e5) so that k refits are distinct
values; T2 keeps (10, 600), so that rising replicas tie at 600 and steep ones at 10."""
import numpy as np

from fetal_t2mapping_amd import _philox

SHAPE = (3, 7, 31)  # 651 voxels: no multiple of 4 (the four-voxel synthesis), of 64 (finalisation) or of 256 (accumulation)
N = int(np.prod(SHAPE))
TE = [114.0, 299.0]
R = 16
SEED = 1234
T2_BOUNDS = (10.0, 600.0)
K_BOUNDS = (1e-3, 1e5)
NEAR = 1e-4  # a sample within NEAR * s of zero may fall on the other side in float32: its voxel is left out of the count equality
# the fit table as fit_table("gaussian", True) returns it, with the k bounds widened (index 0 = k, 1 = T2)
TABLE = {"initial_guess": [650, 165], "param_bounds": [K_BOUNDS, T2_BOUNDS], "solver": "L-BFGS-B",
         "options": {"ftol": 1e-6, "maxls": 50, "disp": False}}

# classes by flat index modulo 8: (name, T2, k, s).  With k = 0 the samples are noise whatever T2 is, so the T2 centre of
# that class is free: 17.503 is a value about which the shifted float64 sums of n = 3, 5..9 equal refits of 600 round to
# a small positive variance (:func:`shifted_variance_of_equal`) -- the case the min / max of the kernel exist for.
CYCLE = (("k0", 17.503, 0.0, 20.0),        # noise alone: a quarter of the replicas count; the centres are far from every refit
         ("k20", 151.3, 20.0, 20.0),
         ("k60", 151.3, 60.0, 20.0),
         ("k10_t40", 40.7, 10.0, 20.0),
         ("k200", 151.3, 200.0, 20.0),    # the intermediate class: counts 13..16
         ("k2000", 151.3, 2000.0, 20.0),  # always counts
         ("k1500_s0", 151.3, 1500.7, 0.0),  # every replica identical
         ("k60", 151.3, 60.0, 20.0))
INF, NAN = float("inf"), float("nan")
# classes at fixed flat indices, written over the cycle: name -> (indices, T2, k, s)
SPECIAL = {
    "zero_s0": ((9, 100, 333), 150.0, 0.0, 0.0),          # all samples 0: never counts
    "t2_nan": ((17, 201, 402), NAN, 1000.0, 20.0),        # never count
    "k_nan": ((26, 211, 500), 150.0, NAN, 20.0),
    "k_inf": ((35, 222, 600), 150.0, INF, 20.0),
    "t2_inf_k60": ((44, 45, 130, 260, 390, 520, 640), INF, 60.0, 20.0),  # S = k at both echoes; refits finite, centre not
    "t2_inf_k2000": ((46, 131, 261), INF, 2000.0, 20.0),  # every refit above 600: all tie at the bound
    "t2_zero": ((53, 140, 270, 400), 0.0, 2000.0, 20.0),  # S = 0
    # a decay steeper than the lower bound with noise far below the second sample: every replica counts, every T2
    # refit ties at 10, the k refits differ
    "steep": (tuple(range(60, N, 50)), 8.1, 2000.0, 1e-14),
}


def maps():
    """(t2, k, noise map, class names) of the case, float32 arrays of SHAPE and an object array of names."""
    t2 = np.empty(N, np.float32)
    k = np.empty(N, np.float32)
    s = np.empty(N, np.float32)
    names = np.empty(N, object)
    for i in range(N):
        names[i], t2[i], k[i], s[i] = CYCLE[i % len(CYCLE)]
    for name, (where, t2v, kv, sv) in SPECIAL.items():
        for i in where:
            names[i], t2[i], k[i], s[i] = name, t2v, kv, sv
    return t2.reshape(SHAPE), k.reshape(SHAPE), s.reshape(SHAPE), names.reshape(SHAPE)


def predict(n_replicas=R, seed=SEED, voxels=slice(None)):
    """The statement of the case in float64, flat over the voxels: samples ``y`` (R, 2, n), ``counted`` (R, n) = both
    samples > 0 and finite, ``near`` (n,) = some sample within NEAR * s of zero, and the T2 the closed form gives a counted replica
    (two points: the line through them whatever the weights), clipped into T2_BOUNDS, NaN where not counted."""
    t2, k, s, _ = (a.reshape(-1) for a in maps())
    y = np.stack([_philox.replica(t2, k, TE, s, None, seed=seed, replica=r, noise="gaussian") for r in range(n_replicas)])
    y = y[:, :, voxels]
    s64 = s.astype(np.float64)[voxels]
    with np.errstate(invalid="ignore", divide="ignore"):
        # (k = +inf gives samples of +inf: positive, but their logarithms leave nothing finite to regress on)
        counted = (y[:, 0] > 0.0) & (y[:, 1] > 0.0) & np.isfinite(y[:, 0]) & np.isfinite(y[:, 1])
        near = np.any(np.abs(y) < NEAR * s64, axis=(0, 1))
        slope = (np.log(y[:, 1]) - np.log(y[:, 0])) / (TE[1] - TE[0])
        t2_fit = np.where(slope < 0.0, -1.0 / slope, np.inf)
    t2_fit = np.where(counted, np.clip(t2_fit, *T2_BOUNDS), np.nan)
    return y, counted, near, t2_fit


TABLE_OPEN_T2 = dict(TABLE, param_bounds=[K_BOUNDS, (T2_BOUNDS[0], float("inf"))])


def predict_open_t2(n_replicas=R, seed=SEED):
    """The same case with no upper T2 bound (TABLE_OPEN_T2): a flat or rising replica converges to T2 = +inf, which
    nothing clips, so it is a converged refit that is not finite and must not count.  Returns ``counted`` (R, n) = both
    samples > 0, finite and falling, and ``near`` (n,): as in :func:`predict`, or two samples of a replica so close that
    float32 samples and float32 logarithms may order them the other way (1e-5 of their size: the logarithm of the
    solver is good to about 1 ulp, 1e-7 of a value up to 16; NEAR * s for the samples themselves)."""
    y, counted, near, _ = predict(n_replicas, seed)
    s = maps()[2].reshape(-1).astype(np.float64)
    with np.errstate(invalid="ignore"):
        falling = y[:, 1] < y[:, 0]
        close = np.abs(y[:, 1] - y[:, 0]) < 1e-5 * (np.abs(y[:, 0]) + np.abs(y[:, 1])) + NEAR * s
    return counted & falling, near | np.any(counted & close & (s > 0.0), axis=0)


def shifted_variance_of_equal(x, centre, n):
    """(sum d^2 - (sum d)^2 / n) / (n - 1) of n equal values x with d = x - centre, accumulated in float64 in order, as
    boot_accum_kernel / boot_final_kernel do it: 0 in exact arithmetic, whatever the rounding leaves otherwise."""
    d = float(x) - float(centre)
    s = ss = 0.0
    for _ in range(n):
        s += d
        ss += d * d
    return (ss - s * (s / n)) / (n - 1)


def masks_with(counts=(0, 1, 63, 64, 65, 255, 256, 257)):
    """One uint8 mask of SHAPE per count, with exactly that many voxels set; voxel 0 and the last voxel are set in some
    and clear in others (the empty mask apart, alternately: both, first only, last only, neither)."""
    rng = np.random.default_rng(77)
    out = []
    for j, c in enumerate(counts):
        m = np.zeros(N, np.uint8)
        ends = [e for e, on in ((0, j % 4 in (1, 2)), (N - 1, j % 4 in (1, 3))) if on][:c]
        m[ends] = 1
        inner = rng.permutation(np.arange(1, N - 1))[: c - len(ends)]
        m[inner] = 1
        assert int(m.sum()) == c
        out.append(m.reshape(SHAPE))
    return out
