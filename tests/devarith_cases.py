"""Operand populations and error measures shared by the tests of the lane arithmetic: the `_seq` forms on the CPU from a
coarse seed (test_lane_solver_hostsim.py) and the device entry points on the GPU (test_device_arithmetic_gpu.py)."""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_echo_times():
    """Every echo time (ms) that occurs in an echo-time set of the golden voxel fixtures."""
    te = set()
    for path in sorted(glob.glob(os.path.join(GOLDEN, "voxels_*.npz"))):
        te.update(float(t) for t in np.load(path)["te"])
    return np.array(sorted(te))


def ordered(x):
    """float64 -> int64 that counts representable numbers (adjacent floats differ by 1, -0.0 and +0.0 coincide)."""
    i = np.ascontiguousarray(x, np.float64).view(np.int64)
    return np.where(i >= 0, i, np.iinfo(np.int64).min - i)


def ulp_distance(a, b):
    """How many representable float64 numbers apart, exactly (int64; a NaN counts as infinitely far).  Numbers of
    opposite sign more than 2^63 steps apart would wrap: clamped through a float64 estimate of the distance."""
    oa, ob = ordered(a), ordered(b)
    d = np.abs(oa - ob).astype(np.float64)
    rough = np.abs(oa.astype(np.float64) - ob.astype(np.float64))
    d = np.where(rough > 2.0 ** 62, rough, d)
    return np.where(np.isnan(a) | np.isnan(b), np.inf, d)


def ordered32(x):
    i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i >= 0, i, -(2 ** 31) - i)


def fit_exp_arguments(n):
    """(a, b) with a / b the exp() arguments the fit forms: (-TE, T2) and (-2 TE, T2) for every golden echo time and T2 on
    a dense grid over [10, 2000] ms; n operand pairs in all (rounded down to whole grids)."""
    te = golden_echo_times()
    m = max(2, n // (2 * len(te)))
    t2 = np.linspace(10.0, 2000.0, m)
    a = np.concatenate([np.repeat(-te, m), np.repeat(-2.0 * te, m)])
    b = np.tile(t2, 2 * len(te))
    return a, b


def division_populations(n, seed=21):
    """The four operand populations of the quotient tests, about n pairs each: name -> (a, b)."""
    rng = np.random.default_rng(seed)
    pops = {"fit_exp_arguments": fit_exp_arguments(n)}
    x = 10.0 ** rng.uniform(np.log10(8.0), 7.0, n)
    x = np.where(x <= 8.0, np.nextafter(8.0, 9.0), x)
    pops["i0e_32_over_x"] = (np.full(n, 32.0), x)
    f = rng.uniform(np.sqrt(0.5) - 1.0, np.sqrt(2.0) - 1.0, n)
    half_root2 = float.fromhex("0x1.6a09e667f3bcdp-1")  # the mantissa threshold of t2_log_lean: the two ends as it forms them
    f[:2] = [half_root2 - 1.0, 2 * np.nextafter(half_root2, 0) - 1.0]
    pops["log_lean_f_over_2_plus_f"] = (f, 2.0 + f)
    sign = lambda: np.where(rng.random(n) < 0.5, -1.0, 1.0)
    a = sign() * rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-300, 301, n)
    b = sign() * rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-300, 301, n)
    pops["random_exponents_pm300"] = (a, b)
    return pops


def quotient_figures(got, a, b):
    """(largest distance from numpy's IEEE a / b in ulps, share of quotients that are not the correctly rounded one)."""
    with np.errstate(all="ignore"):
        want = a / b
    d = ulp_distance(got, want)
    return float(d.max()), float(np.mean(d != 0))


def mp_ulp_error(got, exact_fn, x, dps=40):
    """Largest |got - exact| in ulps of the correctly rounded result, exact_fn(mpf) evaluated with `dps` digits."""
    import mpmath

    worst = 0.0
    with mpmath.workdps(dps):
        for xi, gi in zip(np.asarray(x, np.float64).ravel(), np.asarray(got, np.float64).ravel()):
            exact = exact_fn(mpmath.mpf(float(xi)))
            ulp = float(np.spacing(abs(float(exact))))
            worst = max(worst, float(abs(mpmath.mpf(float(gi)) - exact) / ulp))
    return worst
