"""The reference's objectives with every not-correctly-rounded library function moved by at most one ulp.
TEST INFRASTRUCTURE ONLY (same rule as the rest of oracle/: tests/, smoke() and tools that check parity).

Why: the reference differentiates its objective by forward differences with an absolute step of 1e-8 (scipy's
`eps`), which amplifies rounding noise in the objective by 1e8, and it stops on loose tests (ftol = gtol = 1e-2
for the 3-parameter models; run_t2mapping.py:38-106).  Its result for a voxel therefore depends on the last bit
of every exp() / log() / i0e(): another libm, another SIMD width or another scipy build moves a fraction of the
voxels by many milliseconds (SURVEY.md F5 measured scipy 1.7.1 against 1.15.3).  Repeating the reference's fit
with those results jittered by -1, 0 or +1 ulp at random measures how well the reference agrees with ITSELF --
the best any implementation that is not bit-identical to the reference's binary stack can do -- and tells the
voxels whose answer does not depend on that last bit (the stable set) from the ones where it does.
sqrt and the arithmetic operations are correctly rounded everywhere and are not touched.
"""
import numpy as np
from scipy.special import i0e

EPS = np.finfo(float).eps


def perturbed_objectives(rng, numpy_legacy=False, y_row=None, f32_log_ulp=False):
    """{mode: objective(p, te, y)}: run_t2mapping.py:141-177 with exp, log and i0e jittered by one ulp (rng).
    ``numpy_legacy`` (with ``y_row``, the float32 samples of the one voxel this objective will be used for): the rician
    objective as numpy < 2 evaluates it -- ``np.log(signal) - np.log(sigma**2)`` in float32 (oracle._obj_rician_legacy) --
    with the float32 ``np.log(signal)`` moved by at most one float32 ulp ONCE for the voxel (another libm gives another,
    but always the same, value) and the float64 functions jittered per call as before.
    ``f32_log_ulp`` (default stack, with ``y_row``): ``np.log(signal)`` of the float32 samples is a FLOAT32 function under
    numpy >= 2 as well (only the subtraction is float64), so one ulp of it is a float32 ulp: move it so, once for the voxel,
    instead of by a float64 ulp per call.  It shifts the rician objective by a constant (no trajectory changes), which is
    what an implementation with another float32 log shows in `fun`; tests/golden/make_param_floor.py measures with it,
    make_noise_floor.py (T2, nit: the stable sets) did not need it and stays as it was."""
    def jitter(v):
        return v * (1 + EPS * rng.integers(-1, 2, size=np.shape(v)))

    def pexp(z):
        return jitter(np.exp(z))

    def gauss(p, te, y):
        k, t2 = p
        r = y - k * pexp(-te / t2)
        return np.sum(r ** 2) / len(y)

    def gauss_rician(p, te, y):
        k, t2, s = p
        r = y - (k ** 2 * pexp(-2 * te / t2) + s ** 2) ** (1 / 2)
        return np.sum(r ** 2) / len(y)

    def rician(p, te, y):
        k, t2, s = p
        m = k * pexp(-te / t2)
        x = (m * y) / (s ** 2)
        return -np.sum((jitter(np.log(y)) - jitter(np.log(s ** 2))) - (y ** 2 + m ** 2) / (2 * s ** 2)
                       + (np.abs(x) + jitter(np.log(jitter(i0e(x))))))

    if numpy_legacy or f32_log_ulp:
        with np.errstate(all="ignore"):
            ly = np.log(np.asarray(y_row, np.float32)).astype(np.float32)
        step = rng.integers(-1, 2, size=ly.shape)
        ly = np.where(step > 0, np.nextafter(ly, np.float32(np.inf)), np.where(step < 0, np.nextafter(ly, np.float32(-np.inf)), ly)).astype(np.float32)

    if f32_log_ulp and not numpy_legacy:
        def rician_f32_log(p, te, y):
            k, t2, s = p
            m = k * pexp(-te / t2)
            x = (m * y) / (s ** 2)
            return -np.sum((ly.astype(np.float64) - jitter(np.log(s ** 2))) - (y ** 2 + m ** 2) / (2 * s ** 2)
                           + (np.abs(x) + jitter(np.log(jitter(i0e(x))))))

        return {"gaussian": gauss, "gaussian_rician": gauss_rician, "rician": rician_f32_log}

    if numpy_legacy:

        def rician_legacy(p, te, y):
            k, t2, s = p
            m = k * pexp(-te / t2)
            x = (m * y) / (s ** 2)
            a = ly - np.float32(jitter(np.log(s ** 2)))  # float32 array - float32 scalar: float32 under either numpy
            return -np.sum(a - (y ** 2 + m ** 2) / (2 * s ** 2) + (np.abs(x) + jitter(np.log(jitter(i0e(x))))))

        return {"gaussian": gauss, "gaussian_rician": gauss_rician, "rician": rician_legacy}
    return {"gaussian": gauss, "gaussian_rician": gauss_rician, "rician": rician}


def perturbed_fit_rows(args):
    """Pool worker: the reference's fit (same table, bounds, options as oracle.fit_voxel) of rows ``idx`` of ``rows``
    with the jittered objective.  ``args = (idx, fit, low_field, prior, te, rows, seed)`` -> list of (x, nit, success)."""
    from scipy.optimize import minimize

    from . import t2fit_oracle as O

    idx, fit, low_field, prior, te, rows, seed = args[:7]
    legacy = len(args) > 7 and bool(args[7])
    rng = np.random.default_rng(seed)
    fun = None if legacy else perturbed_objectives(rng)[fit]
    out = []
    for v in idx:
        fp = O.fit_table(fit, low_field)
        lb, ub = O.voxel_bounds(fp, rows[v, 0], prior)
        if legacy:
            fun = perturbed_objectives(rng, True, rows[v])[fit]
        with np.errstate(all="ignore"):
            r = minimize(fun, fp["initial_guess"], args=(te, np.array(rows[v])), method="L-BFGS-B",
                         bounds=list(zip(lb, ub)), options=fp["options"], jac=False)
        out.append((r.x, r.nit, r.success))
    return out


def reference_fit_rows(args):
    """Pool worker: the unperturbed reference-equivalent fit (oracle.fit_voxel) of rows ``idx``.
    ``args = (idx, fit, low_field, prior, te, rows[, numpy_legacy])`` -> list of (x, nit, success)."""
    from . import t2fit_oracle as O

    idx, fit, low_field, prior, te, rows = args[:6]
    legacy = len(args) > 6 and bool(args[6])
    fp = O.fit_table(fit, low_field)
    out = []
    for v in idx:
        with np.errstate(all="ignore"):
            x, ok, nit, f, _ = O.fit_voxel(int(v), fit, fp, te, rows, prior, False, want_trace=False, numpy_legacy=legacy)
        out.append((x, nit, ok))
    return out


# ---- deviation statistics shared by tests/golden/make_param_floor.py (the yardstick) and by every test that is held to it ----
YARDSTICK_MARGIN = 1.2      # an implementation may exceed the reference's own statistic by this factor (as the T2 quantiles at scale)
YARDSTICK_FLOOR = 4 * EPS   # and by a few float64 ulps of relative deviation: bit-identical results against a zero statistic pass


def rel_deviation(a, ref):
    """|a - ref| / |ref|, elementwise in float64 (k and sigma are bounded away from zero by every fit table)."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    with np.errstate(all="ignore"):
        return np.abs(a - ref) / np.abs(ref)


F_STOP_FLOOR = (1e-2 / 2) ** 2  # see fun_floor


def fun_floor(y):
    """Denominator floor of the objective statistic: max(1e-12 * mean(y^2), (gtol / 2)^2 = 2.5e-5).
    The least-squares objectives are mean squared residuals, so on a noise-free row they end near 1e-13 .. 1e-7, where
    a relative deviation measures nothing the reference defines:
      * 1e-12 of the row's signal power is the level rounding of the float32 samples and float64 sums reaches, far
        below any objective of a noisy row;
      * the 3-parameter tables stop once the projected gradient is below gtol = 1e-2, and d f / d p =
        2 mean(r d m / d p) with |d m / d k|, |d m / d sigma| <= 1, so EVERY point with an rms residual below gtol / 2
        satisfies the reference's stop rule: objective values below (gtol / 2)^2 are all equally "converged" to it.
        On the constant edge row (flat_100: f = (sigma - 100)^2) the reference's own perturbed runs spread over
        9e-11 .. 3.3e-8, three times the first floor; no implementation can be held to a number inside that spread.
    One formula for all models and both field strengths; it depends on the row alone (the second term is a constant
    of the reference's tables).  rician: |f_ref| >= 6.5 on every stable row, so the floor is inert there."""
    y = np.asarray(y, np.float64)
    return np.maximum(1e-12 * np.mean(y * y, axis=-1), F_STOP_FLOOR)


def fun_deviation(f, f_ref, y):
    """|f - f_ref| / max(|f_ref|, fun_floor(row)): THE objective statistic (final `fun` and per-iteration `f_val`), one
    formula for all models (rician: |f_ref| >= 6.5 on every stable row, the floor is inert there).  ``y``: the row(s)
    the objective belongs to; ``f`` / ``f_ref`` may carry extra trailing axes (iterations)."""
    f, f_ref = np.asarray(f, np.float64), np.asarray(f_ref, np.float64)
    floor = np.asarray(fun_floor(y))
    floor = floor.reshape(floor.shape + (1,) * (f_ref.ndim - floor.ndim))
    with np.errstate(all="ignore"):
        return np.abs(f - f_ref) / np.maximum(np.abs(f_ref), floor)


def res_ulp_bound(y, k):
    """Per-row bound of the residual map evaluated on IDENTICAL parameters by two implementations of the default
    (float64-prediction) form: one float32 ulp of max(max|y|, |k|).  Each prediction is a float64 value rounded to
    float32, so it lands at most one float32 ulp away when exp() rounds differently, and the mean of n such errors is at
    most one of them."""
    y = np.asarray(y, np.float32)
    with np.errstate(all="ignore"):
        big = np.fmax(np.nanmax(np.abs(y), axis=-1), np.abs(np.asarray(k, np.float32)))
    return np.spacing(big.astype(np.float32))


def deviation_stats(v, qs=(50, 99, 100)):
    """(median, 99th percentile, maximum) -- or the percentiles ``qs`` -- of the finite entries of ``v``."""
    v = np.asarray(v, np.float64).reshape(-1)
    v = v[np.isfinite(v)]
    return tuple(float(np.percentile(v, q)) for q in qs)


def exceeds_yardstick(got, yard, qs=(50, 99, 100)):
    """Compare the statistics of an implementation's deviations ``got`` with those of the reference's own ``yard``
    (pooled over rows and seeds).  Returns the list of (percentile, got, allowed) that exceed
    YARDSTICK_MARGIN x yardstick + YARDSTICK_FLOOR: empty when the implementation is inside the reference's spread."""
    g, y = deviation_stats(got, qs), deviation_stats(yard, qs)
    return [(q, a, YARDSTICK_MARGIN * b + YARDSTICK_FLOOR) for q, a, b in zip(qs, g, y)
            if not a <= YARDSTICK_MARGIN * b + YARDSTICK_FLOOR]


def trace_deviation(got_f, got_s, want_f, want_s, y):
    """Per-iteration deviation of a trace from the golden one over their common length: (fun_deviation of f_val,
    relative deviation of the step length from the second iteration on -- the first has none; NaN where the golden step
    is exactly 0 (one iteration of the 524 on the stable traced rows: scipy kept the iterate), where no relative
    deviation exists)."""
    n = min(len(got_f), len(want_f))
    df = fun_deviation(np.asarray(got_f[:n], np.float64), np.asarray(want_f[:n], np.float64), y)
    want = np.asarray(want_s[1:n], np.float64)
    ds = rel_deviation(np.asarray(got_s[1:n], np.float64), want)
    return df, np.where(want > 0, ds, np.nan)


def perturbed_traced_fit(fun, fit, low_field, prior, te, row):
    """The reference's fit of one row (same table, bounds, options as oracle.fit_voxel) with objective ``fun`` (one of
    perturbed_objectives) and its callback (run_t2mapping.py:180-234): f at xk, ||xk - x_prev||.
    -> (x, nit, success, fun, trace_f, trace_step)."""
    from scipy.optimize import minimize

    from . import t2fit_oracle as O

    fp = O.fit_table(fit, low_field)
    lb, ub = O.voxel_bounds(fp, row[0], prior)
    y = np.array(row)
    tf, ts, prev = [], [], [None]

    def cb(xk):
        ts.append(np.nan if prev[0] is None else np.linalg.norm(xk - prev[0]))
        prev[0] = np.array(xk)
        tf.append(fun(xk, te, y))

    with np.errstate(all="ignore"):
        r = minimize(fun, fp["initial_guess"], args=(te, y), method="L-BFGS-B", bounds=list(zip(lb, ub)),
                     options=fp["options"], jac=False, callback=cb)
    return r.x, r.nit, r.success, r.fun, np.array(tf), np.array(ts)
