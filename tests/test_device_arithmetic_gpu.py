"""The lane arithmetic that exists only in the device build -- the side of every `#if defined(__HIP_DEVICE_COMPILE__)` of
t2fit_lane.h / t2fit_lbfgsb.h that the host simulator (tests/hostsim) never compiles -- run on the GPU through the device
probe (tests/devprobe), one sequence at a time, against correctly rounded or 40-digit references:

  a. t2_sqrt_core and the shared-seed roots (hardware v_rsq_f64 seed)   bit for bit numpy's IEEE sqrt
  b. t2_exp_core                                                        bit for bit the device library's exp; <= 1 ulp
  c. t2_fdiv, t2_div_by_rcp                                             <= 1 ulp; last-bit share pinned; special operands
  d. t2_fast_rcp, t2_fast_rsqrt                                         largest error pinned
  e. t2_log_lean with the frexp builtins                                < 1 ulp; the host's bits where the quotient is exact
  f. the float32 intrinsics of the LM path                              error bounds
  g. the wave paths of t2_log_i0e4 (T2_WAVE_ANY = __ballot)             one answer whatever the neighbours
  h. one Lbfgsb::eval                                                   one answer whatever the neighbours; the oracle's f

The measured figures (`pytest tests/test_device_arithmetic_gpu.py -m gpu -s` prints each one before it is asserted) are
recorded in DESIGN.md section 5d."""
import numpy as np
import pytest

import devarith_cases as dc

pytestmark = pytest.mark.gpu

# ---- pins: measured on an MI355X with this file's operands, then bounded as the docstrings say ----
# c. share of quotients that are not the correctly rounded one: 4 x the measured share (0 where none was found)
# measured: 0 of a million on each of the four populations, for t2_fdiv and for t2_div_by_rcp
FDIV_LAST_BIT_SHARE_MAX = {"fit_exp_arguments": 0.0, "i0e_32_over_x": 0.0, "log_lean_f_over_2_plus_f": 0.0,
                           "random_exponents_pm300": 0.0}
# d. largest error in ulps, the measured value rounded up to the next half ulp (never above 2)
FAST_RCP_MAX_ULP = 0.5    # measured 0.5000: every reciprocal of the million is the correctly rounded one
FAST_RSQRT_MAX_ULP = 1.0  # measured 0.9877
# f. largest error of the float32 intrinsics in float32 ulps of the exact result: 2 x the measured value
F32_MAX_ULP = {"log": 2 * 1.8795, "rsqrt": 2 * 0.8549, "rcp": 2 * 0.5}
# h. |f - f_oracle| / |f_oracle| of the HOST simulator against the oracle's objective in np.longdouble on the rows of
# eval_cases(), measured on the CPU (python tests/test_device_arithmetic_gpu.py --host-distance); the device gets 4 x
HOST_F_DISTANCE = {"gaussian": 1.33e-15, "gaussian_rician": 1.05e-15, "rician": 2.21e-8}


@pytest.fixture(scope="module")
def probe():
    from devprobe import probe as p

    p.build()
    assert p.device_count() > 0, "no HIP device"
    return p


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---- a. square roots ----------------------------------------------------------------------------------------------
def _root_operands():
    """Base radicands x and, for each, three nearby a: the populations of
    test_lane_solver_hostsim.py::test_shared_seed_square_roots_are_the_correctly_rounded_ones."""
    rng = np.random.default_rng(5)
    n = 100_000
    x = 10.0 ** rng.uniform(-2, 10, n)
    third = n // 3
    rel = np.concatenate([rng.uniform(-1, 1, (third, 3)) * 1e-8,                      # the reference's own step
                          rng.uniform(-1, 1, (third, 3)) * 2.0 ** -22,
                          np.tile([[2.0 ** -22, -(2.0 ** -22), 2.0 ** -22]], (n - 2 * third, 1))])  # the precondition's edge
    rel[2 * third::2] *= -1.0                                                          # ... on opposite sides, either order
    a = x[:, None] * (1.0 + rel)
    sq = np.floor(rng.uniform(1, 3e4, 2000)) ** 2
    x = np.concatenate([x, sq])
    a = np.concatenate([a, np.stack([np.nextafter(sq, 0), sq, np.nextafter(sq, np.inf)], axis=1)])
    return x, a


def test_sqrt_core_is_the_correctly_rounded_root(probe):
    """t2_sqrt_core / t2_sqrt_core_h from the hardware's v_rsq_f64 seed == numpy's IEEE sqrt, bit for bit (and so is the
    device library's sqrt): radicands' range, exact squares and their neighbours; 0.0 gives +0.0.  h = 1 / (2 sqrt(x)) comes
    out of ONE coupled Newton step on the seed: from a seed good to 2^-23 (the quality the CPU tests prove the sequences
    with) its error is 1.5 (2^-23)^2 = 2^-45.4, so 2^-45 is asserted; the largest error found is printed."""
    x, a = _root_operands()
    x = np.concatenate([x, a.ravel(), [0.0]])
    want = np.sqrt(x)
    got = probe.unary("sqrt_core", x)
    assert _same_bits(got, want)
    assert got[-1] == 0.0 and not np.signbit(got[-1])
    assert _same_bits(probe.unary("sqrt_lib", x), want)
    pos = x[:-1]
    root, h = probe.unary("sqrt_core_h", pos)
    assert _same_bits(root, np.sqrt(pos))
    h_want = 0.5 / np.sqrt(pos.astype(np.longdouble))
    h_err = float(np.max(np.abs((h - h_want) / h_want)))
    print(f"sqrt_core_h: h = 1 / (2 sqrt(x)) to 2^{np.log2(h_err):.2f}")
    assert h_err <= 2.0 ** -45


def test_shared_seed_roots_are_the_correctly_rounded_ones(probe):
    """t2_sqrt_near, and t2_sqrt_from_h on t2_rsqrt_half_near, from the h of t2_sqrt_core_h(x) (hardware seed): bit for bit
    numpy's sqrt(a) for a within 1e-8 of x, within 2^-22, exactly at +-2^-22 with the displaced arguments on opposite sides,
    and for the neighbours of exact squares.  h' = t2_rsqrt_half_near(a, h) is one Newton step from an h that is 2^-23 off
    (the displacement) or 2^-45 off (its own error): 1.5 (2^-23)^2 = 2^-45.4 again, 2^-45 asserted."""
    x, a = _root_operands()
    near, half, from_h = probe.sqrt_near(np.repeat(x, 3), a.ravel())
    want = np.sqrt(a.ravel())
    assert _same_bits(near, want)
    assert _same_bits(from_h, want)
    h_want = 0.5 / np.sqrt(a.ravel().astype(np.longdouble))
    h_err = float(np.max(np.abs((half - h_want) / h_want)))
    print(f"rsqrt_half_near: h' = 1 / (2 sqrt(a)) to 2^{np.log2(h_err):.2f}")
    assert h_err <= 2.0 ** -45


def test_sqrt_core_below_the_library_rescaling(probe):
    """Below 2^-767 the library's sqrt rescales and t2_sqrt_core does not.  Such radicands are reachable (a sigma bound of
    0, k^2 exp(-2 TE / T2) with 2 TE / T2 in (532, 745)).  The result must be finite, non-negative and at most
    2^-383 (1 + 2^-20): far below half an ulp of any non-zero float32 sample, it cannot move a residual.  The largest
    distance from the correctly rounded root is printed, not bounded."""
    rng = np.random.default_rng(8)
    k2 = rng.uniform(550.0, 3e4, 200_000) ** 2
    with np.errstate(under="ignore"):
        x = np.concatenate([k2 * np.exp(-rng.uniform(532.0, 745.0, len(k2))), 2.0 ** rng.uniform(-1074, -767, 100_000),
                            [5e-324, 2.0 ** -1022, np.nextafter(2.0 ** -1022, 0), np.nextafter(2.0 ** -767, 0)]])
    x = x[(x > 0) & (x < 2.0 ** -767)]
    assert np.sum(x < 2.0 ** -1022) > 1000  # denormals included
    got = probe.unary("sqrt_core", x)
    d = dc.ulp_distance(got, np.sqrt(x))
    normal = x >= 2.0 ** -1022
    print(f"sqrt_core_below_2^-767: n {len(x)} max_ulp_distance normal {d[normal].max():.0f} denormal {d[~normal].max():.3g} "
          f"largest result {got.max():.3e}")
    assert np.all(np.isfinite(got)) and np.all(got >= 0.0)
    assert got.max() <= 2.0 ** -383 * (1 + 2.0 ** -20)


# ---- b. exp ---------------------------------------------------------------------------------------------------------
def _exp_arguments():
    rng = np.random.default_rng(9)
    a, b = dc.fit_exp_arguments(300_000)
    return {"dense": -rng.uniform(0, 750, 400_000), "denormal_band": -rng.uniform(708.3, 745.2, 100_000),
            "underflow": -rng.uniform(745.2, 1000, 20_000), "log_grid": -(10.0 ** rng.uniform(3, 9, 50_000)),
            "limits": np.array([-1e9, -1.4e9, 0.0, -0.0]), "fit_arguments": a / b}


def test_exp_core_is_the_device_librarys_exp(probe):
    """t2_exp_core == the device library's exp, bit for bit, on every argument the fit can form: dense over [-750, 0], the
    denormal-result band, underflow to +0, down to -1e9 (the config_check limit) and -1.4e9, +-0 -> exactly 1, and the
    -TE / T2, -2 TE / T2 of the golden echo-time sets over T2 in [10, 2000] ms."""
    args = _exp_arguments()
    x = np.concatenate(list(args.values()))
    assert len(x) <= 1_000_000
    core, lib = probe.unary("exp_core", x), probe.unary("exp_lib", x)
    assert _same_bits(core, lib)
    part = dict(zip(args, np.split(core, np.cumsum([len(v) for v in args.values()])[:-1])))
    lim = part["limits"]
    assert lim[0] == 0.0 and lim[1] == 0.0 and not np.signbit(lim[0]) and lim[2] == 1.0 and lim[3] == 1.0
    for k in ("underflow", "log_grid"):
        assert np.all(part[k][args[k] < -745.14] == 0.0) and not np.any(np.signbit(part[k])), k
    band = part["denormal_band"]
    assert np.all(band < 2.0 ** -1021) and np.mean((band > 0) & (band < 2.0 ** -1022)) > 0.9  # denormal results delivered


def test_exp_core_is_within_one_ulp(probe):
    """Against a 40-digit exponential both t2_exp_core and the library's exp stay within 1 ulp wherever the result is
    normal (the device library documents 1 ulp), and within one denormal step below."""
    import mpmath

    args = _exp_arguments()
    rng = np.random.default_rng(10)
    x = np.concatenate([rng.choice(args["dense"], 12_000), rng.choice(args["fit_arguments"], 6_000),
                        rng.choice(args["denormal_band"], 2_000), [0.0, -708.39, -1e-300, -1e-17]])
    for op in ("exp_core", "exp_lib"):
        got = probe.unary(op, x)
        normal = got >= 2.0 ** -1022
        worst = dc.mp_ulp_error(got[normal], mpmath.exp, x[normal])
        with mpmath.workdps(40):
            sub = max(float(abs(mpmath.mpf(float(g)) - mpmath.exp(mpmath.mpf(float(v)))) / mpmath.mpf(2) ** -1074)
                      for g, v in zip(got[~normal], x[~normal]))
        print(f"{op}: largest error {worst:.4f} ulp on {int(normal.sum())} normal results, {sub:.4f} denormal steps below")
        assert worst <= 1.0 and sub <= 1.0


# ---- c. divisions ---------------------------------------------------------------------------------------------------
_POPS = {}


def _population(name):
    if not _POPS:
        _POPS.update(dc.division_populations(1_000_000))
    return _POPS[name]


@pytest.mark.parametrize("name", list(FDIV_LAST_BIT_SHARE_MAX))
def test_divisions_are_within_one_ulp(probe, name):
    """t2_fdiv and t2_div_by_rcp(a, b, t2_rcp_for_div(b)) against numpy's IEEE a / b on a million operand pairs: no
    quotient more than 1 ulp off, the share of last-bit differences at most 4 x the measured one (0 where none was
    found), and the device's own `/` equal to numpy's everywhere."""
    a, b = _population(name)
    assert len(a) <= 1_000_000
    with np.errstate(all="ignore"):
        want = a / b
    assert _same_bits(probe.binary("div_ieee", a, b), want)
    for op in ("fdiv", "div_by_rcp"):
        worst, share = dc.quotient_figures(probe.binary(op, a, b), a, b)
        print(f"{op} {name}: n {len(a)} max_ulp {worst:.0f} last_bit_share {share:.3g}")
        assert worst <= 1.0, (op, name)
        assert share <= FDIV_LAST_BIT_SHARE_MAX[name], (op, name, share)


# what t2_fdiv returns for operands outside "finite, normal, quotient in range" (a, b, class): recorded in the table of
# DESIGN.md section 5d next to what IEEE division returns; "nan", "same" (the IEEE result, sign of a zero included),
# "zero_sign" (a zero of the other sign) or "close" (finite, within 1 ulp or one denormal step of it)
_BIG, _DEN = 2.0 ** 1023, 2.0 ** -1060
FDIV_SPECIAL = [
    (1.5, 0.0, "nan"), (-1.5, 0.0, "nan"), (0.0, 0.0, "nan"), (1.5, -0.0, "nan"),           # IEEE: +-inf, NaN
    (1.5, np.inf, "nan"), (1.5, -np.inf, "nan"), (np.inf, 2.0, "nan"),                     # IEEE: +-0, inf
    (1.5, np.nan, "nan"), (np.nan, 2.0, "nan"),                                            # IEEE: NaN
    (1.5, _DEN, "nan"), (2.0 ** -1040, _DEN, "nan"),                                       # 1 / b overflows; IEEE: inf, 2^20
    (1.5, 2.0 ** -1023, "close"),                                                          # denormal b, 1 / b finite
    (1.5, _BIG, "close"), (2.0 ** 1000, 1.5 * _BIG, "close"),                              # |b| > 2^1022: 1 / b denormal
    (0.0, 3.0, "same"), (0.0, -3.0, "same"), (-0.0, 3.0, "zero_sign"), (-0.0, -3.0, "same"),
    (2.0 ** 1000, 2.0 ** -100, "nan"), (-(2.0 ** 1000), 2.0 ** -100, "nan"),               # quotient overflows; IEEE: +-inf
    (2.0 ** -1000, 2.0 ** 60, "close"), (2.0 ** -1000, 2.0 ** 200, "same"),                # quotient denormal / underflows to 0
]


def test_fdiv_special_operands(probe):
    """What t2_fdiv returns where its operands leave the finite, normal range -- b = 0, +-inf, NaN, denormal, |b| > 2^1022,
    a = 0, quotients that overflow or underflow -- is what DESIGN.md section 5d records (NaN where IEEE division gives an
    infinity or a zero from an infinite operand, +0 where IEEE gives -0 for a = -0, b > 0), and the device's `/` is IEEE's.
    The call-site audit there says why none of these operands reaches a value that is used."""
    a = np.array([c[0] for c in FDIV_SPECIAL])
    b = np.array([c[1] for c in FDIV_SPECIAL])
    with np.errstate(all="ignore"):
        ieee = a / b
    dev = probe.binary("div_ieee", a, b)
    assert np.array_equal(np.isnan(dev), np.isnan(ieee)) and _same_bits(dev[~np.isnan(ieee)], ieee[~np.isnan(ieee)])
    for op in ("fdiv", "div_by_rcp"):
        got = probe.binary(op, a, b)
        for (ai, bi, kind), g, w in zip(FDIV_SPECIAL, got, ieee):
            print(f"{op}({ai!r}, {bi!r}) = {g!r}   IEEE {w!r}   [{kind}]")
        for (ai, bi, kind), g, w in zip(FDIV_SPECIAL, got, ieee):
            if kind == "nan":
                assert np.isnan(g), (op, ai, bi, g)
            elif kind == "same":
                assert g == w and np.signbit(g) == np.signbit(w), (op, ai, bi, g, w)
            elif kind == "zero_sign":
                assert g == 0.0 and w == 0.0 and np.signbit(g) != np.signbit(w), (op, ai, bi, g, w)
            else:
                assert np.isfinite(g) and (dc.ulp_distance(np.array([g]), np.array([w]))[0] <= 1), (op, ai, bi, g, w)


# ---- d. reciprocal and reciprocal root ------------------------------------------------------------------------------
def _largest_ulp_error(got, x, exact_ld, exact_mp, rng, n_random=15_000, n_top=500):
    """Largest |got - exact| / ulp(exact): a 40-digit reference on the n_top candidates an extended-precision pass ranks
    worst, and on n_random others."""
    want = exact_ld(x.astype(np.longdouble))
    rough = np.abs((got.astype(np.longdouble) - want) / np.spacing(np.abs(want.astype(np.float64))).astype(np.longdouble))
    pick = np.union1d(np.argsort(rough)[-n_top:], rng.choice(len(x), n_random, replace=False))
    return dc.mp_ulp_error(got[pick], exact_mp, x[pick])


def test_fast_rcp_largest_error(probe):
    """t2_fast_rcp ("~1 ulp") on 10**U(-300, 300), either sign, and on the magnitudes the matrix rebuild and the 3 x 3 solve
    divide by: the largest error in ulps, against 40 digits, is at most the measured one rounded up to half an ulp."""
    rng = np.random.default_rng(14)
    x = np.concatenate([10.0 ** rng.uniform(-300, 300, 500_000), 10.0 ** rng.uniform(-12, 12, 500_000)])
    x *= np.where(rng.random(len(x)) < 0.5, -1.0, 1.0)
    worst = _largest_ulp_error(probe.unary("fast_rcp", x), x, lambda v: 1 / v, lambda v: 1 / v, rng)
    print(f"fast_rcp: largest error {worst:.7f} ulp")
    assert FAST_RCP_MAX_ULP <= 2.0 and worst <= FAST_RCP_MAX_ULP


def test_fast_rsqrt_largest_error(probe):
    """t2_fast_rsqrt ("~1 ulp") on 10**U(-300, 300) and on the curvatures y's the solver scales a pair by."""
    import mpmath

    rng = np.random.default_rng(15)
    x = np.concatenate([10.0 ** rng.uniform(-300, 300, 500_000), 10.0 ** rng.uniform(-20, 10, 500_000)])
    worst = _largest_ulp_error(probe.unary("fast_rsqrt", x), x, lambda v: 1 / np.sqrt(v), lambda v: 1 / mpmath.sqrt(v), rng)
    print(f"fast_rsqrt: largest error {worst:.4f} ulp")
    assert FAST_RSQRT_MAX_ULP <= 2.0 and worst <= FAST_RSQRT_MAX_ULP


# ---- e. the lean log ------------------------------------------------------------------------------------------------
def test_lean_log_on_the_device(probe):
    """t2_log_lean with the frexp builtins: below 1 ulp against a 40-digit logarithm on the populations of
    test_lane_solver_hostsim.py::test_lean_log_is_within_one_ulp, exactly 0 at 1, and bit for bit the host simulator's
    t2_log_lean wherever the device's f / (2 + f) is the correctly rounded quotient (the only operation that differs)."""
    import mpmath

    from hostsim import sim

    rng = np.random.default_rng(13)
    x = np.concatenate([rng.uniform(0.0, 1.0, 4000), 10.0 ** rng.uniform(-12, 0, 2000), 10.0 ** rng.uniform(0, 12, 500),
                        1.0 + rng.uniform(-1e-3, 1e-3, 1000), np.array([1.0, 0.5, 2.0, 0.7071067811865476, 1e-300, 1e300])])
    x = x[x > 0]
    got = probe.unary("log_lean", x)
    worst = dc.mp_ulp_error(got[got != 0], mpmath.log, x[got != 0])
    print(f"log_lean on the device: largest error {worst:.4f} ulp on {len(x)} arguments")
    assert worst < 1.0
    assert got[x == 1.0][0] == 0.0 and np.all(x[got == 0] == 1.0)
    # the quotient's operands as t2_log_lean forms them
    m, _ = np.frexp(x)
    m = np.where(m < float.fromhex("0x1.6a09e667f3bcdp-1"), m + m, m)
    f = m - 1.0
    exact = _bits(probe.binary("fdiv", f, 2.0 + f)) == _bits(f / (2.0 + f))
    print(f"log_lean: quotient correctly rounded on {int(exact.sum())} of {len(x)}")
    assert exact.mean() > 0.9
    assert _same_bits(got[exact], sim.log_lean(x)[exact])


# ---- f. float32 intrinsics of the LM path ---------------------------------------------------------------------------
def test_f32_exp_error_bound(probe):
    """t2_exp(float) = exp2(x log2 e) in float32 (v_exp_f32) over [-104, 0]: the rounded product carries |x| 2^-24 relative
    into the result and v_exp_f32 adds 1 ulp, so the relative error is at most (|x| + 2) 2^-23 (a factor 2 over that sum)
    wherever the exact value is >= 2^-126; below, 0 <= result <= 2^-126 (denormal results may be flushed)."""
    rng = np.random.default_rng(16)
    x = np.concatenate([-rng.uniform(0, 104, 500_000), [0.0, -0.0, -104.0, -87.3, -87.4, -1e-6]]).astype(np.float32)
    got = probe.unary_f32("exp", x).astype(np.float64)
    exact = np.exp(x.astype(np.float64))
    normal = exact >= 2.0 ** -126
    rel = np.abs(got[normal] - exact[normal]) / exact[normal]
    bound = (np.abs(x[normal].astype(np.float64)) + 2.0) * 2.0 ** -23
    print(f"f32 exp: largest relative error / bound {np.max(rel / bound):.3f}, largest relative error {rel.max():.3e}")
    assert np.all(rel <= bound)
    assert np.all((got[~normal] >= 0.0) & (got[~normal] <= 2.0 ** -126))


@pytest.mark.parametrize("op", list(F32_MAX_ULP))
def test_f32_intrinsic_largest_error(probe, op):
    """__logf / __frsqrt_rn / __frcp_rn on the ranges the LM seed and its normal equations use (samples 1e-2 .. 3e4,
    radicands 1e-2 .. 1e10, pivots 1e-12 .. 1e12): largest error against float64 in float32 ulps of the exact result,
    at most 2 x the measured one."""
    rng = np.random.default_rng(17)
    lo, hi, exact = {"log": (-2, 4.5, np.log), "rsqrt": (-2, 10, lambda v: 1 / np.sqrt(v)), "rcp": (-12, 12, lambda v: 1 / v)}[op]
    x = (10.0 ** rng.uniform(lo, hi, 500_000)).astype(np.float32)
    if op == "log":
        x = np.concatenate([x, (1.0 + rng.uniform(-0.2, 0.2, 100_000)).astype(np.float32)])  # cancellation near 1
    got = probe.unary_f32(op, x).astype(np.float64)
    want = exact(x.astype(np.float64))
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    if op == "log":  # near 1 the result's own ulp shrinks to nothing: measured in ulps of max(|log x|, 2^-3) (absolute 2^-27)
        ulp = np.maximum(ulp, 2.0 ** -27)
    err = np.abs(got - want) / ulp
    print(f"f32 {op}: largest error {err.max():.4f} ulp (at x = {x[np.argmax(err)]!r})")
    assert err.max() <= F32_MAX_ULP[op]


# ---- g. the wave paths of t2_log_i0e4 -------------------------------------------------------------------------------
def _i0e_rows():
    """One fixed set of rows of four: name -> (n, 4).  `small` / `large`: every argument on one side of 8 (by magnitude);
    `straddle`: arguments on both sides."""
    rng = np.random.default_rng(18)
    jig = lambda base: base[:, None] * (1.0 + 1e-8 * rng.uniform(-1, 1, (len(base), 4)))
    small = np.concatenate([rng.uniform(0, 8, (150, 4)), np.minimum(jig(rng.uniform(1e-3, 7.99, 150)), 8.0),
                            [[8.0] * 4, [0.0] * 4, [-3.0, -3.00000001, 2.5, -0.0], [1e-300, 7.999999999, 8.0, 0.0]]])
    large = np.concatenate([10.0 ** rng.uniform(np.log10(8.0001), 8, (150, 4)), jig(rng.uniform(8.01, 200, 150)),
                            [[np.nextafter(8.0, 9.0)] * 4, [1e300] * 4, [-9.0, -1e5, 40.0, 8.000001], [1e8, 8.5, 1e300, 1e10]]])
    b = 8.0 * (1.0 + 1e-8 * rng.uniform(-1, 1, (40, 4)))
    b[:, 0] = np.minimum(b[:, 0], 8.0)
    b[:, 1] = np.maximum(b[:, 1], np.nextafter(8.0, 9.0))
    straddle = np.concatenate([b, [[7.999, 8.001, -8.0, -0.0], [0.0, 8.0, np.nextafter(8.0, 9.0), 1e300]]])
    assert np.all(np.abs(small) <= 8.0) and np.all(np.abs(large) > 8.0)
    assert np.all((np.abs(straddle) <= 8).any(1) & (np.abs(straddle) > 8).any(1))
    return {"small": small, "large": large, "straddle": straddle}


def _interleave(i, j):
    n = min(len(i), len(j))
    out = np.empty(2 * n, np.int64)
    out[0::2], out[1::2] = i[:n], j[:n]
    return out


def test_log_i0e4_wave_paths_give_one_answer(probe):
    """Every row of a fixed set, placed in waves that take each path of t2_log_i0e4 -- all lanes small (uniform), all lanes
    large (uniform), small and large lanes interleaved with every lane one-sided (the shared 30-step loop with the per-lane
    vector coefficient loads), the same with a straddling lane in every wave (fallback: both series for everybody) -- and
    in whole waves, a 63-lane wave and a 1-lane wave: the four outputs of a row have the same bits in every placement.
    Against scipy's i0e and a 40-digit log: rtol 1e-13, atol 1e-15 (the host tests' bounds)."""
    import mpmath
    from scipy.special import i0e

    rows = _i0e_rows()
    allrows = np.concatenate([rows["small"], rows["large"], rows["straddle"]])
    ns, nl, nx = (len(rows[k]) for k in ("small", "large", "straddle"))
    S, L, X = np.arange(ns), ns + np.arange(nl), ns + nl + np.arange(nx)
    mixed = _interleave(S, L)
    with_straddler = np.concatenate([np.r_[X[w % nx], mixed[63 * w:63 * w + 63]] for w in range(len(mixed) // 63)])
    layouts = {"all_small": S, "all_large": L, "interleaved": mixed, "interleaved_with_a_straddler": with_straddler,
               "straddlers_only": X, "63_small": S[:63], "63_large": L[5:68], "63_interleaved": mixed[7:70],
               "two_waves_and_63": np.r_[mixed[:128], S[100:131], L[100:132]], "whole_waves_then_1": np.r_[mixed[:64], L[77]]}
    for k, idx in enumerate(np.r_[S[::40], L[::40], X[::15], S[-4:], L[-4:]]):  # alone in a one-lane wave
        layouts[f"alone_{k}"] = np.array([idx])
    assert len(layouts["63_interleaved"]) == 63 and len(layouts["two_waves_and_63"]) % 64 == 63
    first = {}
    for name, idx in layouts.items():
        out = probe.log_i0e4(allrows[idx])
        for i, o in zip(idx, out):
            if i in first:
                assert np.array_equal(_bits(o), first[i][1]), (name, first[i][0], int(i), allrows[i], o)
            else:
                first[int(i)] = (name, _bits(o).copy())
    assert len(first) == len(allrows)
    got = np.array([first[i][1] for i in range(len(allrows))]).view(np.float64)
    with mpmath.workdps(40):
        want = np.array([float(mpmath.log(mpmath.mpf(float(v)))) for v in i0e(allrows).ravel()]).reshape(allrows.shape)
    assert np.allclose(got, want, rtol=1e-13, atol=1e-15)


def test_log_i0e4_shared_reciprocal_root_gives_the_same_bits(probe):
    """near = true (the (8, inf) series' reciprocals from one shared reciprocal square root) on rows whose arguments lie
    within 2^-22 of the first, in waves that run the shared loop: the bits of near = false."""
    rng = np.random.default_rng(19)
    base = np.concatenate([rng.uniform(8.0001, 60, 6000), 10.0 ** rng.uniform(1, 7, 6000), rng.uniform(1e-3, 7.9999, 6000)])
    rng.shuffle(base)  # small and large lanes in every wave
    rel = np.where(rng.random((len(base), 1)) < 0.5, 1e-8, 2.0 ** -22) * rng.uniform(-1, 1, (len(base), 4))
    rel[:, 0] = 0.0
    x = base[:, None] * (1.0 + rel)
    x = x[((x <= 8).all(1) | (x > 8).all(1))]
    assert _same_bits(probe.log_i0e4(x, near=True), probe.log_i0e4(x, near=False))
    assert _same_bits(probe.i0e4_by_lane(x, near=True), probe.i0e4_by_lane(x, near=False))


def test_i0e4_by_lane_equals_the_one_value_form(probe):
    """t2_i0e4_by_lane called directly, small and large lanes interleaved (each lane loads its own series' coefficients,
    two register sets taken in turn): t2_i0e of every argument, bit for bit; scipy's i0e to 1e-14."""
    from scipy.special import i0e

    rows = _i0e_rows()
    x = np.concatenate([rows["small"], rows["large"]])[_interleave(np.arange(len(rows["small"])),
                                                                  len(rows["small"]) + np.arange(len(rows["large"])))]
    got = probe.i0e4_by_lane(x)
    assert _same_bits(got, probe.unary("i0e", x))
    assert np.allclose(got, i0e(x), rtol=1e-14, atol=0)


# ---- h. one evaluation ----------------------------------------------------------------------------------------------
EVAL_NTE = [3, 6, 8, 9, 16, 17, 32]
EVAL_MODELS = ["gaussian", "gaussian_rician", "rician"]


def eval_cases(n_te, n=40):
    """Rows and points as in test_rician_echo_loop_equals_the_statement_by_statement_objective (k inside every model's box)."""
    rng = np.random.default_rng(100 + n_te)
    te = np.round(np.linspace(30.0, 400.0, n_te))
    rows, xs = [], []
    for _ in range(n):
        k, t2v, sg = rng.uniform(610, 890), rng.uniform(20, 500), rng.choice([3.0, 20.0, 40.0, 300.0, 900.0])
        clean = k * np.exp(-te / t2v)
        rows.append(np.hypot(clean + rng.normal(size=n_te) * sg, rng.normal(size=n_te) * sg).astype(np.float32))
        xs.append([rng.uniform(601, 899), rng.uniform(11, 599), rng.uniform(2.1, 999)])
    return te, np.array(rows), np.array(xs)


def eval_config(mod, mode, te):
    """Low-field table with a sigma lower bound of 0 (config_check allows it): a lane can then sit at sigma = 0."""
    cfg = mod.config(mode, True, te)
    cfg.lb[2] = 0.0
    return cfg


def oracle_f_longdouble(mode, te, rows, xs):
    """The oracle's objective (oracle/t2fit_oracle.py) evaluated in np.longdouble.  scipy's i0e has no extended-precision
    loop: it is evaluated in float64 (its 1e-16 relative error is an absolute 1e-16 behind the log) and widened."""
    from scipy.special import i0e

    from oracle import t2fit_oracle as oracle

    ld = np.longdouble
    saved = oracle.i0e
    oracle.i0e = lambda v: i0e(np.asarray(v, np.float64)).astype(ld)
    try:
        n_par = 2 if mode == "gaussian" else 3
        with np.errstate(all="ignore"):
            return np.array([oracle._OBJ[mode](x[:n_par].astype(ld), te.astype(ld), r.astype(ld) if mode != "rician" else r)
                             for r, x in zip(rows, xs)], dtype=ld)
    finally:
        oracle.i0e = saved


def host_f_distance(mode):
    """max |f_hostsim - f_oracle| / |f_oracle| over the rows of eval_cases() for every echo count (CPU)."""
    from hostsim import sim

    worst = 0.0
    for n_te in EVAL_NTE:
        te, rows, xs = eval_cases(n_te)
        f = sim.eval_at(eval_config(sim, mode, te), rows, xs)[:, 0]
        want = oracle_f_longdouble(mode, te, rows, xs)
        worst = max(worst, float(np.max(np.abs((f - want) / want))))
    return worst


@pytest.mark.parametrize("n_te", EVAL_NTE)
@pytest.mark.parametrize("mode", EVAL_MODELS)
def test_one_evaluation_does_not_depend_on_the_neighbours(probe, mode, n_te):
    """f and the forward-difference gradient of Lbfgsb<MODEL>::eval for the same (row, x): in a wave of ordinary lanes; in
    a wave where one other lane sits at a degenerate point -- sigma at a zero lower bound, or a k so small that the step
    is no longer small beside it -- which sends the whole wave through T2_WAVE_ANY(!near) (independent roots /
    independent reciprocals); and alone in a wave.  The bits must be identical (six echoes: in the echo-count
    specialisation too, which must also equal the run-time form).  And f is the oracle's objective in np.longdouble to
    4 x the distance the host simulator keeps from it (HOST_F_DISTANCE): host and device differ by at most an ulp in
    exp, log and the rare division bit."""
    te, rows, xs = eval_cases(n_te)
    cfg = eval_config(probe, mode, te)
    plain = probe.eval_points(cfg, rows, xs)
    assert np.all(np.isfinite(plain))
    for name, xd in (("sigma_at_zero_bound", [700.0, 100.0, 0.0]), ("k_beside_the_step", [1e-3, 100.0, 50.0])):
        got = probe.eval_points(cfg, np.concatenate([rows[:1], rows]), np.concatenate([[xd], xs]))[1:]
        assert _same_bits(got, plain), (name, np.flatnonzero((_bits(got) != _bits(plain)).any(1)))
    for i in range(0, len(rows), 8):
        assert _same_bits(probe.eval_points(cfg, rows[i:i + 1], xs[i:i + 1])[0], plain[i]), i
    if n_te == 6:
        special = probe.eval_points(cfg, rows, xs, nte_special=True)
        assert _same_bits(special, plain)
        got = probe.eval_points(cfg, np.concatenate([rows[:1], rows]), np.concatenate([[[700.0, 100.0, 0.0]], xs]), nte_special=True)[1:]
        assert _same_bits(got, plain)
    want = oracle_f_longdouble(mode, te, rows, xs)
    dist = float(np.max(np.abs((plain[:, 0] - want) / want)))
    print(f"eval {mode} n_te {n_te}: |f - f_oracle| / |f_oracle| <= {dist:.3e} (host simulator: {HOST_F_DISTANCE[mode]:.3e})")
    assert dist <= 4.0 * HOST_F_DISTANCE[mode]


if __name__ == "__main__":
    import sys

    if "--host-distance" in sys.argv:
        for m in EVAL_MODELS:
            print(m, host_f_distance(m))
