"""Inputs shared by tests/test_recon_host.py and tests/test_recon_gpu.py, seeded and built once per process, and the
reference they are held to: :func:`reference_sample` and :func:`reference_merge` restate include/t2fit.h one output voxel
at a time in exact rational arithmetic.  Neither the kernels nor the numpy statement (fetal_t2mapping_amd/_resample.py)
were written from it, and the two reference functions use nothing of the statement.  (The reconstruction helpers further
down do take the statement's grid and affine construction -- ``Geometry``, ``plan`` -- to set a case up; the sampling
they are checked against is the reference's.)

The bar of a linear value ``got`` (float32) against the exact value ``e`` is derived, not measured:
``|got - e| <= ulp32(e) / 2 + 32 * 2^-53 * M`` with ``M = max |tap|`` over the taps used -- the final rounding to float32
plus the float64 arithmetic (three lerp levels ``r + w (hi - r)``, three roundings each on terms of at most ``2 M``: about
18 units of ``2^-53 M``).  A voxel that looks at a single node involves no rounding (``r + w (r - r)`` is ``r``) and
must equal it.  Cases marked ``exact`` have integer-valued nodes and affines whose entries are multiples of 1/8: every float64 operation is then
exact and the result must EQUAL the reference."""
import functools
import math
from fractions import Fraction

import numpy as np

FINITE, POS_INF, NEG_INF, NAN = 0, 1, 2, 3
HALF = Fraction(1, 2)
U53 = Fraction(1, 2 ** 53)
ARITH = 32 * U53  # the float64 part of the bar, per unit of M
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


class Reference:
    """Per output voxel (leading volume axis when the source had one): ``inside``; linear: ``cls`` (FINITE / POS_INF /
    NEG_INF / NAN), ``exact`` (Fraction where FINITE and inside, after the cast when one is asked for), ``M``, ``taps``
    (how many distinct nodes were looked at), ``negzero`` (the cast truncated a value in (-1, 0): the float is -0.0),
    ``undecided`` (the cast of a value the float64 arithmetic cannot place on one side of an integer); nearest:
    ``bits``.  ``coord_ratio``: the worst float64 coordinate error over its bound."""

    def __init__(self, shape, inside_shape):
        self.inside = np.zeros(inside_shape, bool)
        self.cls = np.zeros(shape, np.int8)
        self.exact = np.full(shape, None, object)
        self.M = np.zeros(shape, np.float64)
        self.taps = np.zeros(inside_shape, np.int32)
        self.negzero = np.zeros(shape, bool)
        self.undecided = np.zeros(shape, bool)
        self.bits = np.zeros(shape, np.uint32)
        self.coord_ratio = 0.0

    PER_VOLUME = ("cls", "exact", "M", "negzero", "undecided", "bits")

    def first(self, volumes):
        """The reference of the first ``volumes`` volumes alone."""
        part = Reference((0,), (0,))
        part.inside, part.taps, part.coord_ratio = self.inside, self.taps, self.coord_ratio
        for name in self.PER_VOLUME:
            setattr(part, name, getattr(self, name)[:volumes])
        return part


def _classify(values):
    """FINITE / POS_INF / NEG_INF / NAN of a set of taps with non-zero weight."""
    if any(v != v for v in values):
        return NAN
    pos, neg = any(v == math.inf for v in values), any(v == -math.inf for v in values)
    if pos and neg:
        return NAN
    return POS_INF if pos else NEG_INF if neg else FINITE


def reference_sample(src, A, out_shape, interp="linear", default=0.0, integer_cast=False):
    """The definition of include/t2fit.h in scalar Python.  ``src``: (Z, Y, X) or (n, Z, Y, X); ``A``: 3 x 4; ``out_shape``
    (Z, Y, X).  ``default`` is what an outside voxel holds; it plays no part here (see :func:`check_linear`)."""
    src = np.asarray(src)
    has_vol = src.ndim == 4
    vols = src if has_vol else src[None]
    n_vol = len(vols)
    nz, ny, nx = vols.shape[1:]
    n = (nx, ny, nz)
    a = [[float(v) for v in row] for row in np.asarray(A, np.float64).reshape(3, 4)]
    af = [[Fraction(v) for v in row] for row in a]
    oz, oy, ox = (int(v) for v in out_shape)
    ref = Reference((n_vol, oz, oy, ox), (oz, oy, ox))
    nearest = interp == "nearest"
    if nearest:
        patterns = np.ascontiguousarray(vols).view(np.uint32)
    else:
        if interp != "linear":
            raise ValueError(interp)
        values = [v.astype(np.float64).tolist() for v in vols]  # float32 -> float: exact
    for iz in range(oz):
        for iy in range(oy):
            for ix in range(ox):
                c = []
                for k in range(3):
                    r, rf = a[k], af[k]
                    ck = ((r[0] * ix + r[1] * iy) + r[2] * iz) + r[3]  # IEEE doubles in the order of the definition
                    exact = rf[0] * ix + rf[1] * iy + rf[2] * iz + rf[3]
                    bound = 4 * U53 * (abs(rf[0] * ix) + abs(rf[1] * iy) + abs(rf[2] * iz) + abs(rf[3]))
                    err = abs(Fraction(ck) - exact)
                    assert err <= bound, ("coordinate", k, ix, iy, iz, ck)
                    if bound:
                        ref.coord_ratio = max(ref.coord_ratio, float(err / bound))
                    c.append(ck)
                if not all(-0.5 <= c[k] < n[k] - 0.5 for k in range(3)):  # the inside test reads the float64 value
                    continue
                ref.inside[iz, iy, ix] = True
                cf = [Fraction(v) for v in c]
                if nearest:
                    x, y, z = (min(max(math.floor(cf[k] + HALF), 0), n[k] - 1) for k in range(3))
                    ref.bits[:, iz, iy, ix] = patterns[:, z, y, x]
                    continue
                axis = []
                for k in range(3):
                    lo = min(max(math.floor(cf[k]), 0), n[k] - 1)
                    w = max(cf[k] - lo, Fraction(0))
                    axis.append([(lo, 1 - w)] + ([(min(lo + 1, n[k] - 1), w)] if w != 0 else []))
                taps = [(x, y, z, wx * wy * wz) for z, wz in axis[2] for y, wy in axis[1] for x, wx in axis[0]]
                ref.taps[iz, iy, ix] = len({t[:3] for t in taps})
                for v in range(n_vol):
                    vals = [values[v][z][y][x] for x, y, z, _ in taps]
                    cls = _classify(vals)
                    m = max((abs(t) for t in vals if abs(t) != math.inf and t == t), default=0.0)
                    e = None
                    if cls == FINITE:
                        e = sum((w * Fraction(t) for (_, _, _, w), t in zip(taps, vals)), Fraction(0))
                    if integer_cast and cls != NAN:
                        if cls == FINITE:
                            t = math.trunc(e)  # toward zero
                            if ref.taps[iz, iy, ix] > 1 and -32769 < e < 32768 and abs(e - round(e)) <= ARITH * Fraction(m):
                                ref.undecided[v, iz, iy, ix] = True
                            ref.negzero[v, iz, iy, ix] = t == 0 and e < 0
                            e = Fraction(min(max(t, -32768), 32767))
                        else:
                            e, cls = Fraction(32767 if cls == POS_INF else -32768), FINITE
                    ref.cls[v, iz, iy, ix], ref.exact[v, iz, iy, ix], ref.M[v, iz, iy, ix] = cls, e, m
    if not has_vol:
        for name in Reference.PER_VOLUME:
            setattr(ref, name, getattr(ref, name)[0])
    return ref


def ulp32(e):
    """The spacing of float32 at the exact value ``e`` (a Fraction)."""
    e = abs(e)
    if e < Fraction(1, 2 ** 126):
        return Fraction(1, 2 ** 149)
    k = math.frexp(float(e))[1]  # 2^(k-1) <= |e| < 2^k, up to the rounding of float(e)
    while Fraction(2) ** (k - 1) > e:
        k -= 1
    while Fraction(2) ** k <= e:
        k += 1
    return Fraction(2) ** (k - 24)


def _same_default(got, default):
    d = np.float32(default) if not isinstance(default, np.float32) else default
    if d != d:
        return np.isnan(got)
    return got.view(np.uint32) == np.array(d, np.float32).view(np.uint32)


def check_linear(got, ref, default=0.0, exact=False, integer_cast=False, max_skip=0.0):
    """Hold a float32 linear result to the reference: the default outside, the non-finite class by position, and the
    finite values equal (``exact``) or within the bar.  Undecided casts are skipped only when ``max_skip`` allows a
    share of the inside voxels.  Returns ``(worst |got - e| / bar, worst (|got - e| - ulp32 / 2) / (ARITH M))``."""
    got = np.ascontiguousarray(got)
    assert got.dtype == np.float32 and got.shape == ref.cls.shape, (got.dtype, got.shape, ref.cls.shape)
    inside = np.broadcast_to(ref.inside, got.shape)
    with np.errstate(over="ignore"):
        assert np.all(_same_default(got, default)[~inside]), "an outside voxel does not hold the default"
    for cls, test in ((NAN, np.isnan), (POS_INF, lambda v: v == np.inf), (NEG_INF, lambda v: v == -np.inf)):
        sel = inside & (ref.cls == cls)
        assert np.all(test(got[sel])), ("non-finite class", cls, int(np.sum(~test(got[sel]))), int(sel.sum()))
    finite = inside & (ref.cls == FINITE)
    assert np.all(np.isfinite(got[finite])), "a finite reference value came out non-finite"
    worst, worst_excess, skipped = 0.0, 0.0, 0
    for idx in zip(*np.nonzero(finite)):
        e, g = ref.exact[idx], got[idx]
        single = ref.taps[idx[-3:]] == 1
        if exact or single or integer_cast:
            if integer_cast and not exact and not single and ref.undecided[idx]:
                skipped += 1
                continue
            want = np.float32(float(e))
            assert Fraction(float(want)) == e, ("the case is not exact in float32", idx, e)
            assert g == want, (idx, float(g), float(want))
            if ref.negzero[idx]:
                assert np.signbit(g), ("truncating a value in (-1, 0) gives -0.0", idx)
            continue
        err = abs(Fraction(float(g)) - e)
        half, arith = ulp32(e) / 2, ARITH * Fraction(float(ref.M[idx]))
        assert err <= half + arith, (idx, float(g), float(e), float(err), float(half + arith))
        worst = max(worst, float(err / (half + arith)))
        if arith:
            worst_excess = max(worst_excess, float((err - half) / arith))
    n_inside = int(inside.sum())
    assert skipped <= max_skip * n_inside, (skipped, n_inside)
    return worst, worst_excess


def check_nearest(got, ref, default):
    """Nearest copies the 32-bit pattern: the bits must match, NaN payloads included; the default outside."""
    got = np.ascontiguousarray(got)
    assert got.shape == ref.bits.shape and got.dtype.itemsize == 4, (got.dtype, got.shape)
    inside = np.broadcast_to(ref.inside, got.shape)
    with np.errstate(over="ignore"):
        d = np.array(default, got.dtype).view(np.uint32)
    want = np.where(inside, ref.bits, d)
    assert np.array_equal(got.view(np.uint32), want), int(np.sum(got.view(np.uint32) != want))


def bits_differ(got, want, nan_by_position=True):
    """How many elements differ: the same NaN mask and the same bits wherever not NaN (a NaN that arithmetic made has
    no defined sign or payload: numpy's inf - inf is 0xffc00000 on x86, the device makes the positive quiet NaN).  With
    ``nan_by_position=False`` (nearest: the payload is copied) all 32 bits."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    diff = got.view(np.uint32) != want.view(np.uint32)
    if nan_by_position and got.dtype == np.float32:
        gn, wn = np.isnan(got), np.isnan(want)
        diff = (gn != wn) | (diff & ~gn)
    return int(np.sum(diff))


def reference_merge(a, b, c):
    """``((a + b) + c) / 3`` exact, from three float32 arrays: ``(exact, bar_arith)`` object arrays of Fractions (None
    where the sum is not finite).  ``bar_arith`` bounds the float64 roundings in the order of the definition: one on
    ``a + b``, one on the sum of three, one on the quotient, each relative to the partial result it rounds."""
    a, b, c = (np.asarray(v, np.float32) for v in (a, b, c))
    exact, arith = np.full(a.shape, None, object), np.full(a.shape, None, object)
    for idx in np.ndindex(a.shape):
        x, y, z = float(a[idx]), float(b[idx]), float(c[idx])
        if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
            continue
        s1 = Fraction(x) + Fraction(y)
        s2 = s1 + Fraction(z)
        exact[idx] = s2 / 3
        arith[idx] = 2 * U53 * (abs(s1) + 2 * abs(s2))
    return exact, arith


def check_merge(got, a, b, c):
    got = np.ascontiguousarray(got)
    assert got.dtype == np.float32
    exact, arith = reference_merge(a, b, c)
    with np.errstate(all="ignore"):
        s = (np.asarray(a, np.float64) + np.asarray(b, np.float64)) + np.asarray(c, np.float64)
    for idx in np.ndindex(got.shape):
        if exact[idx] is None:  # a non-finite input: NaN or Inf by IEEE addition, which has one answer
            assert (np.isnan(got[idx]) and np.isnan(s[idx])) or got[idx] == np.float32(s[idx] / 3.0), idx
            continue
        err = abs(Fraction(float(got[idx])) - exact[idx])
        assert err <= ulp32(exact[idx]) / 2 + arith[idx], (idx, float(got[idx]), float(exact[idx]))


# ---- the cases ---------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, src, A, out_shape, interp="linear", default=0.0, integer_cast=False, exact=True, max_skip=0.0,
                 meta=None):
        self.meta = meta
        self.name, self.src, self.A, self.out_shape = name, src, np.ascontiguousarray(A, np.float64), tuple(out_shape)
        self.interp, self.default, self.integer_cast, self.exact, self.max_skip = interp, default, integer_cast, exact, max_skip

    @property
    def n_vol(self):
        return self.src.shape[0] if self.src.ndim == 4 else 1

    def __repr__(self):
        return self.name


_REFERENCES = {}


def reference(case):
    """The reference of a case, computed once per process."""
    if case.name not in _REFERENCES:
        _REFERENCES[case.name] = reference_sample(case.src, case.A, case.out_shape, case.interp, case.default, case.integer_cast)
    return _REFERENCES[case.name]


def check(case, got, volumes=None):
    """Hold ``got`` (the result of the case, or of its first ``volumes`` volumes) to the reference."""
    ref = reference(case)
    if volumes is not None:
        ref = ref.first(volumes)
    if case.interp == "nearest":
        check_nearest(got, ref, case.default)
        return 0.0, 0.0
    return check_linear(got, ref, case.default, case.exact, case.integer_cast, case.max_skip)


def integer_volume(shape, seed, lo=-2000, hi=2000):
    return np.random.default_rng(seed).integers(lo, hi, size=shape).astype(np.float32)


def label_volume(shape, seed):
    """int32 ids over the whole range: a path through float32 cannot carry them."""
    return np.random.default_rng(seed).integers(INT32_MIN, INT32_MAX, size=shape, endpoint=True).astype(np.int32)


FOLLOW = {0: (0, 1, 2), 1: (1, 0, 2), 2: (2, 0, 1)}  # lane axis -> the output axis that source x, y, z follow


def permutation_affine(la, step=(1.0, 1.0, 1.0), shift=(0.0, 0.0, 0.0), sign=(1, 1, 1)):
    """Source axis a follows output axis FOLLOW[la][a] with ``step[a]`` and ``shift[a]``: the kernel's lane axis is la."""
    A = np.zeros((3, 4))
    for a in range(3):
        A[a, FOLLOW[la][a]] = sign[a] * step[a]
        A[a, 3] = shift[a]
    return A


LANE_AXES = (0, 1, 2)
BRICK_OUTPUTS = {  # (ox, oy, oz): one voxel, thinner than a brick along each axis, the exact brick, the brick plus one
    0: [(1, 1, 1), (1, 1, 40), (1, 40, 1), (40, 1, 1), (64, 4, 2), (65, 5, 3)],
    1: [(1, 1, 1), (1, 1, 40), (1, 40, 1), (40, 1, 1), (16, 32, 1), (17, 33, 2)],
    2: [(1, 1, 1), (1, 1, 40), (1, 40, 1), (40, 1, 1), (16, 1, 32), (17, 2, 33)],
}


@functools.lru_cache(maxsize=None)
def brick_cases(la):
    """For the lane axis ``la``: every output of BRICK_OUTPUTS[la], three volumes, linear (integer-valued float32) and
    nearest (int32 over the whole range).  Source axis a is sampled at c = i / 2 - 3/4 of the output axis it follows (the
    first output voxel is outside, the second on the lower rim; the source is just short enough that the last ones are
    outside too); an output axis of one voxel sits at c = 1/4 of a one-voxel source axis."""
    cases = []
    for k, (ox, oy, oz) in enumerate(BRICK_OUTPUTS[la]):
        o = (ox, oy, oz)
        n, step, shift = [], [], []
        for a in range(3):
            length = o[FOLLOW[la][a]]
            n.append(1 if length == 1 else max(1, (length - 1) // 2))
            step.append(0.5)
            shift.append(0.25 if length == 1 else -0.75)
        A = permutation_affine(la, step, shift)
        shape = (3, n[2], n[1], n[0])
        name = f"brick-la{la}-{ox}x{oy}x{oz}"
        cases.append(Case(name + "-linear", integer_volume(shape, 100 + 10 * la + k), A, (oz, oy, ox), default=-7.0))
        cases.append(Case(name + "-nearest", label_volume(shape, 200 + 10 * la + k), A, (oz, oy, ox), "nearest", default=-1))
    return cases


THIN_SOURCES = [(1, 6, 5), (6, 1, 5), (6, 5, 1), (1, 1, 1)]  # (Z, Y, X): one voxel along z, y, x, and a single voxel


@functools.lru_cache(maxsize=None)
def thin_source_cases(la):
    """Sources with a one-voxel axis under a sheared dyadic affine (steps 1/2, cross terms 1/8): on that axis the
    voxel is inside iff -1/2 <= c < 1/2 and both taps are node 0."""
    cases = []
    for k, shape in enumerate(THIN_SOURCES):
        A = permutation_affine(la, (0.5, 0.5, 0.5), (-0.625, -0.375, -0.5))
        A[0, FOLLOW[la][1]] += 0.125
        A[1, FOLLOW[la][2]] -= 0.125
        A[2, FOLLOW[la][0]] += 0.125
        cases.append(Case(f"thin-la{la}-{shape[0]}x{shape[1]}x{shape[2]}", integer_volume(shape, 300 + k), A, (5, 6, 7), default=3.0))
    return cases


RIM_SHIFTS = (-0.75, -0.5, -0.25, 0.25, 0.5)
RIM_N = 6


@functools.lru_cache(maxsize=None)
def rim_cases(la):
    """A whole-voxel grid moved by a dyadic shift along one source axis of length 6, for each axis, shift and
    interpolation: c = -1/2 is inside and takes the edge value, c = n - 1/2 is outside, a nearest tie c = k + 1/2 goes up."""
    cases = []
    for axis in range(3):
        n = [3, 4, 5]
        n[axis] = RIM_N
        o = [0, 0, 0]
        for a in range(3):
            o[FOLLOW[la][a]] = n[a]
        for s in RIM_SHIFTS:
            shift = [0.0, 0.0, 0.0]
            shift[axis] = s
            A = permutation_affine(la, shift=shift)
            for interp in ("linear", "nearest"):
                cases.append(Case(f"rim-la{la}-axis{axis}-{s:+.2f}-{interp}", integer_volume((n[2], n[1], n[0]), 400 + axis), A,
                                  (o[2], o[1], o[0]), interp, default=-7.0, meta=(la, axis, s)))
    return cases


@functools.lru_cache(maxsize=None)
def lane_choice_cases():
    """What lane_axis() can be given: a tie (45 degrees about z: the lower axis wins), a negative dominant step, a
    signed permutation, and a first row without steps (source x constant).  The result must not depend on the choice."""
    s = math.sqrt(0.5)
    src = integer_volume((5, 8, 9), 500)
    tie = np.array([[s, s, 0, -1.5], [-s, s, 0, 3.25], [0, 0, 1, -0.25]])
    assert abs(tie[0, 0]) == abs(tie[0, 1])
    flipped = np.array([[-1.0, 0, 0, 8.25], [0, -1.0, 0, 7.5], [0, 0, 1.0, -0.5]])
    signed = np.array([[0, -1.0, 0, 7.75], [1.0, 0, 0, -0.25], [0, 0, -0.5, 2.5]])
    constant = np.array([[0, 0, 0, 2.25], [0.5, 0, 0.125, -0.25], [0, 0.5, 0, 0.375]])
    return [Case("lane-tie45", src, tie, (6, 9, 10), default=-7.0, exact=False),
            Case("lane-flipped", src, flipped, (6, 9, 10), default=-7.0),
            Case("lane-signed-permutation", src, signed, (10, 9, 10), default=-7.0),
            Case("lane-zero-first-row", src, constant, (10, 9, 10), default=-7.0)]


NAN_QUIET, NAN_SIGNALLING = 0x7FC12345, 0xFFA00001


@functools.lru_cache(maxsize=None)
def nearest_cases():
    """Labels and float32 patterns that only a copy of the 32 bits carries, under c = i / 2 + shift with ties
    (shift -1/2: c = -1/2 -> node 0, c = k + 1/2 -> k + 1), c in [-1/2, 0) and outside voxels; the defaults at the edge
    of each type."""
    A = permutation_affine(0, (0.5, 0.5, 0.5), (-0.5, -0.75, -0.25))
    lab = label_volume((4, 5, 6), 600)
    lab[0, 0, :4] = (INT32_MIN, INT32_MAX, 16777217, 16777219)
    lab[3, 4, 2:6] = (16777219, INT32_MIN, 16777217, INT32_MAX)
    flt = integer_volume((4, 5, 6), 601).view(np.uint32).copy()
    flt[0, 0, :3] = (NAN_QUIET, NAN_SIGNALLING, 0x80000000)
    flt[2, 3, 1:4] = (0x80000000, NAN_SIGNALLING, NAN_QUIET)
    flt = flt.view(np.float32)
    out = (9, 12, 13)
    cases = [Case(f"nearest-int32-default{d}", lab, A, out, "nearest", default=d) for d in (INT32_MIN, INT32_MAX)]
    cases += [Case(f"nearest-float32-default-{name}", flt, A, out, "nearest", default=d)
              for name, d in (("nan", math.nan), ("negzero", -0.0), ("1e39", 1e39))]
    return cases


NON_FINITE_NODES = ((1, 2, 3, np.inf), (3, 4, 5, -np.inf), (2, 1, 1, np.nan), (1, 2, 4, np.inf), (3, 4, 4, np.inf),
                    (4, 5, 6, np.inf), (0, 0, 0, -np.inf), (4, 0, 6, np.nan))  # (z, y, x, value)


def _non_finite_source():
    v = integer_volume((5, 6, 7), 700)
    for z, y, x, value in NON_FINITE_NODES:
        v[z, y, x] = value
    return v


def rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    m = {0: [[1, 0, 0], [0, c, -s], [0, s, c]], 1: [[c, 0, s], [0, 1, 0], [-s, 0, c]], 2: [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis]
    return np.array(m, np.float64)


def oblique_affine(scale, shift, angles=(7.0, -5.0, 11.0)):
    A = np.empty((3, 4))
    A[:, :3] = scale * (rot(0, angles[0]) @ rot(1, angles[1]) @ rot(2, angles[2]))
    A[:, 3] = shift
    return A


@functools.lru_cache(maxsize=None)
def non_finite_cases():
    """+Inf, -Inf and NaN nodes (in the interior, next to each other, in corners) under real interpolation: a shift by a
    whole voxel along one axis (weight 0 there: the upper neighbour along it must not be looked at) with weights 1/4 and
    3/4 on the other two, for each axis; and an oblique affine."""
    src = _non_finite_source()
    cases = []
    for whole in range(3):
        step, shift, out = [0.5, 0.5, 0.5], [0.25, 0.25, 0.25], [14, 12, 10]
        step[whole], shift[whole], out[whole] = 1.0, 1.0, src.shape[2 - whole]
        cases.append(Case(f"non-finite-whole-axis{whole}", src, permutation_affine(0, step, shift), out[::-1], default=-7.0))
    cases.append(Case("non-finite-oblique", src, oblique_affine(0.8, (0.3, -0.2, 0.4)), (6, 7, 8), default=-7.0, exact=False))
    return cases


CAST_TAPS = (-40000.0, -32769.0, -32768.0, -3.0, -1.0, 0.0, 1.0, 4.0, 32767.0, 32768.0, 40000.0, np.inf, -np.inf, np.nan)


def cast_source():
    """(3, 4, 14): along x the 14 taps in an order that puts -1 next to 0 (1/4 of the way: -0.25 -> -0.0), the
    saturation bounds next to their neighbours and the non-finite ones next to finite ones; every row rotated by 3."""
    row = np.array([-1.0, 0.0, 1.0, 4.0, -3.0, 32767.0, 32768.0, 40000.0, np.inf, -40000.0, -32769.0, -32768.0, -np.inf, np.nan],
                   np.float32)
    assert sorted(map(repr, row.tolist())) == sorted(map(repr, np.float32(CAST_TAPS).tolist()))
    return np.stack([np.stack([np.roll(row, 3 * (y + 4 * z)) for y in range(4)]) for z in range(3)])


@functools.lru_cache(maxsize=None)
def cast_cases():
    """The integer cast on saturating and non-finite taps with weights in multiples of 1/8 (step 3/8 along x walks all
    eight, 1/2 along y, whole voxels along z), cast on and off: every float64 operation is exact."""
    src = cast_source()
    A = permutation_affine(0, (0.375, 0.5, 1.0), (-0.375, -0.25, 0.0))
    return [Case("cast-on", src, A, (3, 9, 39), default=-7.0, integer_cast=True),
            Case("cast-off-unsaturated", integer_volume((3, 4, 14), 800), A, (3, 9, 39), default=-7.0)]


@functools.lru_cache(maxsize=None)
def oblique_cases():
    """Four oblique 9 x 8 x 12 outputs of a 7 x 6 x 5 source, data centred on 500 and on 0: where the bar, not
    equality, is the measure."""
    cases = []
    for k, (scale, shift, angles) in enumerate(((0.55, (0.4, 0.1, -0.3), (7.0, -5.0, 11.0)), (0.6, (-0.2, 0.6, 0.2), (-12.0, 9.0, 31.0)))):
        for name, centre in (("500", 500.0), ("0", 0.0)):
            v = np.random.default_rng(900 + k).normal(centre, 200.0, size=(5, 6, 7)).astype(np.float32)
            cases.append(Case(f"oblique{k}-centre{name}", v, oblique_affine(scale, shift, angles), (12, 8, 9), default=-7.0, exact=False))
    return cases


# group name -> builder of its cases: what the host and the device tests are parametrised over
SINGLE_STAGE_GROUPS = {**{f"brick-la{la}": functools.partial(brick_cases, la) for la in LANE_AXES},
                       **{f"thin-la{la}": functools.partial(thin_source_cases, la) for la in LANE_AXES},
                       **{f"rim-la{la}": functools.partial(rim_cases, la) for la in LANE_AXES},
                       "lane-choice": lane_choice_cases, "nearest": nearest_cases, "non-finite": non_finite_cases,
                       "cast": cast_cases, "oblique": oblique_cases}


# ---- reconstruction ----------------------------------------------------------------------------------------------------
RECON_SIZE, RECON_SPACING = (9, 8, 3), (1.0, 1.0, 2.5)
RECON_DIRECTIONS = {"ax": np.eye(3), "cor": np.array([[1, 0, 0], [0, 0, 1], [0, 1, 0.0]]), "sag": np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0.0]])}
RECON_RES, RECON_FIXED = (0.8, 1.0, 1.5), ("ax", "cor", "sag")


def rigid(angles_deg, shift):
    t = np.eye(4)
    t[:3, :3] = rot(0, angles_deg[0]) @ rot(1, angles_deg[1]) @ rot(2, angles_deg[2])
    t[:3, 3] = shift
    return t


def recon_geometries():
    """Three (9, 8, 3) stacks of 1 x 1 x 2.5 mm around one centre, with the scanner's three direction matrices."""
    from fetal_t2mapping_amd import _resample as R

    centre = np.array([1.0, -2.0, 3.0])
    geoms = {}
    for o, d in RECON_DIRECTIONS.items():
        extent = d @ (np.array(RECON_SPACING) * (np.array(RECON_SIZE) - 1) / 2.0)
        geoms[o] = R.Geometry(RECON_SIZE, RECON_SPACING, centre - extent, d.ravel())
    return geoms


@functools.lru_cache(maxsize=None)
def recon_case(fixed, res, n_vol=1, kind="both"):
    """``(stacks, geoms, kwargs)`` of a reconstruction.  ``kind``: 'both' (a small rigid transform on each moving
    stack), 'far' (one of them translated so far that part of the fixed grid maps outside that stack's stage-1 grid: the
    default 0 is then a stage-2 tap next to live values) or 'cast' (the cast case's saturating and non-finite values
    among ordinary ones, integer_cast at both stages)."""
    geoms = recon_geometries()
    rng = np.random.default_rng(1000 + 10 * RECON_FIXED.index(fixed) + RECON_RES.index(res))
    shape = (n_vol,) + RECON_SIZE[::-1]
    stacks = {o: rng.normal(600, 150, size=shape).astype(np.float32) for o in RECON_FIXED}
    moving = [o for o in RECON_FIXED if o != fixed]
    transforms = {moving[0]: rigid((2.0, -1.5, 3.0), (0.3, -0.4, 0.2)), moving[1]: rigid((-2.5, 1.0, 1.5), (-0.2, 0.35, -0.3))}
    kwargs = {"fixed": fixed, "res": res, "transforms": transforms}
    if kind == "far":
        transforms[moving[1]] = rigid((-2.5, 1.0, 1.5), (2.7, -1.9, 2.2))
    elif kind == "cast":
        special = np.float32(CAST_TAPS)
        for o in stacks:
            put = rng.random(shape) < 0.08
            stacks[o][put] = special[rng.integers(0, len(special), size=int(put.sum()))]
        kwargs["integer_cast"] = True
    elif kind != "both":
        raise ValueError(kind)
    return stacks, geoms, kwargs


def ragged(shape, brick=(4, 8, 16)):
    """True when no axis of ``shape`` (Z, Y, X) is a multiple of the fused kernel's 16 x 8 x 4 brick."""
    return all(n % b != 0 for n, b in zip(shape[-3:], brick))


RECON_CAST_MAX_SKIP = 0.005
_STAGE_REFERENCES = {}


def _stage_reference(src, A, out_shape, cast):
    """reference_sample of a stage, kept per process by its inputs' bytes (the host and the device tests hold the same
    arrays to it)."""
    import hashlib

    src, A = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(A, np.float64)
    key = (hashlib.sha1(src.tobytes() + A.tobytes()).hexdigest(), src.shape, tuple(out_shape), cast)
    if key not in _STAGE_REFERENCES:
        _STAGE_REFERENCES[key] = reference_sample(src, A, out_shape, "linear", 0.0, cast)
    return _STAGE_REFERENCES[key]


def check_reconstruction(stacks, geoms, kwargs, merged, stages):
    """Hold a reconstruction (``merged`` and the stage arrays ``{"H": [3], "R": [2]}`` it was made of) to the reference:
    stage 1 from the stacks, stage 2 from these very stage-1 arrays (identical inputs: a one-ulp stage-1 difference would
    otherwise compound), the merge from these stage-2 arrays.  Returns the worst ratio to the bar."""
    from fetal_t2mapping_amd import _resample as R

    cast = bool(kwargs.get("integer_cast", False))
    order, hi, a1, a2 = R.plan({o: R.as_geometry(geoms[o], np.asarray(stacks[o]).shape[-3:]) for o in geoms}, kwargs.get("fixed", "ax"),
                               kwargs.get("res", 1.0), kwargs.get("transforms"))
    skip = RECON_CAST_MAX_SKIP if cast else 0.0
    worst = 0.0
    for i, o in enumerate(order):
        assert stages["H"][i].dtype == np.float32
        ref = _stage_reference(stacks[o], a1[i], hi[i].shape, cast)
        worst = max(worst, check_linear(stages["H"][i], ref, 0.0, False, cast, skip)[0])
    for m in (1, 2):
        ref = _stage_reference(stages["H"][m], a2[m - 1], hi[0].shape, cast)
        worst = max(worst, check_linear(stages["R"][m - 1], ref, 0.0, False, cast, skip)[0])
    check_merge(merged, stages["H"][0], stages["R"][0], stages["R"][1])
    return worst


MERGE_TRIPLES = np.float32([[2.0 ** 60, -2.0 ** 60, 1.0], [1.0, 2.0 ** 60, -2.0 ** 60], [2.0 ** 40, 3.0, -2.0 ** 40], [1e30, 1.0, -1e30],
                            [-0.0, -0.0, -0.0], [np.inf, 1.0, 2.0], [np.inf, -np.inf, 0.0], [np.nan, 1.0, 2.0], [3.0, 3.0, 3.0],
                            [16777216.0, 1.0, 1.0], [-32768.0, 32767.0, 0.5]])


def merge_inputs():
    """Three float32 arrays: ordinary values, and triples whose float64 sum depends on the order ((a + b) + c is exact
    where a + (b + c) loses c)."""
    rng = np.random.default_rng(1100)
    a, b, c = (np.concatenate([rng.normal(600, 150, 200).astype(np.float32), MERGE_TRIPLES[:, k]]) for k in range(3))
    return a, b, c


def rim_facts(case, got):
    """What a rim case must show whatever the reference says: with the shift s along source axis `axis` (n = 6) the output
    index i along the axis that follows it sits at c = i + s.  c = -1/2 is inside and is the edge node; c < -1/2 and
    c >= n - 1/2 are the default; linear on the rim replicates the edge; a nearest tie c = k + 1/2 takes node k + 1."""
    (la, axis, s), interp = case.meta, case.interp
    # the source laid out as the output: output numpy axis 2 - FOLLOW[la][a] is source numpy axis 2 - a
    axes = [0, 0, 0]
    for a in range(3):
        axes[2 - FOLLOW[la][a]] = 2 - a
    src = np.transpose(case.src, axes)
    along = 2 - FOLLOW[la][axis]
    take = lambda arr, i: np.take(arr, i, axis=along)
    assert src.shape == got.shape and src.shape[along] == RIM_N
    for i in range(RIM_N):
        c = i + s
        if c < -0.5 or c >= RIM_N - 0.5:
            assert np.all(take(got, i) == case.default), (case, i)
        elif interp == "nearest":
            assert np.array_equal(take(got, i), take(src, min(max(math.floor(c + 0.5), 0), RIM_N - 1))), (case, i)
        elif c <= 0 or c >= RIM_N - 1:
            assert np.array_equal(take(got, i), take(src, 0 if c <= 0 else RIM_N - 1)), (case, i)
        else:
            lo = math.floor(c)
            want = take(src, lo).astype(np.float64) * (1 - (c - lo)) + take(src, lo + 1).astype(np.float64) * (c - lo)
            assert np.array_equal(take(got, i), want.astype(np.float32)), (case, i)


def recon_facts(kind, stages):
    """The reconstruction cases reach what they are there for: a stage-1 grid whose last nodes lie outside its stack (the
    default 0 is then a stage-2 tap beside live values), and for 'far' a part of the fixed grid outside a moving grid."""
    for h, r in zip(stages["H"][1:], stages["R"]):
        assert np.any(r != 0)
        if kind != "both":
            assert np.any(h == 0) and np.any(r == 0)
    if kind == "cast":
        flat = np.concatenate([h.ravel() for h in stages["H"]])
        assert (flat == 32767).any() and (flat == -32768).any() and np.isnan(flat).any()
