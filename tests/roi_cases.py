"""What csrc/t2fit_roi.hip fixes about the per-label statistics, stated in numpy (`statement`), a reference written from
the definition in exact arithmetic (`reference`), the derived bars between the two (`bars`), and the volumes on which
tests/test_roi_edges_host.py holds the statement to the reference and tests/test_roi_edges_gpu.py holds the device to the
statement bit for bit.  Nothing here imports the package."""
import functools
import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

LANES = 256   # threads of the workgroup that reduces one segment
SPAN = 8192   # voxels one wave of the counting sort walks (volumes up to 2^27 voxels)
U = Fraction(1, 2 ** 53)
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
F32_MAX = np.float32(np.finfo(np.float32).max)
F32_DENORM = np.float32(1e-45)  # the smallest float32 denormal, 2^-149


# ---- the order-preserving key of the median ---------------------------------------------------------------------------
def float_key(x):
    """uint32 image of float32 values whose unsigned order is the floats' total order: negatives with all bits flipped,
    the others with the sign bit flipped (so -0.0 sorts just below +0.0)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    top = np.uint32(0x80000000)
    return np.where(u & top, ~u, u ^ top).astype(np.uint32)


def key_float(k):
    k = np.ascontiguousarray(k, np.uint32)
    top = np.uint32(0x80000000)
    return np.where(k & top, k ^ top, ~k).astype(np.uint32).view(np.float32)


# ---- the statement ------------------------------------------------------------------------------------------------------
# (the four pieces below are module attributes so that tests/test_roi_edges_host.py can patch a mutation in and out)
def _in_segment(values):
    """The values of one label as the segment holds them: in voxel order."""
    return values


def _rows(v):
    """The zero-padded (-1, 256) view: row r holds elements 256 r .. 256 r + 255, thread t owns column t.  (Adding the
    padding's +0.0 changes no bit: a thread's sum starts from +0.0, so it is never -0.0.)"""
    k = -(-len(v) // LANES)
    pad = np.zeros(k * LANES, np.float64)
    pad[: len(v)] = v
    return pad.reshape(k, LANES)


def _halve(sh):
    """sh[t] += sh[t + off] for off = 128 .. 1."""
    sh = np.array(sh, np.float64)
    off = LANES // 2
    while off:
        sh[:off] = sh[:off] + sh[off: 2 * off]
        off //= 2
    return sh[0]


def tree_sum(v):
    """Thread t adds elements t, t + 256, ... one after the other from +0.0; the 256 sums are then halved."""
    sh = np.zeros(LANES, np.float64)
    for row in _rows(np.asarray(v, np.float64)):  # an explicit loop: the order is stated here, not left to numpy
        sh = sh + row
    return _halve(sh)


def _moments(x):
    """numpy's two rounds on the fixed tree: mean = S / n, then the mean of d * d with d = x - mean (multiply and add
    apart: the library is built with -ffp-contract=off), then sqrt."""
    n = np.float64(len(x))
    mean = tree_sum(x) / n
    d = x - mean
    return mean, np.sqrt(tree_sum(d * d) / n)


def _median(x32):
    k = np.sort(float_key(x32))
    n = len(k)
    a, b = key_float(k[[(n - 1) // 2, n // 2]]).astype(np.float64)
    return 0.5 * (a + b)


@dataclass
class Stats:
    mean: np.ndarray
    std: np.ndarray
    median: np.ndarray
    count: np.ndarray
    valid: np.ndarray
    segments: list


def statement(map_flat, roi_flat, n_labels):
    """mean / std / median (float64), count / valid (int64) of the labels 1..n_labels and their segments (float32, the
    non-NaN values in voxel order).  Labels outside 1..n_labels belong to nobody; an empty segment gives three NaNs."""
    m = np.ascontiguousarray(map_flat, np.float32).reshape(-1)
    roi = np.asarray(roi_flat).reshape(-1)
    out = Stats(np.full(n_labels, np.nan), np.full(n_labels, np.nan), np.full(n_labels, np.nan),
                np.zeros(n_labels, np.int64), np.zeros(n_labels, np.int64), [])
    with np.errstate(all="ignore"):
        for i in range(n_labels):
            sel = m[roi == i + 1]
            seg = _in_segment(sel[~np.isnan(sel)])
            out.count[i], out.valid[i] = len(sel), len(seg)
            out.segments.append(seg)
            if len(seg):
                out.mean[i], out.std[i] = _moments(seg.astype(np.float64))
                out.median[i] = _median(seg)
    return out


# ---- the reference, from the definition -----------------------------------------------------------------------------------
@dataclass
class Ref:
    mean: Fraction
    var: Fraction
    median: float
    abs_sum: Fraction


def reference(values):
    """Finite float32 values -> the exact mean, the exact variance sum (x - mean)^2 / n about it, sum |x| (all rationals)
    and the median from sorted() on the total order (value, then sign bit).  Every float32 is an integer multiple of
    2^-149, so the sums are sums of Python integers."""
    xs = [float(v) for v in values]
    n = len(xs)
    assert n and all(math.isfinite(v) for v in xs)
    m = [int(v * 2.0 ** 149) for v in xs]  # exact: a power of two, no overflow in float64
    s = sum(m)
    mean = Fraction(s, n << 149)
    var = Fraction(sum((n * v - s) ** 2 for v in m), n ** 3 << 298)  # x - mean = (n m - s) / (n 2^149)
    order = sorted(xs, key=lambda v: (v, math.copysign(1.0, v)))
    return Ref(mean, var, 0.5 * (order[(n - 1) // 2] + order[n // 2]), Fraction(sum(abs(v) for v in m), 1 << 149))


def bars(n, abs_sum, var):
    """(bar of |mean - mu|, bar of |std^2 - V|) of the statement against the reference, derived; u = 2^-53,
    k = ceil(n / 256).

    Mean.  A thread adds its k elements to +0.0: the first add is exact, the others round, k - 1 roundings; the halving
    has 8 levels, one rounding each on the path of any element; S / n rounds once.  Every rounding is relative to a
    partial sum, which is at most sum |x| in magnitude, so to first order |mean - mu| <= (k + 8) u sum |x| / n; the bar
    is delta = 2 (k + 9) u sum |x| / n, the factor 2 covering the terms of second order.

    Variance.  d = x - mean rounds once (1 + e1), d * d rounds once more on a product of two such factors: d^2 carries
    3 roundings; the tree adds non-negative terms, (k - 1) + 8 roundings relative to the sum itself; the division
    rounds once; the square root rounds once, which is two in its square: (k + 13) u relative to
    sum (x - mean)^2 / n, and that sum is V + (mean - mu)^2 exactly (the cross term vanishes about the exact mean mu).
    With |mean - mu| <= delta: |std^2 - V| <= 2 (k + 14) u V + delta^2.  (std^2 is formed exactly, as a rational.)

    A constant region has d = 0 in every voxel when S / n returns the constant, so std == 0.0 exactly; the cases use
    a constant whose sums are exact in float64."""
    k = -(-n // LANES)
    delta = 2 * (k + 9) * U * abs_sum / n
    return delta, 2 * (k + 14) * U * var + delta * delta


def ratios(mean, std, values):
    """|error| / bar of one segment's mean and variance against the reference (0 where error and bar are both 0)."""
    ref = reference(values)
    b_mean, b_var = bars(len(values), ref.abs_sum, ref.var)
    e_mean = abs(Fraction(float(mean)) - ref.mean)
    e_var = abs(Fraction(float(std)) ** 2 - ref.var)
    ratio = lambda e, b: 0.0 if e == 0 else (math.inf if b == 0 else float(e / b))  # noqa: E731
    return ratio(e_mean, b_mean), ratio(e_var, b_var), ref


def bits_equal(got, want):
    """float64 arrays equal bit for bit, any NaN equal to any NaN."""
    g, w = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    if g.shape != w.shape or not np.array_equal(np.isnan(g), np.isnan(w)):
        return False
    ok = ~np.isnan(w)
    return np.array_equal(g[ok].view(np.uint64), w[ok].view(np.uint64))


# ---- cases ----------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    """A flat volume (1, 1, n): `map` float32 and `roi` int32 of n voxels.  `finite`: every segment is finite, the
    reference applies.  `ragged`: it has segments whose last group of 256 is ragged and that the mutations must trip on."""
    name: str
    map: np.ndarray
    roi: np.ndarray
    n_labels: int
    finite: bool = True
    ragged: bool = False

    @property
    def shape(self):
        return (1, 1, len(self.map))


def _wide(rng, n):
    """float32 values over 48 binades: their float64 sums round, so the bits of a sum depend on the order."""
    return (rng.normal(0.0, 1.0, n) * np.exp2(rng.uniform(-24.0, 24.0, n))).astype(np.float32)


def _clustered(rng, n):
    """A grid of 0.25 with many exact ties, some negatives, a tenth at exactly 100."""
    m = np.round(rng.normal(120.0, 25.0, n) * 4.0) / 4.0
    m = np.where(rng.random(n) < 0.05, -m, m)
    return np.where(rng.random(n) < 0.1, 100.0, m).astype(np.float32)


SIZES = (1, 63, 64, 65, SPAN - 1, SPAN, SPAN + 1, 4 * SPAN + 1, 5 * SPAN - 1, 257 * SPAN - 5)


def size_case(n, last="own"):
    """Labels 1..5 scattered over n voxels, label 1 also on the two voxels either side of every unit boundary
    (multiples of 8192); label 6 has one voxel, the last (`last="own"`).  Where the last unit holds that voxel alone
    (n = 8193, 4 * 8192 + 1) label 1 cannot also sit behind the last boundary: `last="straddle"` gives the last voxel
    to label 1 and leaves label 6 empty.  Label 1: N(120, 25); 2: a grid with ties; 3: 48 binades; 4: 48 binades, a
    tenth NaN; 5: the constant 87.5.  Background voxels hold huge values, infinities and NaN that nobody may read."""
    rng = np.random.default_rng(1000 + n % 99991 + (7 if last == "straddle" else 0))
    p0 = 0.3 if n <= 5 * SPAN else 0.75  # the 257-unit volume: a quarter labelled, so that the host reference stays quick
    roi = rng.choice(6, size=n, p=[p0] + [(1.0 - p0) / 5] * 5).astype(np.int32)
    for b in range(SPAN, n, SPAN):
        roi[b - 2: b + 2] = 1
    roi[n - 1] = 6 if last == "own" else 1
    m = _wide(rng, n)
    m[roi == 0] = rng.choice(np.array([1e30, -3e38, np.inf, -np.inf, np.nan, 0.0], np.float32), int(np.sum(roi == 0)))
    m[roi == 1] = rng.normal(120.0, 25.0, int(np.sum(roi == 1))).astype(np.float32)
    m[roi == 2] = _clustered(rng, int(np.sum(roi == 2)))
    four = np.flatnonzero(roi == 4)
    m[four[rng.random(len(four)) < 0.1]] = np.nan
    m[roi == 5] = 87.5
    m[n - 1] = 33.25
    for b in range(SPAN, n, SPAN):
        assert roi[b - 1] == 1 and (roi[b] == 1 or (b == n - 1 and last == "own"))
    assert (np.sum(roi == 6) == 1 and roi[n - 1] == 6) if last == "own" else not np.any(roi == 6)
    return Case(f"size-{n}" + ("-straddle" if last == "straddle" else ""), m, roi, 6)


def size_cases():
    out = []
    for n in SIZES:
        out.append(size_case(n))
        if n > 1 and (n - 1) % SPAN == 0:
            out.append(size_case(n, "straddle"))
    return out


_PART_BYTES = (0xC2, 0x48, 0x80, 0x10)  # key bytes from the top: 0xC2 is the float's 0x42, values of 32 .. 128


def parting_values(rng, p, n, by_sign=False):
    """n float32 values, shuffled, whose lower half (n // 2 values) has key byte p = A and whose upper half has A + 1; the
    bytes above are shared, the bytes below random.  `by_sign` (p = 0): A = 0x7f, the negative floats next to zero, and
    A + 1 = 0x80, the positive ones -- denormals and the smallest normals."""
    a = 0x7F if by_sign else _PART_BYTES[p]
    assert not by_sign or p == 0
    keys = np.zeros(n, np.uint64)
    for byte in range(4):
        if byte < p:
            col = np.full(n, _PART_BYTES[byte])
        elif byte == p:
            col = np.where(np.arange(n) < n // 2, a, a + 1)
        else:
            col = rng.integers(0, 256, n)
        keys = (keys << np.uint64(8)) | col.astype(np.uint64)
    vals = key_float(rng.permutation(keys).astype(np.uint32))
    assert np.all(np.isfinite(vals))
    k = np.sort(float_key(vals))
    lo, hi = int(k[(n - 1) // 2]), int(k[n // 2])
    if n % 2 == 0:  # the two middle values first differ in byte p
        assert lo != hi and (lo ^ hi) >> (32 - 8 * p) == 0 and (lo ^ hi) >> (24 - 8 * p) != 0
    else:
        assert lo == hi
    return vals


def _scattered(rng, segments, background=0.2, n_labels=None, name="", **kw):
    """The segments (one float32 array per label, in order) scattered over one volume among background voxels; every
    label's values keep their order."""
    labels = np.concatenate([np.full(len(v), i + 1, np.int32) for i, v in enumerate(segments)])
    n_bg = int(background * len(labels)) + 1
    roi = rng.permutation(np.concatenate([labels, np.zeros(n_bg, np.int32)])).astype(np.int32)
    m = np.full(len(roi), np.nan, np.float32)
    for i, v in enumerate(segments):
        m[roi == i + 1] = v
    return Case(name, m, roi, n_labels or len(segments), **kw)


def parting_cases():
    """Per pass p one volume: label 1 has 1000 values, label 2 has 1001 (the base loop of the median runs four times
    with both ranks alive).  Pass 0 adds labels 3 and 4, parted by sign; pass 3 adds label 3, 1000 values whose two
    middle values are equal."""
    out = []
    for p in range(4):
        rng = np.random.default_rng(2000 + p)
        segs = [parting_values(rng, p, 1000), parting_values(rng, p, 1001)]
        if p == 0:
            segs += [parting_values(rng, 0, 1000, True), parting_values(rng, 0, 1001, True)]
        if p == 3:
            v = np.float32(77.125)
            eq = np.concatenate([v - rng.uniform(0.5, 40.0, 499), [v, v], v + rng.uniform(0.5, 40.0, 499)]).astype(np.float32)
            k = np.sort(float_key(eq))
            assert k[499] == k[500] and k[498] < k[499] < k[501]
            segs.append(rng.permutation(eq))
        out.append(_scattered(rng, segs, name=f"parting-pass-{p}"))
    return out


def tree_case():
    """Three segments of 300 values (a ragged second row of 44) on which a changed tree shows.  Label 1: 1.0 followed
    by 299 times 2^-54, a quarter of its ulp -- added one at a time to 1.0 they all vanish, the halving adds them up
    among themselves first.  Label 2: 10000 + N(0, 0.01): E[x^2] - mean^2 cancels eight digits.  Label 3: 48 binades."""
    rng = np.random.default_rng(3000)
    a = np.full(300, 2.0 ** -54, np.float32)
    a[0] = 1.0
    b = (10000.0 + rng.normal(0.0, 0.01, 300)).astype(np.float32)
    segs = [a, b, _wide(rng, 300)]
    labels = np.concatenate([np.full(300, i + 1, np.int32) for i in range(3)])  # one after the other: element 0 stays first
    return Case("tree-300", np.concatenate(segs), labels, 3, ragged=True)


def nonfinite_case():
    """Label 1: one +inf among 8 finite values; 2: both infinities among 9; 3: [-inf, +inf]; 4: [+inf]."""
    rng = np.random.default_rng(4000)
    f = lambda n: rng.normal(50.0, 9.0, n).astype(np.float32)  # noqa: E731
    segs = [rng.permutation(np.append(f(8), np.float32(np.inf))),
            rng.permutation(np.append(f(9), np.float32([np.inf, -np.inf]))),
            np.float32([-np.inf, np.inf]), np.float32([np.inf])]
    return _scattered(rng, segs, name="non-finite", finite=False)


def edge_value_case():
    """Label 1: float32 denormals only; 2: +-float32 max among others; 3: all negative; 4: [-0.0, 0.0, 0.0];
    5: [-0.0, -0.0]."""
    rng = np.random.default_rng(4001)
    den = (rng.integers(1, 1 << 23, 40).astype(np.uint32)).view(np.float32)  # exponent field 0
    den[:5] = [F32_DENORM, F32_DENORM, 3 * F32_DENORM, -F32_DENORM, np.float32(1.1754942e-38)]
    assert np.all(np.abs(den) < np.finfo(np.float32).tiny) and np.all(den != 0)
    big = rng.permutation(np.concatenate([[F32_MAX, -F32_MAX, F32_MAX], rng.normal(0, 1e30, 6).astype(np.float32)])).astype(np.float32)
    neg = -np.abs(_clustered(rng, 37)) - np.float32(0.5)
    segs = [den, big, neg, np.float32([-0.0, 0.0, 0.0]), np.float32([-0.0, -0.0])]
    return _scattered(rng, segs, name="edge-values")


def label_cases():
    """int32 volumes that hold -1, n_labels + 1, INT32_MIN and INT32_MAX among valid labels: n_labels = 1, and
    n_labels = 256 with label 256 populated (and 255, 1, 2)."""
    out = []
    for n_labels, n in ((1, 1000), (256, 3000)):
        rng = np.random.default_rng(5000 + n_labels)
        valid = [1] if n_labels == 1 else [1, 2, 128, 255, 256]
        pool = np.array(valid + [0, -1, n_labels + 1, INT32_MIN, INT32_MAX, 65536 + valid[-1]], np.int64)
        roi = rng.choice(pool, n).astype(np.int32)
        roi[:len(pool)] = pool
        out.append(Case(f"labels-{n_labels}", _wide(rng, n), roi, n_labels))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(size_cases() + parting_cases() + [tree_case(), nonfinite_case(), edge_value_case()] + label_cases())


def case(name):
    return next(c for c in all_cases() if c.name == name)


_EXPECTED = {}


def expected(c):
    """The statement of a case, computed once and shared (treat it as read-only)."""
    if c.name not in _EXPECTED:
        _EXPECTED[c.name] = statement(c.map, c.roi, c.n_labels)
    return _EXPECTED[c.name]
