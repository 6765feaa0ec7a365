"""Named cases of the N4 bias-field steps and an INDEPENDENT reference written from the definition, not
from the kernels or the numpy statement: the B-spline fit is the point-by-point scatter of the MBA paper over the voxels
of M with exact rational weights and extended-precision sums, the field is the 64-tap tensor sum, the histogram is a
Python loop over Python integers.  Shared by tests/test_bias_host.py and tests/test_bias_gpu.py."""
import contextlib
import functools
import math
from fractions import Fraction

import numpy as np

from fetal_t2mapping_amd import _bias

LD = np.longdouble

# the smallest shapes that reach every branch of the kernels (z, y, x)
SHAPES = [(5, 6, 1),      # nx = 1
          (3, 2, 5),      # tiny volume
          (19, 23, 37),   # general small volume
          (7, 5, 64),     # nx = 64 exactly: one full group of lanes
          (7, 5, 65),     # nx = 65: a ragged second group of one term
          (2, 3, 257),    # five terms per lane, ragged
          (40, 48, 70)]   # general, more than 256 rows (two groups of the tree over the rows)
SIDES = _bias.SIDES

# |statement - reference| <= TOL * sum |terms| for delta, omega, the field and the convergence sums.  16 times the largest
# ratio the statement shows over SHAPES x SIDES and both masks (test_bias_host.py prints every case's): 6.72e-14, omega's
# twin 4.46e-14, both on the one-voxel mask of (40, 48, 70), where a node's sum is one term.  That is not the sums' error
# (the field's and the convergence sums' ratios stay below 2e-15) but the weights': p = i s / (n - 1) is rounded to float64
# before k is taken off, so tau carries an absolute error of about 1e-16 p, and a small tau (1 / 69 here) enters b3 cubed
# and a and q at up to the sixth power.  The reference takes tau as an exact fraction.
MEASURED_RATIO = 6.72e-14
TOL = 16 * MEASURED_RATIO


@functools.lru_cache(maxsize=None)
def case(shape, kind="rows"):
    """(volume float32 with some voxels <= 0, input mask uint8, lattice-independent extras).  ``kind='rows'``: a random
    mask that empties whole rows; ``'one'``: a mask of one voxel."""
    rng = np.random.default_rng(sum(shape) * 7919 + len(kind))
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    vol = (200.0 + 100.0 * rng.random(shape)) * np.exp(0.3 * np.sin(0.2 * x + 0.3 * y) + 0.02 * z)
    vol[rng.random(shape) < 0.05] = 0.0
    vol[rng.random(shape) < 0.02] = -3.0
    vol = vol.astype(np.float32)
    if kind == "one":
        mask = np.zeros(shape, np.uint8)
        mask[nz // 2, ny // 2, nx // 2] = 1
        vol[nz // 2, ny // 2, nx // 2] = 123.0
    else:
        mask = (rng.random(shape) < 0.8).astype(np.uint8)
        mask[(z + y) % 3 == 0] = 0          # whole rows empty
        mask[nz - 1, ny - 1, :] = 1         # .. and the last row, with the last voxel of a ragged group, full
        vol[nz - 1, ny - 1, :] = np.abs(vol[nz - 1, ny - 1, :]) + 1.0
    for a in (vol, mask):
        a.setflags(write=False)
    return vol, mask


# The min/max and histogram kernels stride over the voxels with at most kMaxGrid = 1024 workgroups of 256 threads, sized
# for 8 voxels per thread (csrc/t2fit_n4.hip: stride_grid).  Past 1024 x 2048 voxels the grid stops growing, a thread
# makes a ninth trip, and the final kernel reads all 1024 partials.
CAPPED_GRID_VOXELS = 1024 * 2048
CAPPED_N = CAPPED_GRID_VOXELS + 2049


@functools.lru_cache(maxsize=None)
def capped_case():
    """``(u, M)`` of a flat volume of CAPPED_N voxels, as ``log_image`` makes them from a volume with some voxels <= 0 and a
    mask of about 1 %: the smallest and the largest value inside M, and the last voxel, lie past CAPPED_GRID_VOXELS, where
    only a ninth trip of the kernels' loops reads them."""
    n = CAPPED_N
    rng = np.random.default_rng(n)
    vol = (200.0 + 100.0 * rng.random(n)).astype(np.float32)
    vol[rng.random(n) < 0.05] = 0.0
    mask = (rng.random(n) < 0.01).astype(np.uint8)
    vol[CAPPED_GRID_VOXELS + 7], vol[n - 1] = 150.0, 350.0
    mask[CAPPED_GRID_VOXELS + 7], mask[n - 1] = 1, 1
    u, m = _bias.log_image(vol.reshape(1, 1, n), mask.reshape(1, 1, n))
    for a in (u, m):
        a.setflags(write=False)
    return u, m


@functools.lru_cache(maxsize=None)
def check_capped():
    """The conditions on :func:`capped_case`, with numpy alone; returns ``(lo, hi, slope)`` of the statement."""
    u, m = capped_case()
    inside = np.flatnonzero(m.ravel())
    values = u.ravel()[inside]
    assert u.shape == (1, 1, CAPPED_N) and -(-CAPPED_N // 2048) > 1024 and 15000 < inside.size < 25000
    assert inside[-1] == CAPPED_N - 1 and np.count_nonzero(inside >= CAPPED_GRID_VOXELS) >= 10
    lo, hi = _bias.minmax(u, m)
    for extreme in (lo, hi):  # one voxel holds it, in the tail
        at = inside[values == extreme]
        assert at.size == 1 and at[0] >= CAPPED_GRID_VOXELS
    assert (lo, hi) == (np.float32(np.log(150.0)), np.float32(np.log(350.0))) and np.all(u.ravel()[m.ravel() == 0] == 0)
    return lo, hi, _bias.slope_of(lo, hi)


def lattice_of(side, seed=0):
    return np.random.default_rng(1000 + side + seed).normal(0.0, 0.1, (side,) * 3)


def old_field(shape):
    return np.random.default_rng(sum(shape)).normal(0.0, 0.05, shape).astype(np.float32)


# ---- the independent reference -------------------------------------------------------------------------------------------
def ref_axis(n, c):
    """k[n] and the four exact B-spline weights (Fractions) of every voxel index along an axis."""
    s = c - 3
    ks, ws = [], []
    for i in range(n):
        if n == 1:
            k, tau = 0, Fraction(0)
        elif i == n - 1:
            k, tau = s - 1, Fraction(1)
        else:
            p = Fraction(i * s, n - 1)
            k = math.floor(p)
            tau = p - k
        ks.append(k)
        ws.append(((1 - tau) ** 3 / 6, (3 * tau ** 3 - 6 * tau ** 2 + 4) / 6, (-3 * tau ** 3 + 3 * tau ** 2 + 3 * tau + 1) / 6,
                   tau ** 3 / 6))
    return np.array(ks), ws


def _ld(fr):
    return LD(fr.numerator) / LD(fr.denominator)


def _axis_ld(n, c):
    k, ws = ref_axis(n, c)
    return k, np.array([[_ld(w) for w in row] for row in ws], LD)


def ref_fit(values, m, c):
    """The MBA sums by point-by-point scatter: every voxel of M spreads ``w^3 v / sum w^2`` and ``w^2`` over its 64 nodes,
    ``w = bz by bx``.  Returns (delta, sum |delta terms|, omega) as longdouble ``[c, c, c]``."""
    zi, yi, xi = np.nonzero(np.asarray(m) != 0)
    (kz, bz), (ky, by), (kx, bx) = (_axis_ld(n, c) for n in np.shape(m))
    v = np.asarray(values).astype(LD)[zi, yi, xi]
    wz, wy, wx = bz[zi], by[yi], bx[xi]                                  # [N, 4]
    w = wz[:, :, None, None] * wy[:, None, :, None] * wx[:, None, None, :]   # [N, 4, 4, 4]
    ssq = (w * w).sum(axis=(1, 2, 3))
    delta, mag, omega = (np.zeros(c ** 3, LD) for _ in range(3))
    for i in range(4):
        for j in range(4):
            for k in range(4):
                node = ((kz[zi] + i) * c + (ky[yi] + j)) * c + (kx[xi] + k)
                wn = w[:, i, j, k]
                term = wn * wn * wn * v / ssq
                np.add.at(delta, node, term)
                np.add.at(mag, node, np.abs(term))
                np.add.at(omega, node, wn * wn)
    return tuple(a.reshape(c, c, c) for a in (delta, mag, omega))


def ref_field(lattice, shape):
    """The 64-tap tensor sum at every voxel, and the sum of the taps' magnitudes (longdouble)."""
    lat = np.asarray(lattice).astype(LD)
    c = lat.shape[0]
    (kz, bz), (ky, by), (kx, bx) = (_axis_ld(n, c) for n in shape)
    f, mag = np.zeros(shape, LD), np.zeros(shape, LD)
    for i in range(4):
        for j in range(4):
            for k in range(4):
                tap = (bz[:, i, None, None] * by[None, :, j, None] * bx[None, None, :, k]
                       * lat[(kz + i)[:, None, None], (ky + j)[None, :, None], (kx + k)[None, None, :]])
                f += tap
                mag += np.abs(tap)
    return f, mag


def ref_histogram(u, m, lo, slope, bins):
    """Python integers, a Python loop: the definition voxel by voxel."""
    hist = [0] * bins
    lo, slope = float(lo), float(slope)
    for uv in np.asarray(u)[np.asarray(m) != 0].tolist():
        c = (uv - lo) / slope          # (a float32 is exact as a Python float; these are IEEE float64 operations)
        c = min(max(c, 0.0), bins - 1.0)
        i = min(math.floor(c), bins - 2)
        w = math.floor((c - i) * 2 ** 24 + 0.5)
        hist[i] += 2 ** 24 - w
        hist[i + 1] += w
    return hist


# ---- the statement against the reference -----------------------------------------------------------------------------------
def ratio(got, ref, mag):
    """max |got - ref| / sum |terms| over the entries with terms."""
    got, ref, mag = (np.asarray(a, LD).ravel() for a in (got, ref, mag))
    err = np.abs(got - ref)
    assert np.all(err[mag == 0] == 0), "a value without terms is not zero"
    return float(np.max(err[mag > 0] / mag[mag > 0])) if np.any(mag > 0) else 0.0


def setup(shape, kind="rows"):
    """(u0, M, lo, slope, table) of a case by the statement: what the fit takes."""
    vol, mask = case(shape, kind)
    u0, m = _bias.log_image(vol, mask)
    lo, hi = _bias.minmax(u0, m)
    if hi > lo:
        slope = _bias.slope_of(lo, hi)
        table = _bias.sharpen_table(_bias.histogram(u0, m, lo, slope), lo, slope, 0.15)
    else:  # one voxel: no range, no table; the fit takes u itself
        slope, table = 1.0, None
    return u0, m, float(lo), slope, table


def statement_ratios(shape, side, kind="rows"):
    """The statement's error ratios of a case against the reference: {name: ratio}; asserts the histogram exactly."""
    u0, m, lo, slope, table = setup(shape, kind)
    if table is not None:
        assert [int(h) for h in _bias.histogram(u0, m, lo, slope)] == ref_histogram(u0, m, lo, slope, _bias.BINS)
    r = _bias.residual(u0, m, table, lo, slope)
    delta, mag, omega = ref_fit(r, m, side)
    out = {"delta": ratio(_bias.fit_delta(u0, m, side, table, lo, slope), delta, mag),
           "omega": ratio(_bias.fit_weights(m, side), omega, omega)}
    lat = lattice_of(side)
    f, fmag = ref_field(lat, shape)
    got = _bias.field_eval(lat, shape)
    got64 = _bias.field_eval(lat, shape, store=np.float64)  # the sum before its one rounding to float32
    assert np.array_equal(got, got64.astype(np.float32))
    out["field"] = ratio(got64, f, fmag)
    d = _bias.convergence_terms(got, old_field(shape), m)
    sd, sdd = _bias.convergence_sums(got, old_field(shape), m)
    out["sum_d"] = ratio([sd], [math.fsum(d.ravel())], [math.fsum(np.abs(d).ravel())])
    out["sum_dd"] = ratio([sdd], [math.fsum((d * d).ravel())], [math.fsum((d * d).ravel())])
    return out


def check_statement(shape, side, kind="rows"):
    ratios = statement_ratios(shape, side, kind)
    for name, value in ratios.items():
        assert value <= TOL, (name, value, shape, side)
    return ratios


def check_cannot_hide(shape, side):
    """TOL times a node's omega is smaller than half of any single voxel's largest term there: a dropped or doubled voxel
    cannot pass the bar."""
    _, m, _, _, _ = setup(shape)
    _, _, omega = ref_fit(np.ones(shape), m, side)
    zi, yi, xi = np.nonzero(m)
    (kz, bz), (ky, by), (kx, bx) = (_axis_ld(n, side) for n in shape)
    jz, jy, jx = bz[zi].argmax(axis=1), by[yi].argmax(axis=1), bx[xi].argmax(axis=1)
    term = (bz[zi, jz] * by[yi, jy] * bx[xi, jx]) ** 2
    at = omega[kz[zi] + jz, ky[yi] + jy, kx[xi] + jx]
    assert np.all(LD(TOL) * at < term / 2)


# ---- mutations of the statement: each must fail check_statement ------------------------------------------------------------
def _axis_without_last_rule(n, c):
    s = c - 3
    p = np.arange(n, dtype=np.float64) * s / max(n - 1, 1)
    k = np.floor(p)
    b = _bias.bspline(p - k)
    q = b * b
    ssq = ((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3]
    return k.astype(np.int64), b, (q * b) / ssq[:, None], q


_axis = _bias.axis_weights
_tree = _bias.row_tree
_coords = _bias.bin_coords


def _axis_swapped(n, c):
    k, b, a, q = _axis(n, c)
    return k, b, q, a


def _tree_without_ragged_group(terms):
    nx = np.shape(terms)[-1]
    full = nx // _bias.LANES * _bias.LANES
    return _tree(np.asarray(terms)[..., :full] if 0 < full < nx else terms)


def _coords_top_bin_of_its_own(u, lo, slope, bins=_bias.BINS):
    c = (np.asarray(u).astype(np.float64) - float(lo)) / float(slope)
    c = np.minimum(np.maximum(c, 0.0), bins - 1.0)
    i = np.floor(c)
    return i.astype(np.int64), c - i


# name: (the attribute of _bias, the mutated function).  The first and the last put a weight of zero one node past the
# lattice / the table: in numpy that is an IndexError, which fails the check as an assertion does.
MUTATIONS = {"last_voxel_rule_dropped": ("axis_weights", _axis_without_last_rule),
             "a_and_q_swapped": ("axis_weights", _axis_swapped),
             "ragged_last_group_dropped": ("row_tree", _tree_without_ragged_group),
             "top_bin_of_its_own": ("bin_coords", _coords_top_bin_of_its_own)}


@contextlib.contextmanager
def mutated(name):
    attr, fn = MUTATIONS[name]
    saved = getattr(_bias, attr)
    setattr(_bias, attr, fn)
    try:
        yield
    finally:
        setattr(_bias, attr, saved)


# ---- the recovery phantom --------------------------------------------------------------------------------------------------
RECOVERY_SHAPE = (32, 40, 48)


@functools.lru_cache(maxsize=None)
def recovery_phantom(shape=RECOVERY_SHAPE, seed=7):
    """A three-class ball times exp of a smooth polynomial field, plus noise: (volume, mask, classes, true log field)."""
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.linspace(-1, 1, nz), np.linspace(-1, 1, ny), np.linspace(-1, 1, nx), indexing="ij")
    r = np.sqrt(z * z + y * y + x * x)
    cls = np.zeros(shape, np.int32)
    cls[r < 0.9] = 1
    cls[r < 0.65] = 2
    cls[r < 0.4] = 3
    truth = np.array([0.0, 300.0, 600.0, 1000.0])[cls]
    logf = 0.25 * x - 0.2 * y * y + 0.15 * z * x + 0.1 * z
    vol = truth * np.exp(logf) + np.random.default_rng(seed).normal(0.0, 5.0, shape)
    vol = np.where(cls > 0, np.maximum(vol, 1.0), 0.0).astype(np.float32)
    return vol, (cls > 0).astype(np.uint8), cls, logf


def class_cv(vol, cls, label=3):
    s = np.asarray(vol)[cls == label].astype(np.float64)
    return float(s.std() / s.mean())


def field_correlation(log_field, true, mask):
    sel = np.asarray(mask) != 0
    return float(np.corrcoef(np.asarray(log_field).astype(np.float64)[sel], true[sel])[0, 1])


# Measured with the statement on the CPU, full defaults at fwhm = 0.15: iterations (37, 11, 3, 3),
# 1 - corr = 4.36e-4, CV of the brightest class 0.0493 -> 0.00507.  The bars: CV after <= 2 x measured and <= half the
# input's; 1 - corr <= 10 x measured.
RECOVERY_CV_AFTER = 0.00507
RECOVERY_ONE_MINUS_CORR = 4.36e-4


def check_recovery(corrected, log_field):
    vol, mask, cls, logf = recovery_phantom()
    before, after = class_cv(vol, cls), class_cv(corrected, cls)
    miss = 1.0 - field_correlation(log_field, logf, mask)
    print(f"recovery: CV {before:.4f} -> {after:.5f}, 1 - corr {miss:.3e}")
    assert after <= 2 * RECOVERY_CV_AFTER and after <= before / 2
    assert miss <= 10 * RECOVERY_ONE_MINUS_CORR
    return before, after, miss


# ---- three thick-slice stacks that each carry their own field (recon.py --n4) ----------------------------------------------
def recon_phantom(side=32, thick=4, te_ms=(114, 255, 299), seed=11):
    """The three-class ball on a 1 mm cube, decaying over three echoes, sampled into ax / cor / sag stacks of `thick` mm
    slices; every stack is multiplied by a smooth field of its own (the same at every echo) and gets noise.  Returns
    ``(stacks {o: float32 (n_te, slices, y, x)}, geoms, classes on the cube)``."""
    from fetal_t2mapping_amd import _resample as R

    ax_d, cor_d, sag_d = np.eye(3), np.array([[1, 0, 0], [0, 0, 1], [0, 1, 0.0]]), np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0.0]])
    lin = np.linspace(-1, 1, side)
    z, y, x = np.meshgrid(lin, lin, lin, indexing="ij")
    r = np.sqrt(z * z + y * y + x * x)
    cls = np.zeros((side,) * 3, np.int32)
    cls[r < 0.9] = 1
    cls[r < 0.65] = 2
    cls[r < 0.4] = 3
    t2 = np.array([1.0, 120.0, 200.0, 400.0])[cls]
    truth = np.stack([np.array([0.0, 300.0, 600.0, 1000.0])[cls] * np.exp(-te / t2) for te in te_ms])
    n_sl = side // thick
    origin = -(side - 1) / 2.0
    off = origin + (thick - 1) / 2.0
    geoms = {"ax": R.Geometry((side, side, n_sl), (1, 1, thick), (origin, origin, off), ax_d.ravel()),
             "cor": R.Geometry((side, side, n_sl), (1, 1, thick), (origin, off, origin), cor_d.ravel()),
             "sag": R.Geometry((side, side, n_sl), (1, 1, thick), (off, origin, origin), sag_d.ravel())}
    n = len(te_ms)
    clean = {"ax": truth.reshape(n, n_sl, thick, side, side).mean(2),
             "cor": truth.reshape(n, side, n_sl, thick, side).mean(3).transpose(0, 2, 1, 3),
             "sag": truth.reshape(n, side, side, n_sl, thick).mean(4).transpose(0, 3, 1, 2)}
    rng = np.random.default_rng(seed)
    stacks = {}
    for k, o in enumerate(("ax", "cor", "sag")):
        s, v, u = np.meshgrid(np.linspace(-1, 1, n_sl), lin, lin, indexing="ij")  # (slice, stack y, stack x)
        field = np.exp((0.35, -0.3, 0.25)[k] * u + (0.2, 0.3, -0.35)[k] * v - 0.15 * u * v + (0.1, -0.1, 0.15)[k] * s)
        vol = clean[o] * field + rng.normal(0.0, 3.0, clean[o].shape)
        stacks[o] = np.where(clean[o] > 0, np.maximum(vol, 1.0), 0.0).astype(np.float32)
    return stacks, geoms, cls


def write_recon_subject(tmp_path, stacks, geoms, te_ms=(114, 255, 299)):
    """The stacks as NIfTI files under <prj>/<sub>/<ses>/anat and the metadata rows."""
    import pandas as pd

    from fetal_t2mapping_amd import cli, nifti

    bids = str(tmp_path / "projects") + "/"
    rows, run = [], 0
    for i, te in enumerate(te_ms):
        for o in ("ax", "cor", "sag"):
            run += 1
            acq = {"prj": "prj-900", "sub": "sub-001", "ses": "ses-01", "run": f"run-{run:02d}", "EchoTime": te / 1000.0,
                   "CoilString": "HeadNeck", "ImageOrientationPatientSTR": o}
            rows.append(acq)
            g = geoms[o]
            nifti.WriteImage(nifti.Image(stacks[o][i], g.GetSpacing(), g.GetOrigin(), g.GetDirection()),
                             cli.get_img_path(bids, acq, "anat"))
    return bids, pd.DataFrame(rows)


def recon_cv(merged, cls, label=3):
    """CV of a class on the merged 1 mm volume of :func:`recon_phantom`.  The ax stack's 1 mm grid starts at the centre of
    the first 4 mm slice, 1.5 mm into the cube: a merged voxel k lies between the cube's k + 1 and k + 2, and counts when
    both are of the class."""
    core = (cls[1:-1] == label) & (cls[2:] == label)
    s = np.asarray(merged)[:core.shape[0]][core].astype(np.float64)
    return float(s.std() / s.mean())


# ---- the C ABI: the workspace's arithmetic and every refusal ----------------------------------------------------------------
def expected_bytes(nz, ny, nx, c):
    def up(v):
        return -(-v // 256) * 256

    rows, axis = nz * ny, nz + ny + nx
    total = up(4 * axis) + up(96 * axis) + up(8 * rows * c) + up(8 * nz * c * c) + 2 * up(4 * max(rows, 1024))
    n = rows
    while True:
        total += up(16 * n)
        if n <= 256:
            return total
        n = -(-n // 256)


A, ODD4, ODD8, ODD256 = 0x10000, 0x10002, 0x10004, 0x10010  # made-up addresses: a refused call touches none of them
B, D, E, F, G = 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
BIG = 1 << 30


def refusals():
    """(function name, arguments, a word of the message): each call has one thing wrong."""
    s = None  # the stream
    out = []
    out += [("t2fit_n4_log_dev", a, w) for a, w in (
        ((None, None, 10, B, D, s), "NULL"), ((A, None, 10, None, D, s), "NULL"), ((A, None, 10, B, None, s), "NULL"),
        ((A, None, 0, B, D, s), "n_vox"), ((A, None, 1 << 39, B, D, s), "n_vox"), ((ODD4, None, 10, B, D, s), "aligned"),
        ((A, None, 10, ODD4, D, s), "aligned"), ((A, None, 10, A, D, s), "must not"))]
    out += [("t2fit_n4_minmax_dev", a, w) for a, w in (
        ((None, B, 10, D, E, BIG, s), "NULL"), ((A, None, 10, D, E, BIG, s), "NULL"), ((A, B, 10, None, E, BIG, s), "NULL"),
        ((A, B, 0, D, E, BIG, s), "n_vox"), ((ODD4, B, 10, D, E, BIG, s), "aligned"), ((A, B, 10, ODD4, E, BIG, s), "aligned"),
        ((A, B, 10, D, None, BIG, s), "workspace_dev is NULL"), ((A, B, 10, D, ODD256, BIG, s), "256"),
        ((A, B, 10, D, E, 8191, s), "too small"))]
    out += [("t2fit_n4_histogram_dev", a, w) for a, w in (
        ((None, B, 10, 0.0, 1.0, 200, D, s), "NULL"), ((A, None, 10, 0.0, 1.0, 200, D, s), "NULL"),
        ((A, B, 10, 0.0, 1.0, 200, None, s), "NULL"), ((A, B, 0, 0.0, 1.0, 200, D, s), "n_vox"),
        ((A, B, 10, 0.0, 1.0, 1, D, s), "bins"), ((A, B, 10, 0.0, 1.0, 1025, D, s), "bins"),
        ((A, B, 10, float("nan"), 1.0, 200, D, s), "lo / slope"), ((A, B, 10, 0.0, 0.0, 200, D, s), "lo / slope"),
        ((A, B, 10, 0.0, float("inf"), 200, D, s), "lo / slope"), ((ODD4, B, 10, 0.0, 1.0, 200, D, s), "aligned to 4"),
        ((A, B, 10, 0.0, 1.0, 200, ODD8, s), "aligned to 8"))]
    out += [("t2fit_n4_weights_dev", a, w) for a, w in (
        ((None, 4, 5, 6, 4, B, E, BIG, s), "NULL"), ((A, 4, 5, 6, 4, None, E, BIG, s), "NULL"), ((A, 0, 5, 6, 4, B, E, BIG, s), "sizes"),
        ((A, 4, 5, 6, 6, B, E, BIG, s), "side"), ((A, 4, 5, 6, 4, ODD8, E, BIG, s), "aligned to 8"),
        ((A, 4, 5, 6, 4, B, None, BIG, s), "workspace_dev is NULL"), ((A, 4, 5, 6, 4, B, ODD256, BIG, s), "256"),
        ((A, 4, 5, 6, 4, B, E, expected_bytes(4, 5, 6, 4) - 1, s), "too small"))]
    fit = (A, B, 4, 5, 6, D, 0.0, 1.0, 200, 4, E, F, G, 0x70000, BIG, s)

    def put(args, at, value):
        return args[:at] + (value,) + args[at + 1:]

    out += [("t2fit_n4_fit_dev", a, w) for a, w in (
        (put(fit, 0, None), "NULL"), (put(fit, 1, None), "NULL"), (put(fit, 10, None), "NULL"), (put(fit, 11, None), "NULL"),
        (put(fit, 12, None), "NULL"), (put(fit, 3, 0), "sizes"), (put(fit, 9, 8), "side"), (put(fit, 8, 1), "bins"),
        (put(fit, 7, -1.0), "lo / slope"), (put(fit, 6, float("inf")), "lo / slope"), (put(fit, 0, ODD4), "aligned to 4"),
        (put(fit, 5, ODD8), "aligned to 8"), (put(fit, 10, ODD8), "aligned to 8"), (put(fit, 11, ODD8), "aligned to 8"),
        (put(fit, 12, ODD8), "aligned to 8"), (put(fit, 12, F), "three arrays"), (put(fit, 11, E), "three arrays"),
        (put(fit, 13, None), "workspace_dev is NULL"), (put(fit, 13, ODD256), "256"),
        (put(fit, 14, expected_bytes(4, 5, 6, 4) - 1), "too small"))]
    fld = (A, 4, B, D, 4, 5, 6, E, F, G, 0x70000, 0x80000, BIG, s)
    out += [("t2fit_n4_field_dev", a, w) for a, w in (
        (put(fld, 0, None), "NULL"), (put(fld, 2, None), "NULL"), (put(fld, 3, None), "NULL"), (put(fld, 7, None), "NULL"),
        (put(fld, 8, None), "NULL"), (put(fld, 9, None), "NULL"), (put(fld, 10, None), "NULL"), (put(fld, 1, 9), "side"),
        (put(fld, 6, 0), "sizes"), (put(fld, 2, ODD4), "aligned to 4"), (put(fld, 7, ODD4), "aligned to 4"),
        (put(fld, 8, ODD4), "aligned to 4"), (put(fld, 10, ODD4), "aligned to 4"), (put(fld, 0, ODD8), "aligned to 8"),
        (put(fld, 9, ODD8), "aligned to 8"), (put(fld, 8, E), "three arrays"), (put(fld, 7, B), "three arrays"),
        (put(fld, 8, B), "three arrays"), (put(fld, 11, None), "workspace_dev is NULL"), (put(fld, 11, ODD256), "256"),
        (put(fld, 12, 100), "too small"))]
    out += [("t2fit_n4_apply_dev", a, w) for a, w in (
        ((None, B, 10, 1.0, D, s), "NULL"), ((A, None, 10, 1.0, D, s), "NULL"), ((A, B, 10, 1.0, None, s), "NULL"),
        ((A, B, 0, 1.0, D, s), "n_vox"), ((A, B, 10, float("nan"), D, s), "scale"), ((ODD4, B, 10, 1.0, D, s), "aligned"),
        ((A, ODD4, 10, 1.0, D, s), "aligned"), ((A, B, 10, 1.0, ODD4, s), "aligned"), ((A, B, 10, 1.0, B, s), "must not"))]
    return out
