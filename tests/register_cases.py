"""Inputs shared by tests/test_register_host.py and tests/test_register_gpu.py: seeded, built once per process; and
:func:`reference_sums`, the 43 sums restated from their definition in extended precision, which neither the kernel nor
the numpy statement was written from."""
import functools
import math

import numpy as np

from fetal_t2mapping_amd import _resample as R


def rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    m = {0: [[1, 0, 0], [0, c, -s], [0, s, c]], 1: [[c, 0, s], [0, 1, 0], [-s, 0, c]], 2: [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis]
    return np.array(m, np.float64)


OBLIQUE = rot(2, 9.0) @ rot(0, -6.0)


def rigid(angles_deg, shift, centre=(0.0, 0.0, 0.0)):
    """4 x 4: rotations about x, y, z [degrees] composed as Rx Ry Rz about `centre`, then the shift [mm]."""
    t = np.eye(4)
    t[:3, :3] = rot(0, angles_deg[0]) @ rot(1, angles_deg[1]) @ rot(2, angles_deg[2])
    c = np.asarray(centre, np.float64)
    t[:3, 3] = c - t[:3, :3] @ c + np.asarray(shift, np.float64)
    return t


def gaussians(geom, centres, sigmas, amps):
    """A sum of Gaussians at physical `centres` [mm] sampled on the grid `geom`, float32."""
    m, o = R._index_to_point(geom)
    nz, ny, nx = geom.shape
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    pts = np.stack([ix, iy, iz], -1).astype(np.float64) @ m.T + o
    v = np.zeros(geom.shape)
    for c, s, a in zip(centres, sigmas, amps):
        v += a * np.exp(-np.sum((pts - np.asarray(c, np.float64)) ** 2, -1) / (2.0 * s * s))
    return v.astype(np.float32)


@functools.lru_cache(maxsize=None)
def smooth_pair():
    """A smooth 20 x 24 x 28 fixed and 22 x 21 x 30 moving volume (Z, Y, X) on oblique grids, slightly apart."""
    fg = R.Geometry((28, 24, 20), (1.0, 1.1, 1.2), (-13.0, -12.0, -11.0), OBLIQUE.ravel())
    mg = R.Geometry((30, 21, 22), (0.9, 1.2, 1.0), (-12.5, -11.5, -10.0), (rot(1, 4.0) @ OBLIQUE).ravel())
    centres = [(0, 0, 0), (5, -3, 2), (-4, 4, -3), (2, 5, 4)]
    sigmas, amps = [6.0, 4.0, 5.0, 3.5], [800, 600, -300, 500]
    fixed = gaussians(fg, centres, sigmas, amps)
    moving = gaussians(mg, [np.array(c) + (0.7, -0.4, 0.5) for c in centres], sigmas, amps)
    return fixed, fg, moving, mg


RECOVERY_TRUE = rigid((4.0, 3.0, -5.0), (2.5, -1.5, 2.0))


@functools.lru_cache(maxsize=None)
def recovery_pair():
    """A 32 x 40 x 48 blob phantom and its resample through RECOVERY_TRUE (so that fixed(x) = moving(T x)):
    ``(fixed, moving, geometry, fixed mask, moving mask)``."""
    from fetal_t2mapping_amd import _register as G

    shape = (32, 40, 48)
    g = R.Geometry(shape[::-1], (1, 1, 1), tuple(-(np.array(shape[::-1]) - 1) / 2.0))
    rng = np.random.default_rng(5)
    n = 7
    centres = rng.uniform(-0.28, 0.28, (n, 3)) * np.array(shape[::-1])
    fixed = gaussians(g, centres, rng.uniform(3, 6, n), rng.uniform(300, 900, n))
    moving = R.resample(fixed, R.index_affine(g, g, np.linalg.inv(RECOVERY_TRUE)), g.shape)
    return fixed, moving, g, G.build_mask(fixed), G.build_mask(moving)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- the named cases of the 43 sums ----------------------------------------------------------------------------------
def _centred(shape, spacing, direction):
    """A grid of ``shape`` (Z, Y, X) whose middle is the physical origin."""
    size = shape[::-1]
    m = np.asarray(direction, np.float64).reshape(3, 3) * np.asarray(spacing, np.float64)[None, :]
    return R.Geometry(size, spacing, tuple(-m @ ((np.array(size) - 1) / 2.0)), np.asarray(direction).ravel())


def _random_case(seed, fshape, mshape, a, fdensity=0.8, mdensity=0.9):
    rng = np.random.default_rng(seed)
    fixed = rng.normal(400, 120, fshape).astype(np.float32)
    moving = rng.normal(400, 120, mshape).astype(np.float32)
    fmask = (rng.random(fshape) < fdensity).astype(np.uint8)
    mmask = (rng.random(mshape) < mdensity).astype(np.uint8)
    return fixed, moving, a, fmask, mmask


def _centred_case(seed, fshape, mshape, angles=(3.0, -2.0, 4.0), shift=(0.4, -0.7, 0.3), along_y=0.0, **kw):
    """Both grids centred on the origin (thin or tiny volumes overlap), oblique, slightly turned and shifted; ``along_y``
    [mm] more shift along the fixed grid's y axis."""
    fg = _centred(fshape, (1.0, 1.1, 1.2), OBLIQUE)
    mg = _centred(mshape, (1.1, 1.0, 0.9), rot(1, 4.0) @ OBLIQUE)
    shift = np.asarray(shift, np.float64) + along_y * OBLIQUE[:, 1]
    return _random_case(seed, fshape, mshape, R.index_affine(fg, mg, rigid(angles, shift)), **kw)


# non-finite moving nodes (z, y, x) of the "integer" cases
NON_FINITE_NODES = ((4, 5, 6, np.inf), (8, 3, 9, np.nan), (5, 8, 4, -np.inf), (9, 9, 11, np.nan))
INTEGER_SHIFT = (2.0, 1.0, 3.0)  # x, y, z


def _integer_case(eps):
    """A translation by whole voxels (every interpolation weight is exactly 0) onto a moving volume that holds Inf and
    NaN in nodes whose mask byte is 0.  A node's value reaches a voxel at ``c`` only through a zero weight if the node is
    not the lower node of ``c`` -- except in the gradient along an axis, which at a whole ``c`` is the forward difference
    and so by definition reads the upper neighbour along that axis.  The three lower face neighbours of a non-finite node
    are therefore masked out too; its 4 lower edge and corner neighbours and all its upper neighbours count, and for them
    the zero-weight rule must keep the node out of every sum.  ``eps`` moves the translation off the nodes: the weights
    are then tiny and not 0, and the sums that read the nodes are not finite."""
    fshape, mshape = (10, 9, 12), (13, 12, 15)
    a = np.eye(3, 4)
    a[:, 3] = np.array(INTEGER_SHIFT) + eps
    fixed, moving, _, fmask, mmask = _random_case(37, fshape, mshape, a, fdensity=0.9, mdensity=1.1)
    for z, y, x, v in NON_FINITE_NODES:
        moving[z, y, x] = v
        mmask[z, y, x] = mmask[z - 1, y, x] = mmask[z, y - 1, x] = mmask[z, y, x - 1] = 0
    return fixed, moving, a, fmask, mmask


def _thin_moving_case(axis):
    """The "prime" pair with the moving volume one voxel thick along ``axis`` (0 = x); the row of A that maps to it is
    shrunk to 1 % with an offset of 0.1, so that the image of the fixed volume stays inside [-0.5, 0.5) there."""
    fshape, mshape = (19, 23, 37), [21, 18, 41]
    mshape[2 - axis] = 1
    fixed, moving, a, fmask, mmask = _centred_case(41 + axis, fshape, tuple(mshape))
    a = a.copy()
    a[axis] *= 0.01
    a[axis, 3] = 0.1
    return fixed, moving, a, fmask, mmask


def _three_pass_case():
    """(2035, 1034, 3): 255 x 259 x 1 = 66045 slabs, passes [66045, 258, 2].  The fixed grid is ten times as fine as the
    moving one, so a small moving volume covers it; the fixed mask is sparse (0.3 %) to keep the reference quick."""
    fshape, mshape = (2035, 1034, 3), (212, 112, 5)
    fg = _centred(fshape, (0.1, 0.1, 0.1), np.eye(3))
    mg = _centred(mshape, (0.1, 1.0, 1.0), np.eye(3))
    a = R.index_affine(fg, mg, rigid((0.4, 0.02, -0.02), (0.01, 0.3, -0.2)))
    rng = np.random.default_rng(43)
    fixed = rng.normal(400, 120, fshape).astype(np.float32)
    moving = rng.normal(400, 120, mshape).astype(np.float32)
    fmask = (rng.random(fshape, np.float32) < 0.003).astype(np.uint8)
    fmask[:8, :4], fmask[-3:, -2:] = 1, 1  # the first and the last brick
    mmask = (rng.random(mshape) < 0.9).astype(np.uint8)
    return fixed, moving, a, fmask, mmask


def _capped_case(seed, fshape):
    """A fixed volume thin in x with more bricks than the joint histogram launches workgroups, under a moving volume that
    covers it with a margin of one to two voxels and is slightly turned.  Both are measured in millimetres: the moving
    grid of ``_centred_case`` has voxels of 0.9 mm against 1.2 mm along z and stands 4 degrees about y to the fixed one,
    so the moving volume has more voxels along z and y, and the transform turns by 4 degrees about y and a twentieth of a
    degree more about every axis.  A turn of whole degrees would carry the ends of a volume three voxels wide outside,
    and the late bricks (the high z) would hold no voxel that counts."""
    mshape = (int(np.ceil(fshape[0] * 1.2 / 0.9)) + 2, int(np.ceil(fshape[1] * 1.1 / 1.0)) + 3, 5)
    return _centred_case(seed, fshape, mshape, angles=(0.05, 4.02, -0.04), shift=(0.2, -0.3, 0.1))


def _thinned(out, seed, density=0.04):
    """A case with its fixed mask thinned to ``density``, the first and the last brick left as they are (as in
    "three_pass"): for a reference that is a Python loop per voxel."""
    fixed, moving, a, fmask, mmask = out
    thin = fmask * (np.random.default_rng(seed).random(fmask.shape) < density).astype(np.uint8)
    z, y = (fmask.shape[0] - 1) // 8 * 8, (fmask.shape[1] - 1) // 4 * 4  # where the last brick of 64 x 4 x 8 begins (nx <= 64)
    thin[:8, :4], thin[z:, y:] = fmask[:8, :4], fmask[z:, y:]
    return fixed, moving, a, thin, mmask


@functools.lru_cache(maxsize=None)
def case(name):
    """(fixed, moving, A, fixed mask, moving mask) of a named case; the arrays are shared and must not be written."""
    if name in ("prime", "bricks", "empty_bricks", "outside", "nothing"):
        rng = np.random.default_rng(31)
        fshape, mshape = ((40, 48, 70), (37, 50, 66)) if name == "bricks" else ((19, 23, 37), (21, 18, 41))
        fg = R.Geometry(fshape[::-1], (1.0, 1.1, 1.2), tuple(-0.5 * np.array(fshape[::-1])), OBLIQUE.ravel())
        mg = R.Geometry(mshape[::-1], (1.1, 1.0, 0.9), tuple(-0.5 * np.array(mshape[::-1])), (rot(1, 4.0) @ OBLIQUE).ravel())
        shift = {"outside": (14.0, -9.0, 6.0), "nothing": (400.0, 0.0, 0.0)}.get(name, (0.4, -0.7, 0.3))
        a = R.index_affine(fg, mg, rigid((3.0, -2.0, 4.0), shift))
        fixed = rng.normal(400, 120, fshape).astype(np.float32)
        moving = rng.normal(400, 120, mshape).astype(np.float32)
        fmask = (rng.random(fshape) < 0.8).astype(np.uint8)
        mmask = (rng.random(mshape) < 0.9).astype(np.uint8)
        if name == "empty_bricks":  # whole bricks of 64 x 4 x 8 without a voxel, and a mask that ends inside a brick
            fmask[:8], fmask[:, 4:13], fmask[9:, :, 30:] = 0, 0, 0
        out = fixed, moving, a, fmask, mmask
    # two passes: thin fixed volumes, the moving one pushed along them so that the low end lies outside (many voxels do
    # not count) and the high end, whose slabs fill the ragged last group of the first pass, inside
    elif name == "tail774":  # 3 x 258 x 1 slabs: passes [774, 4], the last group of the first pass holds 6 values
        out = _centred_case(33, (19, 1030, 5), (26, 700, 9), angles=(0.3, -0.2, 0.25), along_y=-215.0)
    elif name == "tail257":  # 1 x 257 x 1 slabs: passes [257, 2], the last group of the first pass holds one value
        out = _centred_case(34, (5, 1027, 7), (9, 640, 11), angles=(0.3, -0.2, 0.25), along_y=-270.0)
    elif name == "three_pass":
        out = _three_pass_case()
    # more bricks than the joint histogram's 2048 workgroups: a workgroup walks several before it flushes its table
    elif name == "capped2":  # 9 x 258 x 1 = 2322 bricks: 274 workgroups take a second one
        out = _capped_case(44, (65, 1030, 3))
    elif name == "capped5":  # 33 x 258 x 1 = 8514 bricks: every workgroup takes four, 322 a fifth; past twice the cap too
        out = _capped_case(45, (257, 1030, 3))
    elif name == "capped2_thin":
        out = _thinned(case("capped2"), 46)
    elif name in ("moving_x1", "moving_y1", "moving_z1"):
        out = _thin_moving_case("xyz".index(name[7]))
    elif name == "fixed_1x1x1":
        a = np.eye(3, 4)
        a[:, 3] = (0.3, 1.4, 0.7)
        out = _random_case(35, (1, 1, 1), (3, 3, 3), a, fdensity=1.1, mdensity=1.1)
    elif name == "fixed_3x2x5":
        out = _centred_case(36, (3, 2, 5), (4, 4, 6), fdensity=1.1, mdensity=1.1)
    elif name == "fixed_9x6x65":  # a second brick in x with a single lane, a second in y and in z
        out = _centred_case(38, (9, 6, 65), (10, 7, 80))
    elif name == "fixed_8x4x64":  # one exact brick
        out = _centred_case(39, (8, 4, 64), (10, 7, 80))
    elif name == "integer":
        out = _integer_case(0.0)
    elif name == "integer_eps":
        out = _integer_case(2.0 ** -40)
    elif name == "half_rim":  # c = i - 0.5: the first voxel of every axis lies on -0.5 (inside), the last on n - 0.5 (outside)
        a = np.eye(3, 4)
        a[:, 3] = -0.5
        out = _random_case(40, (6, 7, 9), (5, 6, 8), a)
    else:
        raise KeyError(name)
    return out


@functools.lru_cache(maxsize=None)
def statement_sums(name):
    """The numpy statement's 43 sums of a named case, computed once per process."""
    from fetal_t2mapping_amd import _register as G

    fixed, moving, a, fmask, mmask = case(name)
    return G.registration_sums(fixed, moving, a, fmask, mmask)


@functools.lru_cache(maxsize=None)
def reference(name):
    """:func:`reference_sums` of a named case, computed once per process."""
    fixed, moving, a, fmask, mmask = case(name)
    return reference_sums(fixed, moving, a, fmask, mmask)


TWO_PASS = ("tail774", "tail257")
DEGENERATE = ("moving_x1", "moving_y1", "moving_z1", "fixed_1x1x1", "fixed_3x2x5", "fixed_9x6x65", "fixed_8x4x64", "integer",
              "half_rim")
REFERENCE_CASES = ("prime", "bricks", "empty_bricks", "outside") + TWO_PASS + DEGENERATE


# What the sums may differ by from :func:`reference_sums`, relative to the sum of a sum's absolute terms.  The numpy
# statement's largest ratio over REFERENCE_CASES is 4.6e-16 (tests/test_register_host.py has the figures); the bar is 16
# times that.  The device is bit-equal to the statement today; this is how far it may drift if that is ever given up.
STATEMENT_RATIO = 4.6e-16
TOL = 16 * STATEMENT_RATIO


def reference_ratio(sums, name):
    """The largest ``|s - ref| / scale`` over the 43 sums of a named case (a sum without terms must be exactly 0), after
    asserting what holds whatever the tolerance: the count is exact and one voxel more or less cannot hide."""
    ref, scale = reference(name)
    assert sums[0] == ref[0] and TOL * ref[0] < 0.1, (name, sums[0], ref[0])
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(sums)), name
    assert np.array_equal(sums[scale == 0], ref[scale == 0]), name
    return float(np.max(np.abs(sums - ref)[scale > 0] / scale[scale > 0], initial=0.0))


def assert_within_reference(sums, name):
    ref, scale = reference(name)
    ratio = reference_ratio(sums, name)
    print(f"{name}: N {ref[0]:.0f}, largest |s - ref| / scale {ratio:.3g}")
    bad = np.flatnonzero(~(np.abs(sums - ref) <= TOL * scale))
    assert bad.size == 0, (name, bad, sums[bad], ref[bad], scale[bad])


# ---- the 43 sums from their definition -------------------------------------------------------------------------------
def counted_voxels(fixed_shape, moving_shape, A, fixed_mask, moving_mask):
    """``(iz, iy, ix, c)``: the indices of the fixed voxels that count and their float64 coordinates ``c[k]`` (k = 0 is
    x): the fixed mask is set, ``c`` lies in ``[-0.5, n - 0.5)`` on every axis, the nearest moving-mask node is set."""
    a = np.asarray(A, np.float64).reshape(3, 4)
    n = tuple(moving_shape)[::-1]
    iz, iy, ix = np.nonzero(np.asarray(fixed_mask))
    full = R._coords(a, tuple(fixed_shape))
    c = [ck[iz, iy, ix] for ck in full]
    keep = np.ones(iz.shape, bool)
    for k in range(3):
        keep &= (c[k] >= -0.5) & (c[k] < n[k] - 0.5)
    iz, iy, ix, c = iz[keep], iy[keep], ix[keep], [ck[keep] for ck in c]
    near = [np.clip(np.floor(c[k] + 0.5), 0, n[k] - 1).astype(np.int64) for k in range(3)]
    keep = np.asarray(moving_mask)[near[2], near[1], near[0]] != 0
    return iz[keep], iy[keep], ix[keep], [ck[keep] for ck in c]


@functools.lru_cache(maxsize=None)
def counted_per_slab(name):
    """int64 ``[n_slabs]``: how many voxels count in every brick of a named case, bricks in ``(bz, by, bx)`` order."""
    from fetal_t2mapping_amd import _register as G

    fixed, moving, a, fmask, mmask = case(name)
    iz, iy, ix, _ = counted_voxels(fixed.shape, moving.shape, a, fmask, mmask)
    nbz, nby, nbx = G.brick_counts(fixed.shape)
    return np.bincount(((iz // G.BZ) * nby + iy // G.BY) * nbx + ix // G.BX, minlength=nbz * nby * nbx)


def _exact_sum(terms):
    """The sum of extended-precision terms, exact before its one rounding to float64: every term is split into two
    float64 and math.fsum adds them all.  Non-finite terms: a plain sum (which sums are finite is all that is asked)."""
    hi = terms.astype(np.float64)
    if not np.all(np.isfinite(hi)):
        with np.errstate(all="ignore"):
            return float(np.sum(hi))
    lo = (terms - hi).astype(np.float64)
    return math.fsum(hi.tolist() + lo.tolist())


def reference_sums(fixed, moving, A, fixed_mask=None, moving_mask=None):
    """``(sums, scale)``, float64 ``[43]`` each: the sums of include/t2fit.h from the definition, and for each the sum of
    its absolute terms.  Only the voxels that count are gathered; their coordinates are the resampler's float64 ones
    (part of the definition); everything after is ``np.longdouble``.  The moving volume is edge-padded by one voxel and
    the coordinate clamped to ``[0, n - 1]``; the value is the eight-tap form ``sum wx wy wz v``; the gradient along an
    axis is its derivative (-1 / +1 in place of that axis' two weights), 0 where ``c < 0`` or ``c >= n - 1``.  A tap
    whose weight is exactly 0 adds nothing, whatever it holds.  Each sum is exact up to its last rounding."""
    ld = np.longdouble
    fixed, moving = np.asarray(fixed, np.float32), np.asarray(moving, np.float32)
    fmask = np.ones(fixed.shape, np.uint8) if fixed_mask is None else np.asarray(fixed_mask)
    mmask = np.ones(moving.shape, np.uint8) if moving_mask is None else np.asarray(moving_mask)
    n = moving.shape[::-1]
    iz, iy, ix, c = counted_voxels(fixed.shape, moving.shape, A, fmask, mmask)
    padded = np.pad(moving, 1, mode="edge").astype(ld)
    lo, w, dw = [], [], []
    for k in range(3):
        cc = np.clip(c[k], 0.0, float(n[k] - 1))
        base = np.floor(cc)
        t = cc.astype(ld) - base.astype(ld)
        lo.append(base.astype(np.int64) + 1)  # the index into the padded volume
        w.append((ld(1) - t, t))
        flat = (c[k] < 0.0) | (c[k] >= n[k] - 1)
        dw.append((np.where(flat, ld(0), ld(-1)), np.where(flat, ld(0), ld(1))))
    m = np.zeros(iz.shape, ld)
    g = [np.zeros(iz.shape, ld) for _ in range(3)]
    with np.errstate(all="ignore"):
        for tz in (0, 1):
            for ty in (0, 1):
                for tx in (0, 1):
                    v = padded[lo[2] + tz, lo[1] + ty, lo[0] + tx]
                    for acc, wx, wy, wz in ((m, w[0][tx], w[1][ty], w[2][tz]), (g[0], dw[0][tx], w[1][ty], w[2][tz]),
                                            (g[1], w[0][tx], dw[1][ty], w[2][tz]), (g[2], w[0][tx], w[1][ty], dw[2][tz])):
                        weight = wx * wy * wz
                        acc += np.where(weight == 0, ld(0), weight * v)
        f = fixed[iz, iy, ix].astype(ld)
        u = (ix.astype(ld), iy.astype(ld), iz.astype(ld), np.ones(iz.shape, ld))
        terms = [np.ones(iz.shape, ld), f, m, f * f, m * m, f * m]
        for wv in (None, f, m):
            for k in range(3):
                wg = g[k] if wv is None else wv * g[k]
                terms += [wg * u[j] for j in range(4)]
        sums, scale = np.zeros(43), np.zeros(43)
        for q, t in enumerate(terms):
            sums[q], scale[q] = _exact_sum(t), _exact_sum(np.abs(t))
    return sums, scale


# ---- pyramid levels --------------------------------------------------------------------------------------------------
PYRAMID_FACTORS = (1, 3, 5, 32)


@functools.lru_cache(maxsize=None)
def pyramid_case(s):
    """``(volume, mask)`` whose sizes leave a remainder on every axis at shrink factor ``s``; the mask's density gives
    level masks with zeros and ones."""
    rng = np.random.default_rng(50 + s)
    shape = (33, 40, 70) if s == 32 else (19, 23, 37)
    v = rng.normal(300, 80, shape).astype(np.float32)
    m = (rng.random(shape) < {1: 0.3, 3: 0.03, 5: 0.006, 32: 0.001}[s]).astype(np.uint8)
    if s == 32:  # two blocks: the second one empty, and voxels set in the ragged edge that no block holds
        m[:32, :32, 32:64] = 0
        m[32:, 32:, 64:] = 1
    return v, m


def ordered(a):
    """float32 -> int64 that counts units in the last place: the difference of two is their distance in ulps."""
    i = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


@functools.lru_cache(maxsize=None)
def block_means(s):
    """float32 ``level_shape``: the mean of every whole ``s^3`` block of ``pyramid_case(s)``'s volume, summed exactly
    (math.fsum), divided in float64 and rounded to float32 -- the correctly rounded mean unless the float64 quotient
    falls within its own last place of a float32 tie."""
    v, _ = pyramid_case(s)
    nz, ny, nx = (n // s for n in v.shape)
    b = v[:nz * s, :ny * s, :nx * s].astype(np.float64).reshape(nz, s, ny, s, nx, s).transpose(0, 2, 4, 1, 3, 5)
    b = b.reshape(nz * ny * nx, s ** 3)
    return np.array([math.fsum(row) / float(s ** 3) for row in b.tolist()]).astype(np.float32).reshape(nz, ny, nx)
