"""Inputs shared by tests/test_ffd_host.py and tests/test_ffd_gpu.py: seeded, built once per process.  The named cases
are register_cases', their bin volumes atlas_cases' and their moving ranges mi_cases'; here are the lattices over them,
the statement's results, the recovery phantom (a known lattice on top of atlas_cases' affine pair) and the refusals of the
raw ABI."""
import ctypes as C
import functools

import numpy as np

import atlas_cases as AC
import mi_cases as MI
import register_cases as K
from fetal_t2mapping_amd import _ffd as F
from fetal_t2mapping_amd import _register as G
from fetal_t2mapping_amd import _resample as R

BIN_PAIRS = ((32, 32), (7, 9), (64, 64), (1, 5))
SIDES = (4, 7, 11, 19)
# The kernels' tile is a row of 64 lanes (x), four rows (y) and one plane (z) per workgroup.  Fixed shapes (Z, Y, X):
# every axis one short of, equal to and one past a tile edge; nx < 64 and nx = 65; the register tests' pair; one with more
# than 256 rows (a second group of the Jacobian's reduction over the rows).
TILE_SHAPES = ((1, 3, 63), (1, 4, 64), (2, 5, 65), (3, 8, 128), (2, 9, 129), (5, 7, 31))
NAMED = ("prime", "outside", "nothing", "empty_bricks", "fixed_1x1x1", "fixed_9x6x65")
MANY_ROWS = (9, 37, 20)  # 333 rows


def lattice(side, seed=0, amplitude=1.5):
    """A seeded lattice of ``side``: uniform in +-``amplitude`` voxels."""
    return np.random.default_rng(1000 + 10 * side + seed).uniform(-amplitude, amplitude, (3, side, side, side))


@functools.lru_cache(maxsize=None)
def named(name, n_f, n_m):
    """``(bins, moving, A, fixed mask, moving mask, lo_m, scale_m)`` of a case of mi_cases."""
    return MI.inputs(name, n_f) + MI.moving_range(name, n_m)


# More tiles than the histogram kernel launches workgroups (mi_cases.HIST_GRID = 2048): a workgroup walks ``tile +=
# gridDim.x``, and as 2048 is no multiple of 17 (or 1) rows of tiles, its next tile lies in another plane and another group
# of rows.  130 x 17 = 2210 tiles whose last one per plane holds a single row; 8840: four trips, five for some; ny = 1:
# three of the four waves idle on every trip.
CAPPED_SHAPES = ((130, 65, 5), (520, 65, 5), (2100, 1, 3))


def tile_index(shape):
    """int64 ``[nz, ny, 1]``: the tile of four rows of one plane every fixed voxel lies in, as the kernels count them."""
    tiles_y = -(-shape[1] // 4)
    return (np.arange(shape[0])[:, None] * tiles_y + np.arange(shape[1])[None, :] // 4)[:, :, None]


@functools.lru_cache(maxsize=None)
def shaped(shape, n_f=32, cover=False):
    """A random case on a fixed grid of ``shape`` against a moving volume two voxels larger, slightly turned: ``(bins,
    moving, A, fixed mask, moving mask)``.  ``cover``: for a long thin grid.  The moving grid's voxels are 0.9 mm against
    1.2 mm along z and it stands 4 degrees about y to the fixed one, so two voxels more and a turn of a degree leave the
    far planes outside; here the moving volume covers the fixed one in millimetres with a margin of one to two voxels, and
    the transform turns by those 4 degrees and a fiftieth of a degree more."""
    mshape, angles = tuple(n + 2 for n in shape), (1.0, -0.8, 1.2)
    if cover:
        mshape = (int(np.ceil(shape[0] * 1.2 / 0.9)) + 2, int(np.ceil(shape[1] * 1.1 / 1.0)) + 3, int(np.ceil(shape[2] * 1.0 / 1.1)) + 3)
        angles = (0.02, 4.01, -0.02)
    _, moving, a, fmask, mmask = K._centred_case(51 + sum(shape), shape, mshape, angles=angles, shift=(0.2, -0.3, 0.1))
    bins = np.random.default_rng(7 + sum(shape)).integers(0, n_f, shape).astype(np.uint8)
    return bins, moving, a, fmask, mmask


@functools.lru_cache(maxsize=None)
def check_capped(shape, side, n_f=7, n_m=9):
    """What makes a capped shape worth running, asserted with the statement alone: more tiles than workgroups, and with the
    fixed mask zeroed in the tiles of the first trip the statement's histogram is neither zero nor the whole one.  Returns
    the number of tiles."""
    bins, moving, a, fmask, mmask = shaped(shape, cover=True)
    lo_m, scale_m = G.moving_bin_range(moving, mmask, n_m)
    phi = lattice(side, 0, 1.2)
    n_tiles = shape[0] * -(-shape[1] // 4)
    assert n_tiles > MI.HIST_GRID
    late = np.where(tile_index(shape) < MI.HIST_GRID, 0, fmask).astype(np.uint8)
    assert 0 < np.count_nonzero(late) < np.count_nonzero(fmask)
    h = F.joint_histogram(bins, moving, a, phi, n_f, n_m, lo_m, scale_m, late, mmask)
    assert h.any() and not np.array_equal(h, F.joint_histogram(bins, moving, a, phi, n_f, n_m, lo_m, scale_m, fmask, mmask))
    return n_tiles


def normal_table(n_f, n_m):
    return np.random.default_rng(97).normal(0.0, 1.0, (n_f, n_m))


# ---- the recovery phantom --------------------------------------------------------------------------------------------------
TRUE_SIDE, TRUE_AMPLITUDE = 5, 3.5


@functools.lru_cache(maxsize=None)
def true_lattice():
    """Side 5, node values in +-3.5 voxels, seeded: a displacement of up to 2.3 voxels (1.2 on average), smooth (a node every
    24 / 20 / 16 voxels) and free of folds (the smallest Jacobian is 0.78)."""
    return np.random.default_rng(2024).uniform(-TRUE_AMPLITUDE, TRUE_AMPLITUDE, (3, TRUE_SIDE, TRUE_SIDE, TRUE_SIDE))


@functools.lru_cache(maxsize=None)
def phantom():
    """``(fixed, moving, geometry, fixed mask, moving mask, atlases on the moving grid, truth on the fixed grid)``:
    atlas_cases' cross-contrast pair (``remap(base)(y) = moving(T y)``, T affine) with the fixed volume deformed,
    ``fixed(x) = base(x + d_true(x))``, so that ``fixed(x)`` matches ``moving(T (x + d_true(x)))``: the model of
    :mod:`_ffd` with a known lattice on top of a known affine.  The label volumes are atlas_cases' balls, carried onto the
    fixed grid through the true map."""
    base, moving, g, _, mmask, = AC.recovery_pair()
    fixed = F.warp(base, np.eye(3, 4), true_lattice(), g.shape)
    _, _, _, _, atlases, _ = AC.atlas_case()
    a_true = R.index_affine(g, g, AC.RECOVERY_TRUE)
    truth = {n: F.warp(v, a_true, true_lattice(), g.shape, interp="nearest", default=0) for n, v in atlases.items()}
    return fixed, moving, g, G.build_mask(fixed, threshold=20), mmask, atlases, truth


@functools.lru_cache(maxsize=None)
def phantom_affine():
    """The affine stage of the existing code on the phantom (Mattes, 12 degrees of freedom): the yardstick."""
    fixed, moving, g, fmask, mmask, _, _ = phantom()
    return G.register_affine(fixed, moving, g, g, metric="mattes", dof=12, fixed_mask=fmask, moving_mask=mmask)


@functools.lru_cache(maxsize=None)
def phantom_ffd():
    """The statement's default ``register_ffd`` from :func:`phantom_affine`, once per process."""
    fixed, moving, g, fmask, mmask, _, _ = phantom()
    return F.register_ffd(fixed, moving, g, g, affine=phantom_affine(), fixed_mask=fmask, moving_mask=mmask)


def map_error(transform, phi):
    """The mean distance [moving voxels = mm] inside the fixed mask between ``c(x)`` of (transform, phi) and the true map."""
    _, _, g, fmask, _, _, _ = phantom()
    found = F.coords(R.index_affine(g, g, transform), phi, g.shape)
    true = F.coords(R.index_affine(g, g, AC.RECOVERY_TRUE), true_lattice(), g.shape)
    d = np.sqrt(sum((np.broadcast_to(f, g.shape) - t) ** 2 for f, t in zip(found, true)))
    return float(d[fmask != 0].mean())


def dices(transform, phi):
    """{(atlas, label): Dice against the truth} of the atlases carried by (transform, phi)."""
    _, _, g, _, _, atlases, truth = phantom()
    a = R.index_affine(g, g, transform)
    out = {}
    for n, lab in atlases.items():
        got = F.warp(lab, a, phi, g.shape, interp="nearest", default=0)
        for value in np.unique(lab[lab != 0]):
            out[n, int(value)] = AC.dice(got, truth[n], value)
    return out


def folding_lattice():
    """Side 4 over a 6 x 6 x 6 grid: the x displacement falls by 4 voxels per voxel of x, so every Jacobian is 1 - 4."""
    phi = np.zeros((3, 4, 4, 4))
    phi[0] = -20.0 * np.arange(4, dtype=np.float64)[None, None, :]  # d_x = -20 (p_x + 1), p_x = x / 5: slope -4
    return phi


# ---- the refusals of the raw ABI -------------------------------------------------------------------------------------------
def check_refusals(lib, bins, table, fmask, moving, mmask, lat, hist, grad, src, out, jac, ws, fshape, mshape, a, side, n_f, n_m, stream):
    """Every refusal include/t2fit.h lists for the five symbols, each T2FIT_E_INVALID with its message and before any
    launch -- so the pointers may be made up (the host test) or real.  ``ws``: a 256-aligned workspace of exactly the
    needed size; ``jac``: 16 bytes (the minimum, then the count)."""
    need, scratch = C.c_size_t(0), C.c_size_t(0)
    assert lib.t2fit_ffd_workspace_bytes(*fshape, side, C.byref(need)) == 0
    A = (C.c_double * 12)(*np.asarray(a, np.float64).ravel())
    inf = (C.c_double * 12)(*np.asarray(a, np.float64).ravel())
    inf[5] = np.inf

    def refused(rc, word):
        err = lib.t2fit_last_error().decode()
        assert rc == -1 and word in err, (rc, word, err)

    def hist_dev(bins=bins, fmask=fmask, fs=fshape, moving=moving, mmask=mmask, ms=mshape, A=A, lat=lat, side=side, n_f=n_f, n_m=n_m,
                 lo=0.0, scale=1.0, hist=hist, ws=ws, nbytes=need.value):
        return lib.t2fit_ffd_joint_hist_dev(bins, fmask, *fs, moving, mmask, *ms, A, lat, side, n_f, n_m, lo, scale, hist, ws, nbytes, stream)

    def grad_dev(bins=bins, table=table, n_f=n_f, n_m=n_m, lo=0.0, scale=1.0, fmask=fmask, fs=fshape, moving=moving, mmask=mmask,
                 ms=mshape, A=A, lat=lat, side=side, grad=grad, ws=ws, nbytes=need.value):
        return lib.t2fit_ffd_gradient_dev(bins, table, n_f, n_m, lo, scale, fmask, *fs, moving, mmask, *ms, A, lat, side, grad, ws, nbytes,
                                          stream)

    def warp_dev(src=src, src_type=0, ms=mshape, A=A, lat=lat, side=side, out=out, fs=fshape, interp=0, default=0.0, ws=ws,
                 nbytes=need.value):
        return lib.t2fit_ffd_warp_dev(src, src_type, *ms, A, lat, side, out, *fs, interp, default, ws, nbytes, stream)

    def jac_dev(lat=lat, side=side, fmask=fmask, fs=fshape, jmin=jac, count=jac + 8, ws=ws, nbytes=need.value):
        return lib.t2fit_ffd_jacobian_dev(lat, side, fmask, *fs, jmin, count, ws, nbytes, stream)

    refused(lib.t2fit_ffd_workspace_bytes(*fshape, side, None), "NULL")
    refused(lib.t2fit_ffd_workspace_bytes(fshape[0], 0, fshape[2], side, C.byref(scratch)), ">= 1")
    for bad in (0, 3, 6, 12, 35):
        refused(lib.t2fit_ffd_workspace_bytes(*fshape, bad, C.byref(scratch)), "side")
        for fn in (hist_dev, grad_dev, warp_dev, jac_dev):
            refused(fn(side=bad), "side")
    common = (({"lat": None}, "NULL"), ({"ws": None}, "NULL"), ({"lat": lat + 4}, "aligned to 8"), ({"ws": ws + 128}, "aligned to 256"),
              ({"nbytes": need.value - 1}, "workspace too small"), ({"fs": (fshape[0], 0, fshape[2])}, ">= 1"))
    sampled = common + (({"A": None}, "NULL"), ({"A": inf}, "non-finite"), ({"ms": (mshape[0], mshape[1], -1)}, "moving sizes"))
    metric = sampled + (({"bins": None}, "NULL"), ({"fmask": None}, "NULL"), ({"moving": None}, "NULL"), ({"mmask": None}, "NULL"),
                        ({"moving": moving + 2}, "aligned to 4"), ({"n_f": 0}, "n_f"), ({"n_f": 65}, "n_f"), ({"n_m": 4}, "n_m"),
                        ({"n_m": 65}, "n_m"), ({"lo": np.nan}, "not finite"), ({"scale": np.inf}, "not finite"))
    for kw, word in metric + (({"hist": None}, "NULL"), ({"hist": hist + 4}, "aligned to 8")):
        refused(hist_dev(**kw), word)
    for kw, word in metric + (({"table": None}, "NULL"), ({"grad": None}, "NULL"), ({"grad": grad + 4}, "aligned to 8"),
                              ({"table": table + 4}, "aligned to 8")):
        refused(grad_dev(**kw), word)
    for kw, word in sampled + (({"src": None}, "NULL"), ({"out": None}, "NULL"), ({"src": src + 2}, "aligned to 4"),
                               ({"out": out + 2}, "aligned to 4"), ({"out": src}, "must not be"), ({"src_type": 2}, "src_type"),
                               ({"interp": 2}, "interp"), ({"src_type": 1, "interp": 0}, "int32 source"),
                               ({"src_type": 1, "interp": 1, "default": 3e9}, "default_value")):
        refused(warp_dev(**kw), word)
    for kw, word in common + (({"fmask": None}, "NULL"), ({"jmin": None}, "NULL"), ({"count": None}, "NULL"),
                              ({"jmin": jac + 4}, "aligned to 8"), ({"count": jac + 12}, "aligned to 8")):
        refused(jac_dev(**kw), word)
