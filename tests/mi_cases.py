"""Inputs shared by tests/test_mi_host.py and tests/test_mi_gpu.py: seeded, built once per process.  The named cases are
register_cases' and the bin volumes over them atlas_cases'; here are the moving ranges, the statement's histograms,
tables and gradient sums, the contention cases, the rigid cross-contrast pair and the refusals of the raw ABI."""
import ctypes as C
import functools

import numpy as np

import atlas_cases as AC
import register_cases as K
from fetal_t2mapping_amd import _register as G
from fetal_t2mapping_amd import _resample as R

BIN_PAIRS = ((1, 5), (7, 9), (32, 32), (64, 64))  # (n_f, n_m): the smallest, two odd ones, the default, the largest
HOST_CASES = ("prime", "bricks", "empty_bricks", "outside", "nothing", "fixed_1x1x1", "fixed_9x6x65", "half_rim", "integer",
              "capped2_thin")  # ("capped2" with a fixed mask of 4 %: the reference is a Python loop per voxel)
GPU_CASES = ("prime", "bricks", "empty_bricks", "outside", "nothing", "fixed_1x1x1", "fixed_8x4x64", "fixed_9x6x65", "half_rim",
             "tail257")
CONTENTION = ("constant", "lanes", "brick")
ONE = 1 << 30  # a weight of 1.0 in the histogram's units
# More bricks than workgroups: the histogram kernel walks ``brick += gridDim.x`` and flushes its table once at the end.
# {name: (bricks along z, y, x)}; 'capped2_constant' is "capped2" with a moving volume of one value (below).
CAPPED = {"capped2": (9, 258, 1), "capped5": (33, 258, 1)}
HIST_GRID = 2048  # kHistGrid of csrc/t2fit_register.hip, and the kHistGrid of csrc/t2fit_ffd.hip over its tiles


@functools.lru_cache(maxsize=None)
def inputs(name, n_f):
    """``(bins, moving, A, fixed mask, moving mask)`` of a named case, a layout case of atlas_cases (64 fixed bins, whatever
    ``n_f``: a byte above n_f - 1 counts as n_f - 1), 'constant' (the "bricks" case with a moving volume of one value) or
    'capped2_constant' (the same on "capped2")."""
    if name in ("lanes", "brick"):
        return AC.layout_case(name)
    if name in ("constant", "capped2_constant"):
        of = "bricks" if name == "constant" else "capped2"
        _, moving, a, fmask, mmask = K.case(of)
        return AC.bins_of(of, n_f), np.full(moving.shape, 417.25, np.float32), a, fmask, mmask
    _, moving, a, fmask, mmask = K.case(name)
    return AC.bins_of(name, n_f), moving, a, fmask, mmask


@functools.lru_cache(maxsize=None)
def moving_range(name, n_m):
    """``(lo_m, scale_m)`` as the host chooses them: over the moving samples inside the moving mask."""
    _, moving, _, _, mmask = inputs(name, 64)
    return G.moving_bin_range(moving, mmask, n_m)  # (the "integer" case keeps its Inf and NaN outside the mask)


@functools.lru_cache(maxsize=None)
def statement_hist(name, n_f, n_m):
    bins, moving, a, fmask, mmask = inputs(name, n_f)
    lo_m, scale_m = moving_range(name, n_m)
    h = G.joint_histogram(bins, moving, a, n_f, n_m, lo_m, scale_m, fmask, mmask)
    h.setflags(write=False)
    return h


def brick_index(shape):
    """int64 ``shape``: the brick every fixed voxel lies in, bricks counted in ``(bz, by, bx)`` order as the kernels do."""
    _, nby, nbx = G.brick_counts(shape)
    iz, iy, ix = np.indices(shape, sparse=True)
    return ((iz // G.BZ) * nby + iy // G.BY) * nbx + ix // G.BX


@functools.lru_cache(maxsize=None)
def counted(name):
    """How many voxels of a named case count (register_cases.counted_voxels: no histogram, no sums)."""
    return int(K.counted_per_slab("capped2" if name == "capped2_constant" else name).sum())


@functools.lru_cache(maxsize=None)
def check_capped(name, n_f=7, n_m=9):
    """What makes a capped case worth running, asserted with the statement alone: it has more bricks than the kernel has
    workgroups, and the bricks a workgroup reaches on its second (for "capped5": also its third) trip change the histogram
    -- with the fixed mask zeroed in the bricks of the first trip(s) the statement's histogram is neither zero nor the
    whole one.  Returns the number of bricks."""
    bins, moving, a, fmask, mmask = inputs(name, n_f)
    lo_m, scale_m = moving_range(name, n_m)
    counts = G.brick_counts(bins.shape)
    n_bricks = int(np.prod(counts))
    assert counts == CAPPED[name] and n_bricks > HIST_GRID, (name, counts)
    whole = statement_hist(name, n_f, n_m)
    brick = brick_index(bins.shape)
    for trips in (1, 2) if name == "capped5" else (1,):
        assert n_bricks > trips * HIST_GRID  # ("capped5" stays past the cap if the cap is doubled)
        late = np.where(brick < trips * HIST_GRID, 0, fmask).astype(np.uint8)
        h = G.joint_histogram(bins, moving, a, n_f, n_m, lo_m, scale_m, late, mmask)
        assert h.any() and not np.array_equal(h, whole), (name, trips)
        assert int(K.counted_per_slab(name)[trips * HIST_GRID:].sum()) > 1000
    return n_bricks


@functools.lru_cache(maxsize=None)
def table(name, n_f, n_m, kind):
    """'normal': seeded normals (every entry takes part); 'metric': what mattes_metric returns for the case's histogram
    (zeros where the histogram is empty)."""
    if kind == "normal":
        return np.random.default_rng(97).normal(0.0, 1.0, (n_f, n_m))
    return G.mattes_metric(statement_hist(name, n_f, n_m), n_f, n_m, moving_range(name, n_m)[1])[1]


@functools.lru_cache(maxsize=None)
def statement_gradient(name, n_f, n_m, kind):
    bins, moving, a, fmask, mmask = inputs(name, n_f)
    lo_m, scale_m = moving_range(name, n_m)
    return G.mi_gradient_sums(bins, table(name, n_f, n_m, kind), moving, a, n_m, lo_m, scale_m, fmask, mmask)


# ---- the rigid cross-contrast pair ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rigid_pair():
    """``(fixed, moving, geometry, fixed mask, moving mask)``: atlas_cases' fixed volume and its remapped copy resampled
    through the rigid register_cases.RECOVERY_TRUE."""
    fixed, _, g, fmask, _ = AC.recovery_pair()
    moving = R.resample(AC.remap(fixed), R.index_affine(g, g, np.linalg.inv(K.RECOVERY_TRUE)), g.shape)
    return fixed, moving, g, fmask, G.build_mask(moving, threshold=20)


def rigid_tre(found):
    fixed, _, g, fmask, _ = rigid_pair()
    return G.target_registration_error(found, K.RECOVERY_TRUE, fmask, g)


@functools.lru_cache(maxsize=None)
def recovered(dof):
    """The statement's mattes registration of atlas_cases' recovery pair, once per process."""
    fixed, moving, g, fmask, mmask = AC.recovery_pair()
    return G.register_affine(fixed, moving, g, g, metric="mattes", dof=dof, fixed_mask=fmask, moving_mask=mmask)


# ---- the refusals of the raw ABI -------------------------------------------------------------------------------------------
def check_refusals(lib, bins, table_ptr, fmask, moving, mmask, hist, sums, ws, fshape, mshape, a, n_f, n_m, stream):
    """Every refusal include/t2fit.h lists for the three symbols, each T2FIT_E_INVALID with its message and before any
    launch -- so the pointers may be made up (the host test) or real (the device test, which then checks that no output
    byte changed).  ``ws``: a 256-aligned workspace of exactly the needed size."""
    need, scratch = C.c_size_t(0), C.c_size_t(0)
    assert lib.t2fit_register_mi_workspace_bytes(*fshape, C.byref(need)) == 0
    A = (C.c_double * 12)(*np.asarray(a, np.float64).ravel())
    inf = (C.c_double * 12)(*np.asarray(a, np.float64).ravel())
    inf[5] = np.inf

    def refused(rc, word):
        err = lib.t2fit_last_error().decode()
        assert rc == -1 and word in err, (rc, word, err)

    def hist_dev(bins=bins, fmask=fmask, fs=fshape, moving=moving, mmask=mmask, ms=mshape, A=A, nf=n_f, nm=n_m, lo=0.0, scale=1.0,
                 hist=hist):
        return lib.t2fit_register_joint_hist_dev(bins, fmask, *fs, moving, mmask, *ms, A, nf, nm, lo, scale, hist, stream)

    def grad_dev(bins=bins, table=table_ptr, nf=n_f, nm=n_m, lo=0.0, scale=1.0, fmask=fmask, fs=fshape, moving=moving, mmask=mmask,
                 ms=mshape, A=A, sums=sums, ws=ws, nbytes=need.value):
        return lib.t2fit_register_mi_gradient_dev(bins, table, nf, nm, lo, scale, fmask, *fs, moving, mmask, *ms, A, sums, ws, nbytes,
                                                  stream)

    refused(lib.t2fit_register_mi_workspace_bytes(*fshape, None), "NULL")
    refused(lib.t2fit_register_mi_workspace_bytes(fshape[0], 0, fshape[2], C.byref(scratch)), ">= 1")
    shared = (({"bins": None}, "NULL"), ({"fmask": None}, "NULL"), ({"moving": None}, "NULL"), ({"mmask": None}, "NULL"),
              ({"A": None}, "NULL"), ({"nf": 0}, "n_f"), ({"nf": 65}, "n_f"), ({"nf": -1}, "n_f"), ({"nm": 4}, "n_m"),
              ({"nm": 65}, "n_m"), ({"nm": 0}, "n_m"), ({"fs": (fshape[0], 0, fshape[2])}, "fixed sizes"),
              ({"fs": (-1, fshape[1], fshape[2])}, "fixed sizes"), ({"ms": (mshape[0], mshape[1], -1)}, "moving sizes"),
              ({"ms": (0, mshape[1], mshape[2])}, "moving sizes"), ({"A": inf}, "non-finite"), ({"lo": np.nan}, "not finite"),
              ({"lo": -np.inf}, "not finite"), ({"scale": np.inf}, "not finite"), ({"scale": np.nan}, "not finite"),
              ({"moving": moving + 2}, "aligned to 4"))
    for kw, word in shared + (({"hist": None}, "NULL"), ({"hist": hist + 4}, "aligned to 8")):
        refused(hist_dev(**kw), word)
    refused(hist_dev(fs=(65536, 65536, 2)), "2^32")  # 2^33 voxels: within the 2^40 of the other sums, too many for uint64 entries
    for kw, word in shared + (({"table": None}, "NULL"), ({"sums": None}, "NULL"), ({"ws": None}, "NULL"), ({"sums": sums + 4}, "aligned to 8"),
                              ({"table": table_ptr + 4}, "aligned to 8"), ({"ws": ws + 128}, "aligned to 256"),
                              ({"nbytes": need.value - 1}, "workspace too small"), ({"nbytes": 0}, "workspace too small")):
        refused(grad_dev(**kw), word)
