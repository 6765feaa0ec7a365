"""Named cases of the mask-building stage, shared by tests/test_morph_host.py and tests/test_morph_gpu.py.

1. Balanced inputs.  A dilation or an erosion is only compared where about half of the voxels change: the dilation input
   is a random point set of density 0.7 / |S^n| (S^n: the element dilated by itself n times, what n iterations reach), the
   erosion input the complement of one, so that exp(-0.7) ~ 1 / 2 of the voxels stay clear of every point.  The helper
   asserts on scipy's result alone that ones and zeros both make up MIN_SHARE of the voxels, except in *thin* cases (S^n
   longer than half the volume along an axis: the border decides most of the result), which are compared all the same.
2. Every run offset.  One 65 x 65 x 65 footprint holds each of the 2145 runs -32 <= x0 <= x1 <= 32 in a (dz, dy) row of its
   own; its response to isolated ones is pasted together from the definition, with neither scipy nor the statement.
3. A model of the hole filling's tile sweeps, from the description of the design (8 x 8 rows by 256 voxels, Jacobi sweeps
   over tiles that each grow to their own fixed point), which also counts the sweeps.
4. Mutations of the statement that the balanced inputs catch."""
import contextlib
import functools
import itertools

import numpy as np
from scipy import ndimage as ndi

from fetal_t2mapping_amd import _morph as M

SEED = 7
MIN_SHARE = 0.10      # of the voxels, for ones and for zeros, in scipy's result of every case that is not thin
MAX_THIN_SHARE = 0.25  # of a general shape's cases


def two_runs():
    fp = np.zeros((3, 5, 9), bool)  # not convex, not symmetric: two runs in one row, a lone voxel in a corner
    fp[1, 2, 0:3] = True
    fp[1, 2, 6:9] = True
    fp[0, 4, 8] = True
    fp[2, 1, 2:5] = True
    return fp


FOOTPRINTS = {"ball1": M.ball(1), "ball3": M.ball(3), "ball234": M.ball((2, 3, 4)), "box": M.box((1, 2, 3)), "cross1": M.cross(1),
              "cross2": M.cross(2), "cross3": M.cross(3), "two_runs": two_runs(), "flat5x5": np.ones((1, 5, 5), bool)}
ELEMENTS = dict(FOOTPRINTS, wide=M.box((0, 1, 32)))  # rx = 32: the widest run there is

# (z, y, x).  x = 63, 64, 65: one word less a bit, one word, a word and a one-bit tail; 260: four words and a ragged tail,
# and room for the rx = 32 element.  At most a quarter of a general shape's cases may be thin.
GENERAL_SHAPES = [(24, 40, 48), (17, 33, 70), (20, 30, 37), (12, 20, 260), (20, 30, 63), (20, 30, 64), (20, 30, 65)]
FLAT_SHAPES = [(5, 7, 130), (1, 9, 64)]  # a few rows, a single slice: most of their cases are thin, the tails are not


def scipy_passes(op, a, fp, iterations, border):
    """scipy's result for `iterations` >= 1 as that many single passes, which is its definition.  (Its one-call form
    with iterations > 1 overruns the heap when the structure is larger than the volume along an axis, as on the
    single-slice and narrow shapes.)"""
    for _ in range(iterations):
        a = op(a, fp, border_value=border)
    return a


@functools.lru_cache(maxsize=None)
def nfold(name, n):
    """S^n: an impulse dilated n times by the element, with scipy."""
    fp = ELEMENTS[name]
    a = np.zeros(tuple((s // 2) * 2 * n + 1 for s in fp.shape), bool)
    a[tuple(s // 2 for s in a.shape)] = True
    return scipy_passes(ndi.binary_dilation, a, fp, n, 0)


def is_thin(shape, name, n):
    extent = [int(np.ptp(c)) + 1 for c in np.nonzero(nfold(name, n))]
    return any(2 * e > s for e, s in zip(extent, shape))


@functools.lru_cache(maxsize=None)
def balanced(shape, name, n, op):
    """The input of `op` ('dilate' / 'erode') for n iterations of the element: read-only bool (z, y, x)."""
    pts = np.random.default_rng(SEED).random(shape) < 0.7 / int(nfold(name, n).sum())
    a = pts if op == "dilate" else ~pts
    a.setflags(write=False)
    return a


SCIPY_OPS = {"dilate": ndi.binary_dilation, "erode": ndi.binary_erosion}


@functools.lru_cache(maxsize=None)
def expected(shape, name, n, border, op):
    """scipy's result on the balanced input, after the balance assertion (thin cases are exempt from it)."""
    want = scipy_passes(SCIPY_OPS[op], balanced(shape, name, n, op), ELEMENTS[name], n, border)
    share = min(float(want.mean()), 1.0 - float(want.mean()))
    if not is_thin(shape, name, n):
        assert share >= MIN_SHARE, f"unbalanced case {shape} {name} x{n} border {border} {op}: minority share {share:.3f}"
    want.setflags(write=False)
    return want


def minority_share(shape, names, iterations):
    """The smallest minority share over the shape's cases that are not thin (what the summary of a change records)."""
    return min(min(float(w.mean()), 1.0 - float(w.mean()))
               for name, n, border, op in cases(shape, names, iterations) if not is_thin(shape, name, n)
               for w in [expected(shape, name, n, border, op)])


def cases(shape, names, iterations, general=True):
    """[(name, n, border, op)] of a shape; raises when more than a quarter of a general shape's cases are thin."""
    out = list(itertools.product(sorted(names), iterations, (0, 1), ("dilate", "erode")))
    thin = sum(is_thin(shape, name, n) for name, n, _, _ in out)
    if general and thin > MAX_THIN_SHARE * len(out):
        raise ValueError(f"test construction: {thin} of {len(out)} cases of shape {shape} are thin")
    return out


def scipy_close_open(op, a, fp, iterations, border, unbounded):
    """Closing / opening by single scipy passes; unbounded: on the volume padded with zeros by the reach, cropped."""
    first, second = (ndi.binary_dilation, ndi.binary_erosion) if op == "close" else (ndi.binary_erosion, ndi.binary_dilation)
    if not unbounded:
        return scipy_passes(second, scipy_passes(first, a, fp, iterations, border), fp, iterations, border)
    pad = max(s // 2 for s in fp.shape) * iterations
    p = np.pad(a, pad)
    p = scipy_passes(second, scipy_passes(first, p, fp, iterations, 0), fp, iterations, 0)
    return p[tuple(slice(pad, pad + s) for s in a.shape)]


# ---- mutations of the statement ----------------------------------------------------------------------------------------------
_reflect, _dilate_once = M.reflect_runs, M._dilate_once


def _reflect_is_identity(runs):
    return np.asarray(runs, np.int32).reshape(-1, 4)


def _erode_with_its_own_border(a, element, iterations=1, border_value=0):
    a = M._volume(a)
    runs, size = M._as_runs(element)
    back = M.reflect_runs(runs)
    for _ in range(int(iterations)):
        a = ~M._dilate_once(~a, back, size, 1 if border_value else 0)  # the complement's border is 1 - border_value
    return a


def _dilate_once_x_swapped(a, runs, size, border):
    """Reads a[.., x + x0 .. x + x1]: the run walked from the wrong end (x - x0 and x - x1 with the signs lost)."""
    r = np.asarray(runs).reshape(-1, 4)
    return _dilate_once(a, np.stack([r[:, 0], r[:, 1], -r[:, 3], -r[:, 2]], axis=1), size, border)


# name: (the attribute of _morph, the mutated function)
MUTATIONS = {"reflect_runs_is_identity": ("reflect_runs", _reflect_is_identity),
             "erode_passes_border_value": ("erode", _erode_with_its_own_border),
             "dilate_once_x_swapped": ("_dilate_once", _dilate_once_x_swapped)}


@contextlib.contextmanager
def mutated(name):
    attr, fn = MUTATIONS[name]
    saved = getattr(M, attr)
    setattr(M, attr, fn)
    try:
        yield
    finally:
        setattr(M, attr, saved)


# ---- every run offset, by impulse response -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def all_runs_footprint():
    """Row (i // 65, i % 65) holds the i-th of the 2145 runs -32 <= x0 <= x1 <= 32 and nothing else."""
    pairs = [(x0, x1) for x0 in range(-32, 33) for x1 in range(x0, 33)]
    assert len(pairs) == 2145
    fp = np.zeros((65, 65, 65), bool)
    for i, (x0, x1) in enumerate(pairs):
        fp[i // 65, i % 65, x0 + 32:x1 + 33] = True
    fp.setflags(write=False)
    return fp


@functools.lru_cache(maxsize=None)
def all_runs():
    """The same element as (dz, dy, x0, x1) rows, from the pairs and not from footprint_runs."""
    pairs = [(x0, x1) for x0 in range(-32, 33) for x1 in range(x0, 33)]
    return tuple((i // 65 - 32, i % 65 - 32, x0, x1) for i, (x0, x1) in enumerate(pairs))


# name: (shape, the isolated ones as (z, y, x)).  x = 0, 63, 64, 127, 128, nx - 1: both ends of a word and of the row.  dz is
# -32 .. 0, so z = 32 and z = nz - 1 show every row of the element, the smaller z clip it at the low face (the reflected
# element at the high one); y near 0, near ny - 1 and central clips the 65 rows of dy at either face or at both.  Points
# that share z rows keep their x ranges apart, up to a single shared column.
IMPULSES = {"six_points": ((70, 70, 200), ((32, 3, 0), (69, 66, 63), (20, 35, 64), (60, 10, 127), (25, 60, 128), (69, 30, 199))),
            "two_bit_tail": ((40, 70, 130), ((32, 5, 129), (39, 64, 65), (12, 36, 1)))}


@functools.lru_cache(maxsize=None)
def impulse_volume(name):
    shape, points = IMPULSES[name]
    a = np.zeros(shape, bool)
    for p in points:
        a[p] = True
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def pasted(name, reflected=False):
    """The dilation of the points by the element (or by the element reflected through its origin) from the definition:
    every run, shifted to every point and clipped to the volume, pasted into a zero array."""
    (nz, ny, nx), points = IMPULSES[name]
    out = np.zeros((nz, ny, nx), bool)
    for z, y, x in points:
        for dz, dy, x0, x1 in all_runs():
            if reflected:
                dz, dy, x0, x1 = -dz, -dy, -x1, -x0
            if 0 <= z + dz < nz and 0 <= y + dy < ny:
                out[z + dz, y + dy, max(x + x0, 0):max(min(x + x1, nx - 1) + 1, 0)] = True
    out.setflags(write=False)
    return out


def impulse_expected(name, which):
    """'dilate': the points dilated, border 0.  'dual': the complement of the points eroded with border 1.  'erode0': the same
    with border 0, which also takes away every voxel whose footprint leaves the volume."""
    if which == "dilate":
        return pasted(name)
    want = ~pasted(name, reflected=True)  # erode(~a)[v] = no point at any v + s
    if which == "erode0":
        offs = np.array(all_runs())
        lo = (offs[:, 0].min(), offs[:, 1].min(), offs[:, 2].min())
        hi = (offs[:, 0].max(), offs[:, 1].max(), offs[:, 3].max())
        inside = np.zeros(want.shape, bool)
        inside[tuple(slice(max(-l, 0), s - max(h, 0)) for l, h, s in zip(lo, hi, want.shape))] = True
        assert inside.any()
        want = want & inside
    return want


# ---- the hole filling's sweeps -------------------------------------------------------------------------------------------------
TILE = (8, 8, 256)


def sweep_model(a, slice_axis=None):
    """(filled volume, number of sweeps, the last, quiet one included).  A sweep is a Jacobi step over the tiles: every tile
    takes the reached set of the sweep before in its own voxels and in the one-voxel halo around them, and grows it through
    the free voxels of the tile, along the axes the flood may cross, until nothing in the tile changes."""
    a = np.asarray(a) != 0
    free = ~a
    axes = [ax for ax in range(3) if ax != slice_axis]
    structure = np.zeros((3, 3, 3), bool)
    structure[1, 1, 1] = True
    reached = np.zeros(a.shape, bool)
    for ax in axes:
        for k in (0, 2):
            idx = [1, 1, 1]
            idx[ax] = k
            structure[tuple(idx)] = True
        for edge in (0, a.shape[ax] - 1):
            idx = [slice(None)] * 3
            idx[ax] = edge
            reached[tuple(idx)] = free[tuple(idx)]
    boxes = [tuple(slice(o, min(o + t, s)) for o, t, s in zip(origin, TILE, a.shape))
             for origin in itertools.product(*[range(0, s, t) for s, t in zip(a.shape, TILE)])]
    sweeps = 0
    while True:
        new = np.zeros(a.shape, bool)
        for box in boxes:
            seed = reached[box].copy()
            for ax in axes:  # the halo: the voxels one step outside the tile's faces
                for side, outside in ((0, box[ax].start - 1), (-1, box[ax].stop)):
                    if 0 <= outside < a.shape[ax]:
                        src, dst = list(box), [slice(None)] * 3
                        src[ax], dst[ax] = outside, side
                        seed[tuple(dst)] |= reached[tuple(src)]
            seed &= free[box]
            lab, _ = ndi.label(free[box], structure)
            hit = np.unique(lab[seed])
            new[box] = np.isin(lab, hit[hit > 0])
        sweeps += 1
        if np.array_equal(new, reached):
            return ~reached, sweeps
        reached = new


def channel(shape, axis):
    """A solid block with a one-voxel channel along `axis` through its middle: open at the low face, closed one voxel before
    the high face."""
    a = np.ones(shape, bool)
    idx = [s // 2 for s in shape]
    idx[axis] = slice(0, shape[axis] - 1)
    a[tuple(idx)] = False
    return a


# name: (volume, slice_axis, the sweeps the design gives by hand: one per tile along the channel and the quiet one)
CHANNELS = {}
for _n in (32, 40, 48, 56):  # ceil(n / 8) + 1 = 5, 6, 7, 8: the quiet sweep on each of the four places of a batch of four
    CHANNELS[f"y{_n}"] = (channel((3, _n, 3), 1), None, (_n + 7) // 8 + 1)
    CHANNELS[f"z{_n}"] = (channel((_n, 3, 3), 0), None, (_n + 7) // 8 + 1)
CHANNELS["x1280"] = (channel((3, 3, 1280), 2), None, 6)
CHANNELS["y40_in_one_plane"] = (channel((3, 40, 3), 1), 0, 6)


def fill_per_plane(a, axis):
    return np.stack([ndi.binary_fill_holes(np.take(a, i, axis)) for i in range(a.shape[axis])], axis)


def _enclosed_zero(x):
    a = np.ones((3, 3, 130), bool)
    a[1, 1, x] = False
    return a


def _word_run(end):
    """Zeros in words 1 .. 2 (x = 64 .. 191) of a four-word row inside a solid block, with one way in: above its high end
    (the flood runs towards lower x) or above its low end (towards higher x)."""
    a = np.ones((3, 3, 250), bool)
    a[1, 1, 64:192] = False
    a[1, 0, 191 if end == "high" else 64] = False
    return a


DEGENERATE = {"one_voxel_0": np.zeros((1, 1, 1), bool), "one_voxel_1": np.ones((1, 1, 1), bool),
              "nx1": np.random.default_rng(SEED).random((9, 11, 1)) < 0.5,
              "all_ones": np.ones((9, 10, 70), bool), "all_zeros": np.zeros((9, 10, 70), bool),
              "enclosed_zero_x63": _enclosed_zero(63), "enclosed_zero_x64": _enclosed_zero(64),
              "word_run_from_high_end": _word_run("high"), "word_run_from_low_end": _word_run("low")}
