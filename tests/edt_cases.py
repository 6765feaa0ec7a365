"""Shared builders of the distance-transform tests (test_edt_host.py, test_edt_drivers_host.py, test_edt_gpu.py): the
shapes, the site patterns, the two named traps of the tie rule, and the statement's results, computed once per case.
Everything is small: no volume exceeds 64 thousand voxels."""
import functools

import numpy as np

from fetal_t2mapping_amd import _edt

UNIT = (1.0, 1.0, 1.0)
DYADIC = ((4.5, 1.0, 1.0), (1.25, 0.5, 0.5))          # every operation of the statement is exact
INEXACT = ((0.8, 1.1, 1.0), (3.3, 0.7, 0.9))          # d2 still equals the brute force; the index may differ at near-ties
EXACT = (UNIT,) + DYADIC
SPACINGS = EXACT + INEXACT
DEVICE_SPACINGS = (UNIT, DYADIC[0], DYADIC[1], INEXACT[0])

# where a row leaves a wave (64), a workgroup (256) and the shared rows of the x pass (256 / nx), where an axis
# degenerates, and one cube
DEVICE_SHAPES = ((1, 1, 1), (1, 1, 65), (65, 1, 1), (1, 65, 1), (3, 130, 67), (70, 5, 129), (2, 3, 600), (2, 600, 3), (600, 2, 3),
                 (40, 40, 40))
DENSITIES = ("half", "sparse", "corner")
SMALL_SHAPES = ((1, 1, 1), (1, 1, 7), (5, 1, 1), (3, 4, 5), (7, 3, 6), (4, 9, 11), (6, 6, 6))  # for the brute force


def sites(shape, density, seed=0):
    """A uint8 volume whose non-zero voxels are the sites: 50 %, 1 % (at least one), or the single far corner."""
    a = np.zeros(shape, np.uint8)
    if density == "corner":
        a[-1, -1, -1] = 1
        return a
    rng = np.random.default_rng(seed + 7 * int(np.prod(shape)))
    a[...] = rng.random(shape) < (0.5 if density == "half" else 0.01)
    if density == "sparse" and not a.any():
        a.reshape(-1)[int(rng.integers(a.size))] = 1
    return a


def _volume(shape, *where):
    a = np.zeros(shape, np.uint8)
    for w in where:
        a[w] = 1
    return a


def traps():
    """``name -> (sites uint8, query (z, y, x), the site (z, y, x) the rule picks)``.

    scan_order: sites (0,2,0) and (2,0,0) are equally far from (1,1,0); in the y pass the candidate met first (j = 0)
    carries the larger key, and the answer is (0,2,0): "first met wins" is wrong.
    beyond_*: one candidate at offset 3 along the last scanned axis with g = 16 gives 25; a site at offset 5 with g = 0
    also gives 25 = (1 * 5)^2 and has the lower key: a scan that stops at t t >= best never sees it.  On both sides of
    the query, for the x pass (`_x`) and for the y pass (`_y`)."""
    out = {"scan_order": (_volume((3, 3, 2), (0, 2, 0), (2, 0, 0)), (1, 1, 0), (0, 2, 0))}
    for side, sign in (("right", 1), ("left", -1)):
        out[f"beyond_{side}_x"] = (_volume((1, 9, 13), (0, 8, 6 + 3 * sign), (0, 4, 6 + 5 * sign)), (0, 4, 6), (0, 4, 6 + 5 * sign))
        out[f"beyond_{side}_y"] = (_volume((9, 13, 2), (8, 6 + 3 * sign, 1), (4, 6 + 5 * sign, 1)), (4, 6, 1), (4, 6 + 5 * sign, 1))
    return out


def linear(shape, zyx):
    return (zyx[0] * shape[1] + zyx[1]) * shape[2] + zyx[2]


def as_input(a, invert):
    """The volume whose sites under `invert` are the non-zero voxels of `a`."""
    return (a == 0).astype(np.uint8) if invert else a


@functools.lru_cache(maxsize=None)
def statement(shape, density, invert, spacing):
    """``_edt.nearest`` of ``as_input(sites(shape, density), invert)``: computed once, shared, read-only."""
    d2, index = _edt.nearest(as_input(sites(shape, density), invert), invert, spacing)
    d2.setflags(write=False)
    index.setflags(write=False)
    return d2, index


def ball_mask(shape, centre, radius):
    z, y, x = np.indices(shape)
    return ((z - centre[0]) ** 2 + (y - centre[1]) ** 2 + (x - centre[2]) ** 2 <= radius ** 2).astype(np.uint8)


def blobs(shape=(14, 16, 19), seed=3):
    """A mask with two balls, one cut by the grid's edge, specks and a hole, for the morphology equalities and the
    surfaces; its erosion by a ball of radius 3 is not empty."""
    rng = np.random.default_rng(seed)
    a = ball_mask(shape, (6, 7, 8), 5) | ball_mask(shape, (9, 12, 16), 4)
    a |= (rng.random(shape) < 0.01).astype(np.uint8)
    a[2, 7, 8] = 0  # a hole
    return a


def slab():
    """``(classes int32, island size)``: two classes side by side, an island of each inside the other (2 x 2 x 2 voxels),
    and a speck of class 2 in the class-0 margin."""
    c = np.zeros((8, 10, 16), np.int32)
    c[1:7, 1:9, 1:7] = 1
    c[1:7, 1:9, 7:13] = 2
    c[3:5, 4:6, 3:5] = 2   # an island of 2 inside 1
    c[3:5, 4:6, 9:11] = 1  # an island of 1 inside 2
    c[4, 5, 15] = 2        # a speck surrounded by class 0
    return c, 8
