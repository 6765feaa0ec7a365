"""Shared builders of the connected-component tests (test_components_host.py, test_components_gpu.py): the shapes around
the device's tile, the patterns, and scipy's labelling as the reference.  Everything is small: the largest volume has
about 20 thousand voxels."""
import functools

import numpy as np

from fetal_t2mapping_amd import _components

T = _components.TILE  # (z, y, x)
CONNECTIVITIES = (1, 2, 3)
DENSITIES = (0.05, 0.2, 0.31, 0.5, 0.9)


def shapes():
    """(1,1,1), (1,1,65), (1,7,9); per axis T-1, T, T+1 and 2T+1 with the other two axes small; one volume of two tiles
    and a bit along every axis."""
    out = [(1, 1, 1), (1, 1, 65), (1, 7, 9)]
    small = (3, 5, 6)
    for axis in range(3):
        for n in (T[axis] - 1, T[axis], T[axis] + 1, 2 * T[axis] + 1):
            s = list(small)
            s[axis] = n
            out.append(tuple(s))
    out.append(BIG)
    return out


BIG = (2 * T[0] + 1, 2 * T[1] + 1, 2 * T[2] + 3)  # (9, 17, 131)
MID = (T[0] + 1, T[1] + 2, T[2] + 3)              # (5, 10, 67): more than one tile along every axis


def empty(shape):
    return np.zeros(shape, np.uint8)


def full(shape):
    return np.ones(shape, np.uint8)


def corners(shape):
    a = np.zeros(shape, np.uint8)
    a[np.ix_(*[sorted({0, n - 1}) for n in shape])] = 1
    return a


def checkerboard(shape):
    z, y, x = np.indices(shape)
    return ((z + y + x) % 2 == 0).astype(np.uint8)


def serpentine(shape):
    """One voxel wide and one component: in every other plane every other row is a line along x; consecutive lines are
    joined at alternating ends, consecutive planes at the end of the last line.  The path visits every tile."""
    nz, ny, nx = shape
    a = np.zeros(shape, np.uint8)
    ys, zs = list(range(0, ny, 2)), list(range(0, nz, 2))
    end = nx - 1
    for kz, z in enumerate(zs):
        order = ys if kz % 2 == 0 else ys[::-1]
        for ky, y in enumerate(order):
            a[z, y, :] = 1
            if ky + 1 < len(order):
                a[z, (y + order[ky + 1]) // 2, end] = 1
                end = nx - 1 - end
        if kz + 1 < len(zs):
            a[z + 1, order[-1], end] = 1
            end = nx - 1 - end
    return a


def comb(shape):
    """Columns along z at every other x and y, joined only by a bar in the last plane: every provisional label merges
    late, and the first voxel lies far from the join."""
    a = np.zeros(shape, np.uint8)
    a[:, ::2, ::2] = 1
    a[-1, :, :] = 1
    return a


def touching_pairs():
    """Pairs of voxels that touch only by an edge and only by a corner, placed across a tile face, a tile edge and a
    tile corner, each pair far from the others: a list of (volume, n at connectivity 1, 2, 3)."""
    shape = (2 * T[0], 2 * T[1], 2 * T[2])
    tz, ty, tx = T
    out = []
    edge_pairs = [((1, 1, tx - 1), (1, 2, tx)),          # across the x face
                  ((1, ty - 1, 5), (2, ty, 5)),          # across the y face
                  ((tz - 1, 3, 9), (tz, 4, 9)),          # across the z face
                  ((1, ty - 1, tx - 1), (1, ty, tx)),    # across a tile edge (y and x)
                  ((tz - 1, ty - 1, 7), (tz, ty, 7)),    # across a tile edge (z and y)
                  ((tz - 1, ty, tx), (tz, ty, tx - 1)),  # x falls while z rises, at a tile corner
                  ((1, 2, 3), (1, 3, 4))]                # inside a tile
    corner_pairs = [((tz - 1, ty - 1, tx - 1), (tz, ty, tx)),  # across a tile corner
                    ((tz - 1, ty, tx - 1), (tz, ty - 1, tx)),  # y falls while z and x rise
                    ((tz - 1, ty - 1, tx), (tz, ty, tx - 1)),  # x falls
                    ((1, 1, tx - 1), (2, 2, tx)),              # across the x face
                    ((tz - 1, 1, 1), (tz, 2, 2)),              # across the z face
                    ((0, 0, 0), (1, 1, 1))]                    # inside a tile
    for pairs, counts in ((edge_pairs, (2, 1, 1)), (corner_pairs, (2, 2, 1))):
        for p, q in pairs:
            a = np.zeros(shape, np.uint8)
            a[p] = a[q] = 1
            out.append((a, counts))
    return out


def random_mask(shape, density, seed=0):
    rng = np.random.default_rng([seed, int(density * 1000), *shape])
    return (rng.random(shape) < density).astype(np.uint8)


def random_classes(shape, seed=0):
    """Classes 0..3, in blobs of a few voxels so that components of one class touch components of another."""
    rng = np.random.default_rng([seed, 77, *shape])
    coarse = rng.integers(0, 4, [(n + 1) // 2 + 1 for n in shape])
    a = np.repeat(np.repeat(np.repeat(coarse, 2, 0), 2, 1), 2, 2)[:shape[0], :shape[1], :shape[2]]
    flip = rng.random(shape) < 0.2
    return np.where(flip, rng.integers(0, 4, shape), a).astype(np.int32)


def two_blobs(shape=MID):
    """Two boxes of equal size (the tie of `largest`: the lower label wins), a smaller box and a single voxel."""
    a = np.zeros(shape, np.uint8)
    a[0:2, 0:3, 0:4] = 1       # 24 voxels, label 1
    a[3:5, 5:8, 60:64] = 1     # 24 voxels, across the x tile face
    a[0:2, 6:8, 20:23] = 1     # 12 voxels
    a[4, 0, 30] = 1
    return a


@functools.lru_cache(maxsize=None)
def mask_cases():
    """(name, uint8 volume) of every binary case; built once, read-only."""
    out = []
    for s in shapes():
        tag = "x".join(str(n) for n in s)
        out += [(f"empty-{tag}", empty(s)), (f"full-{tag}", full(s)), (f"corners-{tag}", corners(s)),
                (f"checker-{tag}", checkerboard(s)), (f"random0.31-{tag}", random_mask(s, 0.31))]
    for s in (MID, BIG):
        tag = "x".join(str(n) for n in s)
        out += [(f"serpentine-{tag}", serpentine(s)), (f"comb-{tag}", comb(s))]
        out += [(f"random{d}-{tag}", random_mask(s, d, seed=1)) for d in DENSITIES]
    out += [(f"pair{k}", a) for k, (a, _) in enumerate(touching_pairs())]
    out.append(("two-blobs", two_blobs()))
    for _, a in out:
        a.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def class_cases():
    return tuple(("classes-" + "x".join(str(n) for n in s), random_classes(s)) for s in ((1, 7, 9), (3, 5, 2 * T[2] + 1), MID, BIG))


def scipy_label(a, connectivity):
    """scipy's labelling of a mask, or for classes the per-class labellings merged and renumbered by first voxel."""
    from scipy import ndimage

    st = ndimage.generate_binary_structure(3, connectivity)
    a = np.asarray(a)
    if a.dtype == np.uint8:
        lab, n = ndimage.label(a, st)
        return lab.astype(np.int32), int(n)
    first, parts = [], []
    for c in np.unique(a[a != 0]):
        lab, n = ndimage.label(a == c, st)
        flat = lab.reshape(-1)
        for i in range(1, n + 1):
            first.append(int(np.argmax(flat == i)))
            parts.append((lab, i))
    out = np.zeros(a.shape, np.int32)
    for rank, k in enumerate(np.argsort(first)):
        lab, i = parts[k]
        out[lab == i] = rank + 1
    return out, len(first)


@functools.lru_cache(maxsize=None)
def _reference(kind, index, connectivity):
    a = (mask_cases() if kind == "mask" else class_cases())[index][1]
    lab, n = _components.label(a, connectivity)
    lab.setflags(write=False)
    return lab, n


def statement(kind, index, connectivity):
    """The statement's labelling of a case, computed once and shared (read-only)."""
    return _reference(kind, index, connectivity)


def loop_lut(sizes, min_size, max_size, largest, renumber):
    """The selection table, written as a loop."""
    n = len(sizes) - 1
    keep = [False] * (n + 1)
    for i in range(1, n + 1):
        keep[i] = sizes[i] >= min_size and (max_size == 0 or sizes[i] <= max_size)
    if largest:
        best = 0
        for i in range(1, n + 1):
            if keep[i] and (best == 0 or sizes[i] > sizes[best]):
                best = i
        keep = [i == best and best != 0 for i in range(n + 1)]
    table, rank = [0] * (n + 1), 0
    for i in range(1, n + 1):
        if keep[i]:
            rank += 1
            table[i] = rank if renumber else i
    return np.array(table, np.int32), rank


def phantom(shape=(24, 40, 72), centres=((12, 10, 12), (12, 10, 40), (12, 28, 26), (11, 29, 58)), radius=5, specks=12):
    """A synthetic vial phantom: balls of intensity 1000 at the (z, y, x) centres on a background of 0, and single bright
    voxels far from them.  Returns (float32 volume, centres as [x, y, z])."""
    z, y, x = np.indices(shape)
    vol = np.zeros(shape, np.float32)
    for cz, cy, cx in centres:
        vol[(z - cz) ** 2 + (y - cy) ** 2 + (x - cx) ** 2 <= radius * radius] = 1000.0
    rng = np.random.default_rng(5)
    placed = 0
    while placed < specks:
        p = tuple(int(rng.integers(0, n)) for n in shape)
        if all((p[0] - c[0]) ** 2 + (p[1] - c[1]) ** 2 + (p[2] - c[2]) ** 2 > (radius + 3) ** 2 for c in centres):
            vol[p] = 1000.0
            placed += 1
    return vol, [[c[2], c[1], c[0]] for c in centres]
