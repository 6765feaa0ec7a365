"""Connected components in numpy: the statement the kernels of csrc/t2fit_components.hip are held to, element for element
(``_gpu_components`` binds them; ``t2map.components``).  Everything is integer arithmetic.  No scipy: for a binary
volume ``label`` equals ``scipy.ndimage.label(a, generate_binary_structure(3, connectivity))`` -- scipy numbers the
components in ascending order of their first voxel in C order, and so does this -- which the tests check.

A volume is ``(nz, ny, nx)``; ``v = (z * ny + y) * nx + x`` is a voxel's linear index.  ``uint8`` (or bool) input:
foreground = not 0.  Any other integer dtype: classes -- two voxels are connected only when they are neighbours and hold
the same value, which is not 0.  ``connectivity`` 1, 2, 3: 6, 18, 26 neighbours."""
from __future__ import annotations

import numpy as np

from ._abi import COMPONENTS_TILE

TILE = COMPONENTS_TILE  # the tile of the device's local phase (include/t2fit.h T2FIT_COMPONENTS_TILE_*); the statement has none
MAX_VOXELS = 2**31 - 1


def lower_offsets(connectivity):
    """The 3 / 9 / 13 offsets ``(dz, dy, dx)`` of the neighbourhood that lead to a smaller linear index."""
    if connectivity not in (1, 2, 3):
        raise ValueError(f"connectivity must be 1, 2 or 3, got {connectivity!r}")
    out = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dz, dy, dx) < (0, 0, 0) and abs(dz) + abs(dy) + abs(dx) <= connectivity:
                    out.append((dz, dy, dx))
    return out


def as_classes(vol):
    """The volume as the int32 classes the labelling compares: a uint8 / bool volume gives 0 / 1."""
    a = np.asarray(vol)
    if a.ndim != 3:
        raise ValueError(f"a volume must be 3-D (z, y, x), got shape {a.shape}")
    if a.size < 1 or a.size > MAX_VOXELS:
        raise ValueError("a volume must have between 1 and 2^31 - 1 voxels")
    if a.dtype == np.uint8 or a.dtype == np.bool_:
        return (a != 0).astype(np.int32)
    if a.dtype.kind not in "iu":
        raise ValueError("a volume must be uint8 (a mask) or of an integer dtype (classes)")
    if a.size and (a.min() < -2**31 or a.max() >= 2**31):
        raise ValueError("classes must fit int32")
    return a.astype(np.int32)


def _window(n, d):
    """Slices (of the voxel, of its neighbour at offset d) along an axis of length n."""
    return (slice(max(0, -d), n - max(0, d)), slice(max(0, d), n + min(0, d)))


def label(vol, connectivity=1):
    """``(labels int32, n)``: 0 on the background, 1..n on the components, numbered by ascending linear index of their
    first voxel.  A union-find by repeated hooking of the larger root under the smaller and full flattening: every root
    is its set's smallest index."""
    a = as_classes(vol)
    shape = a.shape
    idx = np.arange(a.size, dtype=np.int64).reshape(shape)
    ps, qs = [], []
    for dz, dy, dx in lower_offsets(connectivity):
        (mz, oz), (my, oy), (mx, ox) = _window(shape[0], dz), _window(shape[1], dy), _window(shape[2], dx)
        me, other = a[mz, my, mx], a[oz, oy, ox]
        joined = (me != 0) & (me == other)
        ps.append(idx[mz, my, mx][joined])
        qs.append(idx[oz, oy, ox][joined])
    p, q = np.concatenate(ps), np.concatenate(qs)
    parent = np.arange(a.size, dtype=np.int64)
    while True:
        rp, rq = parent[p], parent[q]
        differ = rp != rq
        if not differ.any():
            break
        np.minimum.at(parent, np.maximum(rp, rq)[differ], np.minimum(rp, rq)[differ])
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
    fg = a.reshape(-1) != 0
    roots = np.flatnonzero(fg & (parent == np.arange(a.size)))
    labels = np.zeros(a.size, np.int32)
    labels[fg] = np.searchsorted(roots, parent[fg]).astype(np.int32) + 1
    return labels.reshape(shape), int(roots.size)


def stats(labels, n):
    """``(sizes int64 (n + 1,), bbox int32 (n + 1, 6), sums int64 (n + 1, 3))`` of the values 0..n of an integer label
    volume (row 0 is the background; other values are ignored): voxel counts, inclusive boxes
    ``(z0, y0, x0, z1, y1, x1)``, coordinate sums ``(sum z, sum y, sum x)``.  A value that does not occur has size 0 and
    the empty box ``(nz, ny, nx, -1, -1, -1)``."""
    lab = np.asarray(labels)
    if lab.ndim != 3 or lab.dtype.kind not in "iu":
        raise ValueError("labels must be a 3-D integer volume")
    n = int(n)
    if n < 0:
        raise ValueError("n must not be negative")
    nz, ny, nx = lab.shape
    sizes = np.zeros(n + 1, np.int64)
    bbox = np.tile(np.array([nz, ny, nx, -1, -1, -1], np.int32), (n + 1, 1))
    sums = np.zeros((n + 1, 3), np.int64)
    z, y, x = np.nonzero((lab >= 0) & (lab <= n))
    rows = lab[z, y, x].astype(np.int64)
    np.add.at(sizes, rows, 1)
    for axis, c in enumerate((z, y, x)):
        np.add.at(sums[:, axis], rows, c.astype(np.int64))
        np.minimum.at(bbox[:, axis], rows, c.astype(np.int32))
        np.maximum.at(bbox[:, 3 + axis], rows, c.astype(np.int32))
    return sizes, bbox, sums


def check_selection(min_size, max_size):
    if int(min_size) < 0 or int(max_size) < 0:
        raise ValueError("min_size and max_size must not be negative (max_size 0: no upper limit)")


def lut(sizes, min_size=0, max_size=0, largest=False, renumber=False):
    """``(table int32 (n + 1,), n_kept)`` from the sizes of stats (row 0 is ignored, ``table[0] = 0``).  Component i
    passes when ``min_size <= sizes[i]`` and (``max_size == 0`` or ``sizes[i] <= max_size``); with ``largest`` only the
    largest of those is kept, on a tie the lowest label.  A kept component maps to its label, with ``renumber`` to its
    rank among the kept; the others to 0."""
    check_selection(min_size, max_size)
    sizes = np.asarray(sizes, np.int64)
    n = sizes.size - 1
    keep = (sizes >= int(min_size)) & ((int(max_size) == 0) | (sizes <= int(max_size)))
    keep[0] = False
    if largest and keep.any():
        best = int(np.flatnonzero(keep & (sizes == sizes[keep].max()))[0])
        keep[:] = False
        keep[best] = True
    table = np.zeros(n + 1, np.int32)
    table[keep] = (np.cumsum(keep)[keep] if renumber else np.flatnonzero(keep)).astype(np.int32)
    return table, int(keep.sum())


def largest_lut(sizes, k):
    """The table that keeps the k largest components (ties: the lower label first, a stable sort) under their own
    labels."""
    sizes = np.asarray(sizes, np.int64)
    if int(k) < 1:
        raise ValueError("k must be at least 1")
    order = np.argsort(-sizes[1:], kind="stable")[:int(k)] + 1
    table = np.zeros(sizes.size, np.int32)
    table[order] = order.astype(np.int32)
    return table


def centroids(sizes, sums):
    """The centroids of the components that occur, rounded half up in integers, ``(2 sum + size) // (2 size)`` per axis:
    int64 ``(m, 3)`` rows ``(x, y, z)`` in label order -- the order of a seed."""
    sizes, sums = np.asarray(sizes, np.int64), np.asarray(sums, np.int64)
    rows = np.flatnonzero(sizes[1:] > 0) + 1
    s = sizes[rows, None]
    return ((2 * sums[rows] + s) // (2 * s))[:, ::-1]


def select(labels, n, min_size=0, max_size=0, largest=False, renumber=False):
    lab = np.asarray(labels)
    table, _ = lut(stats(lab, n)[0], min_size, max_size, largest, renumber)
    return np.where((lab >= 0) & (lab <= n), table[np.clip(lab, 0, n)], 0).astype(np.int32)


def keep_largest(mask, k=1, connectivity=1):
    """The k largest components of a mask (ties: the lower label), as a uint8 mask."""
    lab, n = label(np.asarray(mask) != 0, connectivity)
    return (largest_lut(stats(lab, n)[0], k)[lab] != 0).astype(np.uint8)


def remove_small(vol, min_size, connectivity=1):
    """The volume without the components of fewer than ``min_size`` voxels: a mask gives a uint8 mask, classes give
    int32 classes with the small islands set to 0."""
    a = np.asarray(vol)
    binary = a.dtype == np.uint8 or a.dtype == np.bool_
    lab, n = label(a, connectivity)
    kept = lut(stats(lab, n)[0], min_size)[0][lab] != 0
    return kept.astype(np.uint8) if binary else np.where(kept, as_classes(a), 0).astype(np.int32)


def seeds(mask, connectivity=1, min_size=1, max_size=0):
    """The rounded centroids ``[x, y, z]`` of the components whose size is in range, in label order: the list
    ``cli.load_seeds`` reads."""
    lab, n = label(np.asarray(mask) != 0, connectivity)
    lab = select(lab, n, min_size, max_size, renumber=True)
    sizes, _, sums = stats(lab, int(lab.max(initial=0)))
    return [[int(v) for v in row] for row in centroids(sizes, sums)]
