"""Binary morphology, hole filling and seed labels as the library defines them (csrc/t2fit_morph.hip), in plain numpy:
the statement the device results are compared with, bit for bit.  No scipy here; tests/test_morph_host.py checks these
functions against scipy.ndimage.

Volumes are boolean ``(z, y, x)`` arrays.  A structuring element is a boolean footprint with odd sizes whose origin is
its centre, or its run list: int32 rows ``(dz, dy, x0, x1)`` meaning "the offsets (dz, dy, x), x0 <= x <= x1, belong to
the element" (several runs per (dz, dy) row are allowed).

    dilate(a, S)[v] = OR  over s in S of a[v - s]        outside the volume a reads as border_value
    erode(a, S)[v]  = AND over s in S of a[v + s]        = ~dilate(~a, reflected S, border 1 - border_value)
    close = dilate (n times) then erode (n times);  open = erode then dilate
    unbounded=True: the operation on the volume extended by zeros as far as the element reaches, cropped at the end
"""
from __future__ import annotations

import numpy as np

MAX_RADIUS = 32           # |offset| per axis
MAX_RUNS = 65 * 65 * 4


def _radii(radius):
    r = (radius,) * 3 if np.isscalar(radius) else tuple(radius)
    if len(r) != 3 or any(int(v) != v or v < 0 for v in r):
        raise ValueError(f"radius must be a non-negative integer or three of them (z, y, x), got {radius!r}")
    return tuple(int(v) for v in r)


def ball(radius):
    """The ellipsoid ``sum((d_i / (r_i + 0.5))**2) <= 1`` on the ``(2 r + 1)`` grid; ``radius``: int or (rz, ry, rx)."""
    r = _radii(radius)
    d = np.meshgrid(*[np.arange(-v, v + 1, dtype=np.float64) / (v + 0.5) for v in r], indexing="ij")
    return d[0] ** 2 + d[1] ** 2 + d[2] ** 2 <= 1.0


def box(radius):
    """All ones on the ``(2 r + 1)`` grid; ``radius``: int or (rz, ry, rx)."""
    return np.ones(tuple(2 * v + 1 for v in _radii(radius)), bool)


def cross(connectivity=1):
    """scipy's ``generate_binary_structure(3, connectivity)``: the 3 x 3 x 3 offsets with |dz| + |dy| + |dx| <= c."""
    if connectivity not in (1, 2, 3):
        raise ValueError("connectivity must be 1, 2 or 3")
    d = np.abs(np.arange(-1, 2))
    return d[:, None, None] + d[None, :, None] + d[None, None, :] <= connectivity


def _footprint(fp):
    fp = np.asarray(fp)
    if fp.ndim == 2:
        raise ValueError("a 2-D footprint is ambiguous here: give it its plane, e.g. fp[None] for a (y, x) element")
    if fp.ndim != 3:
        raise ValueError(f"the footprint must be 3-D (z, y, x), got shape {fp.shape}")
    if any(s % 2 == 0 for s in fp.shape):
        raise ValueError(f"footprint sizes must be odd (the origin is the centre), got {fp.shape}")
    if any(s > 2 * MAX_RADIUS + 1 for s in fp.shape):
        raise ValueError(f"footprint sizes must be at most {2 * MAX_RADIUS + 1}, got {fp.shape}")
    return fp != 0


def footprint_runs(fp):
    """``(runs, size)`` of a boolean footprint: int32 ``(n, 4)`` rows (dz, dy, x0, x1) in (z, y, x) order, and the
    footprint's shape."""
    fp = _footprint(fp)
    cz, cy, cx = (s // 2 for s in fp.shape)
    runs = []
    for iz in range(fp.shape[0]):
        for iy in range(fp.shape[1]):
            row = np.concatenate(([False], fp[iz, iy], [False]))
            edges = np.flatnonzero(row[1:] != row[:-1])  # starts and one-past-ends alternate
            for a, b in zip(edges[0::2], edges[1::2]):
                runs.append((iz - cz, iy - cy, int(a) - cx, int(b) - 1 - cx))
    return np.asarray(runs, np.int32).reshape(-1, 4), tuple(int(s) for s in fp.shape)


def runs_footprint(runs, size):
    """The inverse of :func:`footprint_runs`."""
    fp = np.zeros(size, bool)
    cz, cy, cx = (s // 2 for s in size)
    for dz, dy, x0, x1 in np.asarray(runs).reshape(-1, 4):
        fp[dz + cz, dy + cy, x0 + cx:x1 + cx + 1] = True
    return fp


def reflect_runs(runs):
    """The run list of the element reflected through its origin."""
    r = np.asarray(runs, np.int32).reshape(-1, 4)
    return np.stack([-r[:, 0], -r[:, 1], -r[:, 3], -r[:, 2]], axis=1).astype(np.int32)


def _as_runs(element):
    """(runs, size) from a footprint or from an already made (runs, size) pair."""
    if isinstance(element, tuple) and len(element) == 2 and np.asarray(element[0]).ndim == 2:
        return np.asarray(element[0], np.int32).reshape(-1, 4), tuple(int(s) for s in element[1])
    return footprint_runs(element)


def _volume(a):
    a = np.asarray(a)
    if a.ndim != 3:
        raise ValueError(f"the volume must be 3-D (z, y, x), got shape {a.shape}")
    return a != 0


def _dilate_once(a, runs, size, border):
    rz, ry, rx = (s // 2 for s in size)
    nz, ny, nx = a.shape
    p = np.pad(a, ((rz, rz), (ry, ry), (rx, rx)), constant_values=bool(border))
    c = np.zeros((p.shape[0], p.shape[1], p.shape[2] + 1), np.int32)  # c[.., k] = number of ones before padded x = k
    np.cumsum(p, axis=2, out=c[:, :, 1:])
    out = np.zeros(a.shape, bool)
    for dz, dy, x0, x1 in runs:  # a[z - dz, y - dy, x - x1 .. x - x0] holds a one
        rows = c[rz - dz:rz - dz + nz, ry - dy:ry - dy + ny]
        out |= rows[:, :, rx - x0 + 1:rx - x0 + 1 + nx] > rows[:, :, rx - x1:rx - x1 + nx]
    return out


def dilate(a, element, iterations=1, border_value=0):
    a = _volume(a)
    runs, size = _as_runs(element)
    for _ in range(int(iterations)):
        a = _dilate_once(a, runs, size, border_value)
    return a


def erode(a, element, iterations=1, border_value=0):
    a = _volume(a)
    runs, size = _as_runs(element)
    back = reflect_runs(runs)
    for _ in range(int(iterations)):
        a = ~_dilate_once(~a, back, size, 0 if border_value else 1)
    return a


def _unbounded(a, size, iterations):
    pad = tuple((s // 2) * int(iterations) for s in size)
    crop = tuple(slice(p, p + n) for p, n in zip(pad, a.shape))
    return np.pad(a, tuple((p, p) for p in pad)), crop


def close(a, element, iterations=1, border_value=0, unbounded=False):
    a = _volume(a)
    runs, size = _as_runs(element)
    if unbounded:
        if border_value:
            raise ValueError("the unbounded-domain form has zeros outside the volume: border_value must be 0")
        p, crop = _unbounded(a, size, iterations)
        return erode(dilate(p, (runs, size), iterations), (runs, size), iterations)[crop]
    return erode(dilate(a, (runs, size), iterations, border_value), (runs, size), iterations, border_value)


def open(a, element, iterations=1, border_value=0, unbounded=False):  # noqa: A001 (the operation's name)
    a = _volume(a)
    runs, size = _as_runs(element)
    if unbounded:
        if border_value:
            raise ValueError("the unbounded-domain form has zeros outside the volume: border_value must be 0")
        p, crop = _unbounded(a, size, iterations)
        return dilate(erode(p, (runs, size), iterations), (runs, size), iterations)[crop]
    return dilate(erode(a, (runs, size), iterations, border_value), (runs, size), iterations, border_value)


def fill_holes(a, slice_axis=None):
    """The complement of the background that is face-connected to the border.  ``slice_axis`` in (0, 1, 2): every plane
    perpendicular to that axis of the (z, y, x) array is its own 2-D problem whose border is the plane's rim."""
    a = _volume(a)
    if slice_axis not in (None, 0, 1, 2):
        raise ValueError("slice_axis must be None, 0, 1 or 2")
    free = ~a
    axes = [ax for ax in range(3) if ax != slice_axis]
    reached = np.zeros(a.shape, bool)
    for ax in axes:
        idx = [slice(None)] * 3
        for edge in (0, -1):
            idx[ax] = edge
            reached[tuple(idx)] = free[tuple(idx)]
    while True:
        grown = reached.copy()
        for ax in axes:
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[ax], hi[ax] = slice(0, -1), slice(1, None)
            grown[tuple(hi)] |= reached[tuple(lo)]
            grown[tuple(lo)] |= reached[tuple(hi)]
        grown &= free
        if np.array_equal(grown, reached):
            return ~reached
        reached = grown


def seed_labels(shape, seeds, labels, element, dtype=np.uint8):
    """``out[v] = max over seeds s of labels[s] * [v - seed_s in element]``; seeds are (x, y, z) indices; what leaves
    the volume is clipped."""
    runs, size = _as_runs(element)
    fp = runs_footprint(runs, size)
    nz, ny, nx = (int(v) for v in shape)
    out = np.zeros((nz, ny, nx), dtype)
    offs = np.argwhere(fp) - np.array([s // 2 for s in size])
    for (x, y, z), lab in zip(np.asarray(seeds, np.int64).reshape(-1, 3), labels):
        v = offs + np.array([z, y, x])
        v = v[np.all((v >= 0) & (v < np.array([nz, ny, nx])), axis=1)]
        out[v[:, 0], v[:, 1], v[:, 2]] = np.maximum(out[v[:, 0], v[:, 1], v[:, 2]], np.asarray(lab).astype(dtype))
    return out


def relabel(labels, lut):
    """``out[v] = lut[labels[v]]`` where ``0 <= labels[v] < len(lut)``, else 0 (int32)."""
    lab = np.asarray(labels).astype(np.int64)
    lut = np.asarray(lut, np.int32)
    ok = (lab >= 0) & (lab < lut.size)
    return np.where(ok, lut[np.where(ok, lab, 0)], 0).astype(np.int32)


# SynthSeg label -> FeTA tissue class (the table of the reference's convert_synthseg_to_feta): data, not logic
SYNTHSEG_TO_FETA = {
    1: (24,),
    2: (3, 42),
    3: (2, 41),
    4: (4, 5, 14, 15, 43, 44),
    5: (7, 8, 46, 47),
    6: (10, 11, 12, 13, 17, 18, 26, 28, 49, 50, 51, 52, 53, 54, 58, 60),
    7: (16,),
}


def feta_lut():
    """The table as an int32 lookup array: ``lut[synthseg id] = FeTA class``, 0 for every other id."""
    lut = np.zeros(max(max(ids) for ids in SYNTHSEG_TO_FETA.values()) + 1, np.int32)
    for cls, ids in SYNTHSEG_TO_FETA.items():
        lut[list(ids)] = cls
    return lut
