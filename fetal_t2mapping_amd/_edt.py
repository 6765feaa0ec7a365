"""The exact Euclidean distance transform in numpy: the statement the kernels of csrc/t2fit_edt.hip are held to, element
for element (``_gpu_edt`` binds them; ``t2map.distance``).  No scipy: ``sqrt(d2)`` equals
``scipy.ndimage.distance_transform_edt(mask, sampling=spacing)`` and the tests check that, but scipy's *indices* differ at
ties and are no yardstick.

A volume is ``(nz, ny, nx)``; ``v = (z * ny + y) * nx + x`` is a voxel's linear index.  The **sites** are the voxels
equal to 0 (``invert=1``: scipy's convention for a mask) or the voxels not equal to 0 (``invert=0``).  ``spacing`` is
``(sz, sy, sx)`` in float64, each finite and > 0, default 1.  Per voxel: ``d2`` (float64), the squared distance to the
nearest site, and ``index`` (int32), that site's linear index; with no site anywhere ``d2 = +inf`` and ``index = -1``.

The statement IS three passes, in the order z, y, x, each an exact 1-D minimisation along its axis::

    start:   g = 0.0 at a site, +inf elsewhere;   key = the site's own linear index, -1 elsewhere
    pass a:  g'[i] = min over j along axis a of  g[j] + t * t,  t = float64(i - j) * s_a
             key'[i] = key[j] of the minimising j; among equal values the LOWEST key wins; a j with key -1 never wins

(one multiply, one square, one add, all float64).  The pass order makes the sum ``((dz sz)^2 + (dy sy)^2) + (dx sx)^2``,
the order in which scipy squares and adds; for unit and for dyadic spacing every operation is exact, ``d2`` is the exact
squared distance and ``index`` the lowest linear index among the nearest sites.  For any spacing ``d2`` equals the
brute-force minimum of that expression over all sites: float addition is monotone, so minimising per axis loses nothing.
(Spacings whose squares overflow or underflow float64 are outside the statement's guarantees.)"""
from __future__ import annotations

import numpy as np

from . import _components, _morph

MAX_AXIS = 2048  # the device's limit per axis (include/t2fit.h T2FIT_EDT_MAX_AXIS); the statement has none
MAX_VOXELS = 2**31 - 1


def check_spacing(spacing):
    """``(sz, sy, sx)`` as float64; None is 1."""
    s = np.ones(3, np.float64) if spacing is None else np.asarray(spacing, np.float64).reshape(-1)
    if s.size != 3 or not np.all(np.isfinite(s)) or not np.all(s > 0):
        raise ValueError(f"spacing must be three finite numbers > 0 (sz, sy, sx), got {spacing!r}")
    return s


def _volume(vol):
    a = np.asarray(vol)
    if a.ndim != 3:
        raise ValueError(f"a volume must be 3-D (z, y, x), got shape {a.shape}")
    if a.size < 1 or a.size > MAX_VOXELS:
        raise ValueError("a volume must have between 1 and 2^31 - 1 voxels")
    return a


def _pass(g, key, axis, s):
    """One exact min-plus pass along `axis`: a loop over the source position j, vectorised over the volume."""
    g, key = np.moveaxis(g, axis, 0), np.moveaxis(key, axis, 0)
    n = g.shape[0]
    best = np.full(g.shape, np.inf)
    bkey = np.full(key.shape, -1, np.int32)
    i = np.arange(n, dtype=np.int64)
    tail = (1,) * (g.ndim - 1)
    for j in range(n):
        t = (i - j).astype(np.float64) * s
        cand = g[j][None] + (t * t).reshape((n,) + tail)
        kj = np.broadcast_to(key[j][None], cand.shape)
        take = (kj >= 0) & ((cand < best) | ((cand == best) & ((bkey < 0) | (kj < bkey))))
        best = np.where(take, cand, best)
        bkey = np.where(take, kj, bkey)
    return np.ascontiguousarray(np.moveaxis(best, 0, axis)), np.ascontiguousarray(np.moveaxis(bkey, 0, axis))


def nearest(vol, invert=0, spacing=None):
    """``(d2 float64, index int32)`` of the volume: the three passes of the module docstring."""
    a = _volume(vol)
    if invert not in (0, 1, False, True):
        raise ValueError(f"invert must be 0 or 1, got {invert!r}")
    s = check_spacing(spacing)
    site = (a == 0) if invert else (a != 0)
    g = np.where(site, 0.0, np.inf)
    key = np.where(site, np.arange(a.size, dtype=np.int64).reshape(a.shape), -1).astype(np.int32)
    for axis in range(3):
        g, key = _pass(g, key, axis, s[axis])
    return g, key


def brute(vol, invert=0, spacing=None):
    """``(d2, index)`` by the minimum of ``((dz sz)^2 + (dy sy)^2) + (dx sx)^2`` over all sites, the lowest linear index
    among the minima: what the passes must give (``index`` where the arithmetic is exact).  For small volumes."""
    a = _volume(vol)
    s = check_spacing(spacing)
    site = np.flatnonzero((a.reshape(-1) == 0) if invert else (a.reshape(-1) != 0))
    if site.size == 0:
        return np.full(a.shape, np.inf), np.full(a.shape, -1, np.int32)
    z, y, x = np.unravel_index(np.arange(a.size), a.shape)
    qz, qy, qx = np.unravel_index(site, a.shape)
    tz = (z[:, None] - qz[None]).astype(np.float64) * s[0]
    ty = (y[:, None] - qy[None]).astype(np.float64) * s[1]
    tx = (x[:, None] - qx[None]).astype(np.float64) * s[2]
    d = (tz * tz + ty * ty) + tx * tx
    best = d.min(axis=1)
    first = np.argmax(d == best[:, None], axis=1)  # the sites are in ascending linear index
    return best.reshape(a.shape), site[first].astype(np.int32).reshape(a.shape)


def edt(mask, spacing=None, squared=False):
    """scipy's convention: the distance from every voxel to the nearest voxel that is 0 (``inf`` if the mask has no zero);
    ``sqrt(d2)``, or ``d2`` with ``squared``."""
    d2 = nearest(mask, 1, spacing)[0]
    return d2 if squared else np.sqrt(d2)


def fill_nearest(labels, where, index):
    """``out[v] = labels[index[v]]`` where ``where[v] != 0 and index[v] >= 0``, else ``labels[v]``."""
    lab = np.asarray(labels)
    flat, idx = lab.reshape(-1), np.asarray(index).reshape(-1)
    take = (np.asarray(where).reshape(-1) != 0) & (idx >= 0)
    return np.where(take, flat[np.where(take, idx, 0)], flat).reshape(lab.shape)


def dilate_mm(mask, r, spacing=None):
    """The mask grown by a Euclidean ball of radius ``r`` (in the units of ``spacing``): ``d2(sites = mask != 0) <= r^2``."""
    return (nearest(np.asarray(mask) != 0, 0, spacing)[0] <= np.float64(r) ** 2).astype(np.uint8)


def erode_mm(mask, r, spacing=None):
    """The mask shrunk by that ball: ``d2(sites = mask == 0) > r^2``.  The outside of the grid holds no site, so a mask
    without a zero stays whole."""
    return (nearest(np.asarray(mask) != 0, 1, spacing)[0] > np.float64(r) ** 2).astype(np.uint8)


def surface(mask):
    """The mask's voxels with a 6-neighbour outside it (the outside of the grid counts as outside):
    ``mask & ~erode(mask, cross(1), border_value=0)``."""
    m = np.asarray(mask) != 0
    return (m & ~(_morph.erode(m, _morph.cross(1), border_value=0) != 0)).astype(np.uint8)


def surface_reduce(ab, ba):
    """The surface measures from the gathered distances, a's surface to b's (`ab`) and the reverse, each in ascending
    linear index of its surface voxel.  The sums run in that order with numpy's ``sum`` over float64, `ab` first."""
    ab, ba = np.asarray(ab, np.float64), np.asarray(ba, np.float64)
    return {"hausdorff": float(max(ab.max(), ba.max())),
            "hd95": float(max(np.percentile(ab, 95), np.percentile(ba, 95))),
            "assd": float((ab.sum() + ba.sum()) / (ab.size + ba.size)),
            "n_a": int(ab.size), "n_b": int(ba.size)}


def surface_distances(a, b, spacing=None):
    """Hausdorff, HD95 and the average symmetric surface distance of two masks: the distances ``sqrt(d2)`` from every
    surface voxel of ``a`` to the sites ``surface(b)``, and the reverse.  ``hausdorff``: the maximum of both; ``hd95``:
    the larger of the two ``np.percentile(., 95)``; ``assd``: the sum of both over the count of both; ``n_a``, ``n_b``:
    the counts.  An empty surface is a ValueError."""
    sa, sb = surface(a), surface(b)
    if sa.shape != sb.shape:
        raise ValueError("the two masks must share a grid")
    if not sa.any() or not sb.any():
        raise ValueError("surface_distances: a mask is empty, it has no surface")
    to_b, to_a = np.sqrt(nearest(sb, 0, spacing)[0]), np.sqrt(nearest(sa, 0, spacing)[0])
    return surface_reduce(to_b[sa != 0], to_a[sb != 0])


def reassign_small(classes, min_size, connectivity=1, spacing=None):
    """``(classes int32, n_changed)``: every component (``_components.label`` of the class volume) of fewer than
    ``min_size`` voxels takes, voxel by voxel, the class at its nearest site, the sites being the voxels that are not 0
    and not in a small component.  Class 0 stays 0; one round; with no site the volume comes back unchanged.  A speck
    surrounded by class 0 takes the class of the nearest tissue but stays a speck: deleting it is ``remove_small``'s job."""
    c = np.asarray(classes)
    a = _components.as_classes(c.astype(np.int32) if c.dtype == np.uint8 else c)  # uint8 holds classes here, not a mask
    if int(min_size) < 0:
        raise ValueError("min_size must not be negative")
    lab, n = _components.label(a, connectivity)
    sizes = _components.stats(lab, n)[0]
    small = (sizes < int(min_size))[lab] & (lab != 0)
    _, index = nearest((a != 0) & ~small, 0, spacing)
    out = fill_nearest(a, small, index).astype(np.int32)
    return out, int((out != a).sum())
