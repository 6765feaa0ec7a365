"""Resampling of a volume onto another grid and the merge of three orthogonal thick-slice stacks, restated in numpy:
the executable statement of the definition in include/t2fit.h (t2fit_resample_dev, t2fit_reconstruct_dev), which stands
for steps 1 and 2 of the reference's run_qmri_reconstruction.py (utils/qmri_utils.py: resample_volume :62-80,
reconstruct_vol_trilinear :82-136) with the rigid registration taken as an input.  Arrays are ``(Z, Y, X)``, x fastest;
geometry is ITK's (size, spacing, origin, direction in the LPS frame, as ``nifti.Image`` carries it) and stays on the
host: the device sees the 12 doubles of :func:`index_affine` and nothing else.  Every operation is one float64 rounding
in the order written.  Host code for tests and baselines: the product path is the HIP kernel.

Pinned against the reference's own calls (tests/test_recon_host.py): the merge -- scipy's RegularGridInterpolator at
its own nodes is the identity, ``np.mean`` of three arrays is ``((a + b) + c) / 3``.  Not pinned (SimpleITK is not
available where this was written): ITK's handling of the half-voxel rim, the tie rule of its nearest-neighbour
interpolator and its cast of the float64 result to an integer pixel type; they are stated here as ITK documents them."""
from __future__ import annotations

import numpy as np

LINEAR, NEAREST = 0, 1
INTERPS = {"linear": LINEAR, "nearest": NEAREST}
ORIENTATIONS = ("ax", "cor", "sag")


class Geometry:
    """Size (x, y, z), spacing, origin and 3 x 3 direction (row-major 9-tuple) of a grid, with the Get* methods of
    ``nifti.Image`` / ``SimpleITK.Image``."""

    def __init__(self, size, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0),
                 direction=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)):
        self._size = tuple(int(v) for v in size)
        self._spacing, self._origin = tuple(map(float, spacing)), tuple(map(float, origin))
        self._direction = tuple(map(float, np.asarray(direction, np.float64).ravel()))
        if len(self._size) != 3 or len(self._spacing) != 3 or len(self._origin) != 3 or len(self._direction) != 9:
            raise ValueError("a geometry has 3 sizes, 3 spacings, 3 origin coordinates and a 3 x 3 direction")

    def GetSize(self): return self._size
    def GetSpacing(self): return self._spacing
    def GetOrigin(self): return self._origin
    def GetDirection(self): return self._direction

    @property
    def shape(self):
        """The ``(Z, Y, X)`` shape of an array on this grid."""
        return self._size[::-1]

    def __repr__(self):
        return f"Geometry(size={self._size}, spacing={self._spacing}, origin={self._origin}, direction={self._direction})"


def as_geometry(g, shape=None) -> Geometry:
    """A :class:`Geometry` from anything with the four Get* methods; ``shape`` (Z, Y, X) overrides the size (an image read
    header-only has an empty array)."""
    if isinstance(g, Geometry) and shape is None:
        return g
    size = tuple(int(v) for v in shape)[::-1] if shape is not None else g.GetSize()
    return Geometry(size, g.GetSpacing(), g.GetOrigin(), g.GetDirection())


def _index_to_point(g):
    """(M, o): physical point p = o + M i of the continuous index i = (ix, iy, iz); M = D diag(s)."""
    d = np.asarray(g.GetDirection(), np.float64).reshape(3, 3)
    return d * np.asarray(g.GetSpacing(), np.float64)[None, :], np.asarray(g.GetOrigin(), np.float64)


def index_affine(dst_geom, src_geom, transform=None) -> np.ndarray:
    """float64 ``A[3, 4]``: the continuous index into the source, ``c_a = A[a, 0] ix + A[a, 1] iy + A[a, 2] iz + A[a, 3]``
    (a = 0 is x), of the integer output index.  ``transform``: 4 x 4, maps an output (fixed) physical point to a source
    (moving) physical point, the sense of ``sitk.Resample``; None is the identity."""
    m_dst, o_dst = _index_to_point(dst_geom)
    m_src, o_src = _index_to_point(src_geom)
    p = np.empty((3, 4), np.float64)
    p[:, :3], p[:, 3] = m_dst, o_dst
    if transform is not None:
        t = np.asarray(transform, np.float64)
        if t.shape != (4, 4) or not np.all(np.isfinite(t)):
            raise ValueError("transform must be a finite 4 x 4 matrix")
        q = np.empty((3, 4), np.float64)
        q[:, :3] = t[:3, :3] @ p[:, :3]
        q[:, 3] = t[:3, :3] @ p[:, 3] + t[:3, 3]
        p = q
    p[:, 3] = p[:, 3] - o_src
    a = np.linalg.solve(m_src, p)  # a division per entry for an axis-aligned source: its own grid maps to the exact identity
    if not np.all(np.isfinite(a)):
        raise ValueError("the source geometry is singular")
    return np.ascontiguousarray(a)


def isotropic_geometry(geom, res=1.0) -> Geometry:
    """The grid ``resample_volume`` (utils/qmri_utils.py:62-80) makes: same origin and direction, spacing ``res``, size
    ``int(round(osz * ospc / nspc))`` per axis (Python's round: halves go to the even neighbour)."""
    new_spacing = [float(res)] * 3
    size = [int(round(osz * ospc / nspc)) for osz, ospc, nspc in zip(geom.GetSize(), geom.GetSpacing(), new_spacing)]
    if min(size) < 1:
        raise ValueError(f"resolution {res} leaves an empty grid {size}")
    return Geometry(size, new_spacing, geom.GetOrigin(), geom.GetDirection())


def _coords(a, out_shape, start=(0, 0, 0)):
    """c_x, c_y, c_z of the output voxels ``start`` (x, y, z) + [0, out_shape), each of shape ``out_shape``."""
    oz, oy, ox = out_shape
    iz = np.arange(start[2], start[2] + oz, dtype=np.float64)[:, None, None]
    iy = np.arange(start[1], start[1] + oy, dtype=np.float64)[None, :, None]
    ix = np.arange(start[0], start[0] + ox, dtype=np.float64)[None, None, :]
    return [np.broadcast_to(((a[k, 0] * ix + a[k, 1] * iy) + a[k, 2] * iz) + a[k, 3], out_shape) for k in range(3)]


def resample(src, A, out_shape, interp="linear", default=0.0, integer_cast=False, start=(0, 0, 0), coords=None):
    """``src`` ``(Z, Y, X)`` (or ``(n, Z, Y, X)``: volumes that share the geometry) sampled at the points of ``A`` (from
    :func:`index_affine`) for an output of ``out_shape`` (Z, Y, X).  linear: float32 result; nearest: the source's type
    (int32 or float32).  ``start`` (x, y, z): evaluate the box of ``out_shape`` whose first voxel has this output index (a
    part of a larger output, with the very same coordinates).  ``coords``: the source coordinates ``(c_x, c_y, c_z)`` of
    every output voxel from the caller (:mod:`_ffd`: a deformation), in place of ``A`` applied to the output index.  See
    include/t2fit.h for the definition."""
    src = np.asarray(src)
    if src.ndim == 4:
        return np.stack([resample(v, A, out_shape, interp, default, integer_cast, start, coords) for v in src])
    if src.ndim != 3:
        raise ValueError("src must be (Z, Y, X) or (n, Z, Y, X)")
    mode = INTERPS[interp] if isinstance(interp, str) else int(interp)
    a = np.asarray(A, np.float64).reshape(3, 4)
    out_shape = tuple(int(v) for v in out_shape)
    n = src.shape[::-1]  # (nx, ny, nz)
    c = _coords(a, out_shape, tuple(int(v) for v in start)) if coords is None else coords
    inside = np.ones(out_shape, bool)
    for k in range(3):
        inside &= (c[k] >= -0.5) & (c[k] < n[k] - 0.5)
    if mode == NEAREST:
        if src.dtype not in (np.float32, np.int32):
            raise ValueError("nearest takes a float32 or int32 source")
        idx = [np.clip(np.floor(c[k] + 0.5), 0, n[k] - 1).astype(np.int64) for k in range(3)]
        got = src[idx[2], idx[1], idx[0]]
        return np.where(inside, got, src.dtype.type(default)).astype(src.dtype)
    if mode != LINEAR:
        raise ValueError(f"unknown interpolation {interp!r}")
    v = src.astype(np.float64)
    b = [np.clip(np.floor(c[k]), 0, n[k] - 1) for k in range(3)]
    d = [np.maximum(c[k] - b[k], 0.0) for k in range(3)]
    lo = [b[k].astype(np.int64) for k in range(3)]
    hi = [np.minimum(lo[k] + 1, n[k] - 1) for k in range(3)]

    def lerp(p, q, w):  # where w == 0 the upper sample is not looked at: an Inf / NaN there stays there
        # An infinite p makes p + w (q - p) the NaN of Inf - Inf; the weighted mean it stands for is that Inf (NaN only
        # against the opposite Inf), which p + q is -- and p + q is NaN wherever p or q is
        with np.errstate(all="ignore"):
            r = p + w * (q - p)
            return np.where(w == 0.0, p, np.where(np.isnan(r), p + q, r))

    def along_x(z, y):
        return lerp(v[z, y, lo[0]], v[z, y, hi[0]], d[0])

    def along_y(z):
        return lerp(along_x(z, lo[1]), along_x(z, hi[1]), d[1])

    r = lerp(along_y(lo[2]), along_y(hi[2]), d[2])
    if integer_cast:  # the stack keeps an int16 pixel type: truncate toward zero, saturate
        r = np.clip(np.trunc(r), -32768.0, 32767.0)
    with np.errstate(all="ignore"):
        return np.where(inside, r.astype(np.float32), np.float32(default))


def merge(h_fixed, r_a, r_b):
    """``np.mean([h_fixed, r_a, r_b], axis=0)`` of float64 arrays, as float32: ``((h_fixed + r_a) + r_b) / 3``."""
    with np.errstate(all="ignore"):
        s = (np.asarray(h_fixed, np.float64) + np.asarray(r_a, np.float64)) + np.asarray(r_b, np.float64)
        return (s / 3.0).astype(np.float32)


def moving_order(fixed="ax"):
    if fixed not in ORIENTATIONS:
        raise ValueError(f"fixed must be one of {ORIENTATIONS}, got {fixed!r}")
    return [o for o in ORIENTATIONS if o != fixed]


def plan(geoms, fixed="ax", res=1.0, transforms=None):
    """The host half of :func:`reconstruct`: for the orientations in the order [fixed, moving a, moving b] the stage-1
    grids ``H_o``, the stage-1 affines (``H_o`` index -> ``L_o`` index) and the two stage-2 affines (fixed-grid index
    -> ``H_m`` index, through ``transforms[m]``).  Returns ``(order, hi_geoms, A1 list of 3, A2 list of 2)``."""
    missing = [o for o in ORIENTATIONS if o not in geoms]
    if missing:
        raise ValueError(f"the reconstruction needs the three orientations ax, cor, sag; missing: {', '.join(missing)}")
    order = [fixed] + moving_order(fixed)
    transforms = transforms or {}
    unknown = [k for k in transforms if k not in order[1:]]
    if unknown:
        raise ValueError(f"transforms are given per moving orientation {order[1:]}, got {unknown}")
    lo = [as_geometry(geoms[o]) for o in order]
    hi = [isotropic_geometry(g, res) for g in lo]
    a1 = [index_affine(h, g) for h, g in zip(hi, lo)]
    a2 = [index_affine(hi[0], hi[m], transforms.get(order[m])) for m in (1, 2)]
    return order, hi, a1, a2


def reconstruct(stacks, geoms, fixed="ax", res=1.0, transforms=None, integer_cast=False, return_stages=False):
    """``stacks``: {"ax" | "cor" | "sag": ``(Z, Y, X)`` or ``(n, Z, Y, X)`` float32}, ``geoms``: their geometries.
    Stage 1 resamples every stack to ``res`` mm isotropic on its own grid, stage 2 the two moving ones onto the fixed
    one's grid (``transforms``: {moving orientation: 4 x 4, fixed point -> moving point}, identity where absent), the
    merge averages the three.  ``integer_cast`` applies to both stages.  Returns ``(merged float32, Geometry of the
    fixed grid)``; with ``return_stages`` also ``{"H": [3 arrays], "R": [2 arrays]}``."""
    geoms = {o: as_geometry(geoms[o], np.asarray(stacks[o]).shape[-3:]) for o in geoms if o in stacks}
    order, hi, a1, a2 = plan(geoms, fixed, res, transforms)
    h = [resample(np.asarray(stacks[o], np.float32), a1[i], hi[i].shape, LINEAR, 0.0, integer_cast)
         for i, o in enumerate(order)]
    r = [resample(h[m], a2[m - 1], hi[0].shape, LINEAR, 0.0, integer_cast) for m in (1, 2)]
    out = merge(h[0], r[0], r[1])
    if return_stages:
        return out, hi[0], {"H": h, "R": r}
    return out, hi[0]
