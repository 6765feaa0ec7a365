"""Inputs shared by tests/test_register_host.py and tests/test_register_gpu.py: seeded, built once per process."""
import functools

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
