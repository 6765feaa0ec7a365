"""Cases shared by tests/test_sr_slice_host.py and tests/test_sr_slice_gpu.py: stacks whose slices each have their own
rigid pose.  The dense matrix written pair by pair from the definition in include/t2fit.h with Python floats and an affine
per slice (nothing of fetal_t2mapping_amd._sr), the mixed poses of the device tests, and the phantom acquired through the
operator itself from a subject that moves between slices."""
import numpy as np

import sr_cases as K
from fetal_t2mapping_amd import _resample as R
from fetal_t2mapping_amd import _sr as S
from sr_cases import _coord, _prof, _tri

AXIS_ALIGNED = ("ax", "cor", "sag")


def dense_matrix_slices(Bs, hr_shape, lr_shape, profile, rel):
    """``W[j, v]`` and ``N[j]`` as :func:`sr_cases.dense_matrix`, sample j taking u from the affine of its own slice."""
    hz, hy, hx = hr_shape
    lz, ly, lx = lr_shape
    n_h = hz * hy * hx
    W = np.zeros((lz * ly * lx, n_h), np.float64)
    N = np.zeros(lz * ly * lx, np.float64)
    j = 0
    for jz in range(lz):
        b = [[float(v) for v in row] for row in np.asarray(Bs[jz], np.float64).reshape(3, 4)]
        u = [(_coord(b, 0, x, y, z), _coord(b, 1, x, y, z), _coord(b, 2, x, y, z)) for z in range(hz) for y in range(hy) for x in range(hx)]
        for jy in range(ly):
            for jx in range(lx):
                n = 0.0
                for v, (ux, uy, uz) in enumerate(u):
                    w = (_tri(ux - jx) * _tri(uy - jy)) * _prof(uz - jz, profile, rel)
                    if w > 0.0:
                        W[j, v] = w
                        n = n + w
                N[j] = n
                j += 1
    return W, N


def motion(lz, deg, mm, seed):
    """``(lz, 6)`` Euler parameters, every component uniform in ``+-deg`` degrees / ``+-mm`` millimetres."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1.0, 1.0, size=(lz, 6))
    p[:, :3] *= np.deg2rad(deg)
    p[:, 3:] *= mm
    return p


def moved_case(name, deg=6.0, mm=1.5, seed=61, size="small"):
    """``(case, Bs (lz, 3, 4))``: ``sr_cases.small_case`` / ``gpu_case`` with a random rigid pose per slice about the slice's
    own centre, on top of the case's stack transform."""
    c = K.small_case(name) if size == "small" else K.gpu_case(name)
    lz = c.stack.shape[0]
    t = S.compose_slice_transforms(K.rigid(), motion(lz, deg, mm, seed), c.stack)
    return c, S.slice_affines(c.hr, c.stack, t)


def _about(centre, rot, shift=(0.0, 0.0, 0.0)):
    t = np.eye(4)
    t[:3, :3] = rot
    t[:3, 3] = np.asarray(centre) - rot @ np.asarray(centre) + np.asarray(shift)
    return t


class MixedCase:
    """``gpu_case`` geometry (HR 27 x 23 x 25, stack 21 x 19 x 5 at 1.0 x 1.1 x 4.5 mm, 5 mm thick) with the poses mixed on
    purpose.  Slice 0 keeps the exact stack pose (the identity for ax / cor / sag, so that the half-open box edge falls on
    voxel centres; the rigid transform of ``sr_cases`` for the oblique ones), slice 1 is rotated by 25, -17 and 11 degrees,
    slice 2 is shifted wholly off the grid (all N = 0), slice 3 is shifted so that part of it leaves the grid and rotated
    by -25 degrees in plane, slice 4 is tilted and fully masked."""

    def __init__(self, name, seed=62):
        base = None if name in AXIS_ALIGNED else K.rigid()
        self.name = name
        self.hr = R.Geometry((27, 23, 25), (1.0, 1.0, 1.0), (-11.0, -14.5, -7.2))
        self.stack = K.centred_stack(K.DIRECTIONS[name], (21, 19, 5), (1.0, 1.1, 4.5), K.grid_centre(self.hr))
        self.rel = 5.0 / 4.5
        b0 = np.eye(4) if base is None else base
        c = K.grid_centre(self.hr)
        d = np.asarray(K.DIRECTIONS[name], np.float64)
        self.transforms = np.stack([
            b0,
            _about(c, K._rot(0, 25.0) @ K._rot(1, -17.0) @ K._rot(2, 11.0)) @ b0,
            _about(c, np.eye(3), (400.0, -300.0, 250.0)) @ b0,
            _about(c, d @ K._rot(2, -25.0) @ d.T, d @ np.array([9.0, -7.0, 0.0])) @ b0,
            _about(c, K._rot(1, 8.0), (0.5, 0.25, -1.0)) @ b0,
        ])
        self.B = S.slice_affines(self.hr, self.stack, self.transforms)
        if base is None:  # the exact stack pose: the very affine the stack-wise path takes
            assert np.array_equal(self.B[0], R.index_affine(self.hr, self.stack))
        rng = np.random.default_rng(seed)
        self.mask = (rng.random(self.stack.shape) > 0.2).astype(np.uint8)
        self.mask[4] = 0


def thin_case():
    """A thin-slice stack with more slices than one culling pass of 256: 9 x 8 x 300 at 1.0 x 1.1 x 0.1 mm, 1.5 mm thick,
    against HR 11 x 9 x 10, every slice with a small pose of its own."""
    hr = R.Geometry((11, 9, 10), (1.0, 1.0, 1.0), (-11.0, -14.5, -7.2))
    stack = K.centred_stack(K.DIRECTIONS["ax_oblique"], (9, 8, 300), (1.0, 1.1, 0.1), K.grid_centre(hr) + np.array([0.0, 0.0, -8.0]))
    t = S.compose_slice_transforms(K.rigid(0.5), motion(300, 5.0, 1.0, 63), stack)
    return hr, stack, S.slice_affines(hr, stack, t), 1.5 / 0.1


# ---- the phantom, acquired from a moving subject ---------------------------------------------------------------------------
_MOVED = {}


def moved_phantom(n_te=1, deg=4.0, mm=2.0, sigma=15.0, seed=64):
    """``(stacks, geoms, truth, grid, slice_transforms)``: the truth of ``sr_cases.phantom()`` (its first ``n_te`` echoes)
    acquired through the operator itself, every slice with its own rigid pose about its own centre (components uniform in
    ``+-deg`` / ``+-mm``), plus Rician noise of ``sigma``."""
    key = (n_te, deg, mm, sigma, seed)
    if key not in _MOVED:
        _, geoms, truth, grid, _, _ = K.phantom()
        truth = truth[:n_te]
        rng = np.random.default_rng(seed)
        stacks, poses = {}, {}
        for i, o in enumerate(("ax", "cor", "sag")):
            lz = geoms[o].shape[0]
            poses[o] = S.compose_slice_transforms(None, motion(lz, deg, mm, seed + 1 + i), geoms[o])
            clean = S.forward_slices(truth, S.slice_affines(grid, geoms[o], poses[o]), geoms[o].shape, "box", 1.0, out_dtype=np.float64)[0]
            noisy = np.sqrt((clean + rng.normal(0, sigma, clean.shape)) ** 2 + rng.normal(0, sigma, clean.shape) ** 2)
            stacks[o] = noisy.astype(np.float32)
        _MOVED[key] = (stacks, geoms, truth, grid, poses)
    return _MOVED[key]


def moved_statement(n_iter, prox_iter, aware, **kw):
    """The statement's loop on the moved phantom, with or without the slice poses, once per argument set."""
    key = ("s", n_iter, prox_iter, aware, tuple(sorted(kw.items())))
    if key not in _MOVED:
        stacks, geoms, _, _, poses = moved_phantom(**kw)
        _MOVED[key] = S.reconstruct_sr(stacks, geoms, n_iter=n_iter, prox_iter=prox_iter, return_info=True,
                                       slice_transforms=poses if aware else None)
    return _MOVED[key]
