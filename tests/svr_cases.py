"""Cases shared by tests/test_svr_host.py and tests/test_svr_gpu.py: batches of slices with an affine each (stacks of
unequal brick counts, poses mixed on purpose, edge coordinates), the slice tree written lane by lane in Python floats
(nothing of fetal_t2mapping_amd._svr), a small registration problem with known poses, and the displacement error of a set of
poses on the moved phantom."""
import numpy as np

import register_cases as RC
import sr_cases as K
import sr_slice_cases as L
from fetal_t2mapping_amd import _register as G
from fetal_t2mapping_amd import _resample as R
from fetal_t2mapping_amd import _svr as V


def smooth_volume(geom, seed, n=6, amp=300.0):
    """A float32 volume on ``geom``: a sum of Gaussians at random places plus a little noise, nowhere flat."""
    rng = np.random.default_rng(seed)
    m, o = R._index_to_point(geom)
    size = np.array(geom.GetSize(), np.float64)
    lo, hi = o, o + m @ (size - 1)
    centres = rng.uniform(np.minimum(lo, hi), np.maximum(lo, hi), size=(n, 3))
    sigmas = rng.uniform(3.0, 7.0, size=n)
    amps = rng.uniform(0.4, 1.0, size=n) * amp
    return (RC.gaussians(geom, centres, sigmas, amps) + rng.normal(0, 2.0, geom.shape)).astype(np.float32)


class Batch:
    """``stacks`` / ``masks`` (lists), ``volume`` / ``volume_mask``, and the records ``A (K, 3, 4)``, ``stack``, ``slice``."""

    def __init__(self, geoms, poses, hr, seed):
        rng = np.random.default_rng(seed)
        self.geoms, self.hr, self.poses = geoms, hr, poses
        self.stacks = [rng.normal(500, 200, g.shape).astype(np.float32) for g in geoms]
        self.masks = [(rng.random(g.shape) > 0.2).astype(np.uint8) for g in geoms]
        self.volume = rng.normal(500, 200, hr.shape).astype(np.float32)
        self.volume_mask = (rng.random(hr.shape) > 0.1).astype(np.uint8)
        self.A = np.stack([R.index_affine(g, hr, np.linalg.inv(t)) for g, ts in zip(geoms, poses) for t in ts])
        self.stack = np.array([s for s, g in enumerate(geoms) for _ in range(g.shape[0])], np.int32)
        self.slice = np.array([k for g in geoms for k in range(g.shape[0])], np.int32)

    def reference(self, r, with_masks=True):
        """``(sums, scale)`` of record ``r`` from tests/register_cases.reference_sums: the whole stack with the fixed mask
        cleared outside the record's slice."""
        s, k = self.stack[r], self.slice[r]
        only = np.zeros(self.stacks[s].shape, np.uint8)
        only[k] = self.masks[s][k] if with_masks else 1
        return RC.reference_sums(self.stacks[s], self.volume, self.A[r], only, self.volume_mask if with_masks else None)


def mixed_batch():
    """HR 27 x 23 x 25; stacks 21 x 19 x 5 (oblique, the mixed poses of ``sr_slice_cases.MixedCase``: the exact stack pose,
    rotations up to 25 degrees, a slice wholly off the grid, one partly off, one fully masked), 19 x 40 x 3 and 70 x 33 x 4
    (1, 2 and 4 bricks a slice) with random poses up to 25 degrees."""
    c = L.MixedCase("ax_oblique")
    centre = K.grid_centre(c.hr)
    g1 = K.centred_stack(K.DIRECTIONS["cor"], (19, 40, 3), (1.1, 0.5, 5.0), centre)
    g2 = K.centred_stack(K.DIRECTIONS["sag_oblique"], (70, 33, 4), (0.3, 0.6, 4.0), centre)
    rng = np.random.default_rng(91)
    poses = [c.transforms]
    for g in (g1, g2):
        lz = g.shape[0]
        p = rng.uniform(-1, 1, size=(lz, 6)) * np.array([np.deg2rad(25.0)] * 3 + [3.0] * 3)
        poses.append(np.stack([G.compose(p[k], centre) for k in range(lz)]))
    b = Batch([c.stack, g1, g2], poses, c.hr, 92)
    b.masks[0] = c.mask
    return b


def edge_batch():
    """One stack 6 x 5 x 3 against a 5 x 4 x 3 volume under ``c = i - 0.5`` on x and ``c = i + 0.5`` on y: ``ix = 0`` lands
    exactly on -0.5 (inside) and ``iy = 3`` exactly on ``n - 0.5`` (outside); and a volume of one voxel along each axis in
    turn; slices ``k > 0`` throughout."""
    out = []
    stack_geom = R.Geometry((6, 5, 3))
    a = np.array([[1.0, 0, 0, -0.5], [0, 1.0, 0, 0.5], [0, 0, 1.0, 0.0]])
    hr = R.Geometry((5, 4, 3))
    b = Batch([stack_geom], [np.repeat(np.eye(4)[None], 3, axis=0)], hr, 93)
    b.A = np.repeat(a[None], 3, axis=0)
    out.append(("edges", b))
    for axis in range(3):
        size = [7, 6, 5]
        size[axis] = 1
        hr = R.Geometry(size)
        sg = R.Geometry((6, 5, 3), (0.9, 1.1, 1.3), (0.2, 0.3, 0.1) if axis != 2 else (0.2, 0.3, -1.4))
        b = Batch([sg], [np.stack([RC.rigid((3.0, -2.0, 4.0), (0.3, -0.2, 0.1))] * 3)], hr, 94 + axis)
        out.append((f"thin{axis}", b))
    return out


# ---- the tree, lane by lane ---------------------------------------------------------------------------------------------
def _halving(v):
    v = list(v)
    while len(v) > 1:
        h = len(v) // 2
        v = [v[i] + v[i + h] for i in range(h)]
    return v[0]


def tree_by_hand(terms):
    """The slice tree of include/t2fit.h over one kind of terms, ``(ly, lx)`` float64, in Python floats: a lane adds 8
    rows from 0.0, 64 lanes by halving, the four waves as (w0 + w2) + (w1 + w3), the slabs in passes of 256."""
    t = np.asarray(terms, np.float64)
    ly, lx = t.shape
    rows = [[float(v) for v in row] for row in t]
    slabs = []
    for by in range(-(-ly // 32)):
        for bx in range(-(-lx // 64)):
            waves = []
            for w in range(4):
                lanes = []
                for lane in range(64):
                    x, acc = 64 * bx + lane, 0.0
                    for r in range(8):
                        y = 32 * by + 8 * w + r
                        if x < lx and y < ly:
                            acc = acc + rows[y][x]
                        else:
                            acc = acc + 0.0
                    lanes.append(acc)
                waves.append(_halving(lanes))
            slabs.append((waves[0] + waves[2]) + (waves[1] + waves[3]))
    v = slabs
    while True:
        groups = -(-len(v) // 256)
        v = [_halving((v[256 * g:256 * g + 256] + [0.0] * 256)[:256]) for g in range(groups)]
        if groups == 1:
            return v[0], len(slabs)


# ---- a registration problem with known poses ----------------------------------------------------------------------------
class Problem:
    """A smooth 24^3-scale volume on an oblique grid and two stacks (9 and 7 slices) whose slices are sampled from it at
    known rigid poses about the centroid of their own masks, under a non-identity stack transform for the second stack.
    ``true`` holds the parameters; ``masks`` keep the image of every slice well inside the volume."""

    def __init__(self, deg=2.5, mm=1.2, seed=71):
        self.hr = R.Geometry((24, 26, 22), (1.0, 1.0, 1.0), (-11.0, -14.5, -7.2), RC.OBLIQUE.ravel())
        self.volume = smooth_volume(self.hr, seed)
        centre = K.grid_centre(self.hr)
        self.geoms = {"a": K.centred_stack(RC.OBLIQUE, (14, 15, 5), (1.0, 1.1, 2.5), centre),
                      "b": K.centred_stack(RC.OBLIQUE @ RC.rot(0, 90.0), (13, 12, 4), (1.1, 1.0, 3.0), centre)}
        self.transforms = {"b": RC.rigid((2.0, -3.0, 1.5), (0.8, -0.6, 0.4), centre)}
        self.masks = {}
        for o, g in self.geoms.items():
            m = np.zeros(g.shape, np.uint8)
            m[:, 2:-2, 2:-2] = 1
            self.masks[o] = m
        self.true = {o: L.motion(g.shape[0], deg, mm, seed + 1 + i) for i, (o, g) in enumerate(self.geoms.items())}
        self.models = {o: V.SliceModel(g, self.masks[o], self.hr, self.transforms.get(o)) for o, g in self.geoms.items()}
        self.stacks = {}
        for o, g in self.geoms.items():
            lz = g.shape[0]
            planes = [R.resample(self.volume, self.models[o].affine(k, self.true[o][k]), (1,) + g.shape[1:], start=(0, 0, k))[0]
                      for k in range(lz)]
            self.stacks[o] = np.stack(planes).astype(np.float32)


_MADE = {}


def problem():
    if "p" not in _MADE:
        _MADE["p"] = Problem()
    return _MADE["p"]


# ---- the moved phantom --------------------------------------------------------------------------------------------------
def phantom_masks():
    stacks = L.moved_phantom()[0]
    return {o: (v[0] > 60).astype(np.uint8) for o, v in stacks.items()}


def displacement_error(found):
    """{stack: the mean over its slices of the mean distance [mm] between the images of the slice's mask voxels under the
    found and the true pose (stack point -> volume point)} on ``sr_slice_cases.moved_phantom()``; ``found`` None: the
    stacks' own poses."""
    _, geoms, _, _, poses = L.moved_phantom()
    masks = phantom_masks()
    out = {}
    for o, g in geoms.items():
        m, og = R._index_to_point(g)
        per_slice = []
        for k in range(g.shape[0]):
            idx = np.argwhere(masks[o][k])[:, ::-1].astype(np.float64)
            pts = np.concatenate([idx, np.full((len(idx), 1), float(k))], axis=1) @ m.T + og
            a = np.eye(4) if found is None else np.linalg.inv(found[o][k])
            b = np.linalg.inv(poses[o][k])
            d = pts @ (a[:3, :3] - b[:3, :3]).T + (a[:3, 3] - b[:3, 3])
            per_slice.append(np.mean(np.sqrt(np.sum(d * d, axis=1))))
        out[o] = float(np.mean(per_slice))
    return out


SVR_N_ITER, SVR_PROX_ITER = 4, 10  # of the reconstructions inside the recovery tests: short, the poses are the subject


def phantom_statement(rounds):
    """``_svr.reconstruct_svr`` on the moved phantom with masks ``stack > 60``, once per number of rounds."""
    key = ("svr", rounds)
    if key not in _MADE:
        stacks, geoms = L.moved_phantom()[:2]
        _MADE[key] = V.reconstruct_svr(stacks, geoms, rounds=rounds, slice_masks=phantom_masks(), n_iter=SVR_N_ITER,
                                       prox_iter=SVR_PROX_ITER)
    return _MADE[key]
