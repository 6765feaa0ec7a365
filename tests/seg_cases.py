"""Cases of the tissue-segmentation tests and a reference written from the definition with per-voxel loops, independent
of fetal_t2mapping_amd._seg (which is vectorised): the host tests hold _seg to it, the GPU tests hold the device to _seg."""
import math

import numpy as np

# ---- the benefit phantom: nested ellipsoids, 4 classes, 2 channels, the atlas displaced and mis-scaled ---------------------
PHANTOM_SHAPE = (32, 40, 48)
PHANTOM_CLASSES = (1, 2, 3, 4)
PHANTOM_MEANS = np.array([[400.0, 300.0], [160.0, 120.0], [280.0, 180.0], [120.0, 400.0]])  # class x channel
PHANTOM_NOISE = 40.0
PHANTOM_RADII = (1.0, 0.8, 0.6, 0.3)  # class k + 1 inside radius k of the unit ellipsoid
ATLAS_SHIFT = (1.0, -2.0, 2.0)
ATLAS_SCALE = 0.9


def _ellipsoid_labels(shape, shift=(0.0, 0.0, 0.0), scale=1.0):
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    half = [(n - 1) / 2.0 for n in shape]
    axes = [0.45 * n * scale for n in shape]
    r = np.sqrt(sum(((v - h - s) / a) ** 2 for v, h, s, a in zip((z, y, x), half, shift, axes)))
    lab = np.zeros(shape, np.int32)
    for k, rad in enumerate(PHANTOM_RADII):
        lab[r < rad] = PHANTOM_CLASSES[k]
    return lab


def phantom(seed=20):
    """(y (2, Z, Y, X) float32, mask uint8, truth int32, atlas int32): the subject, its mask, the true labels and the
    labels an imperfect registration would propagate."""
    truth = _ellipsoid_labels(PHANTOM_SHAPE)
    atlas = _ellipsoid_labels(PHANTOM_SHAPE, ATLAS_SHIFT, ATLAS_SCALE)
    rng = np.random.default_rng(seed)
    y = np.zeros((2,) + PHANTOM_SHAPE, np.float32)
    for c in range(2):
        img = np.zeros(PHANTOM_SHAPE)
        for k, cls in enumerate(PHANTOM_CLASSES):
            img[truth == cls] = PHANTOM_MEANS[k, c]
        y[c] = (img + PHANTOM_NOISE * rng.standard_normal(PHANTOM_SHAPE)).astype(np.float32)
    return y, (truth > 0).astype(np.uint8), truth, atlas


def dice(a, b, classes):
    out = []
    for c in classes:
        x, y = a == c, b == c
        out.append(2.0 * np.sum(x & y) / (np.sum(x) + np.sum(y)))
    return np.array(out)


def propagated_labels(atlas, mask, classes):
    """What the atlas alone gives inside the mask (a mask voxel the atlas leaves at 0 counts as wrong for every class)."""
    return np.where(mask != 0, atlas, 0).astype(np.int32)


# ---- small random cases ------------------------------------------------------------------------------------------------
def random_case(shape, K, C, seed, holes=True, nan=False, dead=False):
    """Labels, channels, mask and smooth random posteriors of a shape.  `dead`: the last class has no voxel."""
    rng = np.random.default_rng(seed)
    classes = np.arange(1, K + 1, dtype=np.int32) * 3 - 1  # not 1 .. K: the class values are looked up, not assumed
    labels = rng.integers(0, K + (0 if dead else 1), shape).astype(np.int32)
    labels = np.where(labels > 0, classes[np.clip(labels - 1, 0, K - 1)], 0).astype(np.int32)
    y = np.zeros((C,) + tuple(shape), np.float32)
    for c in range(C):
        y[c] = (100.0 + 40.0 * c + 30.0 * (labels % (5 + c)) + 10.0 * rng.standard_normal(shape)).astype(np.float32)
    mask = np.ones(shape, np.uint8)
    if holes:
        mask[rng.random(shape) < 0.2] = 0
    if nan:
        idx = tuple(int(v) // 2 for v in shape)
        y[(C - 1,) + idx] = np.nan
        mask[idx] = 1
    p = rng.random((K,) + tuple(shape)).astype(np.float32)
    p /= p.sum(axis=0, keepdims=True)
    return classes, labels, y, mask, p.astype(np.float32)


def ulp_distance_f32(a, b):
    """Representable float32 values between a and b (0: equal bits up to the sign of zero)."""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# ---- the reference: per-voxel loops straight from the definition ------------------------------------------------------------
def ref_blur(vol, w, axis):
    r = (len(w) - 1) // 2
    vol = np.asarray(vol, np.float32)
    out = np.zeros(vol.shape, np.float32)
    n = vol.shape[axis]
    for idx in np.ndindex(*vol.shape):
        acc = 0.0
        for j in range(2 * r + 1):
            q = idx[axis] + j - r
            if 0 <= q < n:
                src = list(idx)
                src[axis] = q
                acc = acc + float(w[j]) * float(vol[tuple(src)])
        out[idx] = np.float32(acc)
    return out


def ref_priors(labels, classes, taps_zyx):
    wz, wy, wx = taps_zyx
    return np.stack([ref_blur(ref_blur(ref_blur((labels == c).astype(np.float32), wx, 2), wy, 1), wz, 0) for c in classes])


def ref_in_m(y, mask):
    return (np.asarray(mask) != 0) & np.all(np.isfinite(y), axis=0)


def ref_terms(p, y, mask, k):
    """The lists of float64 terms of class k's moments over M, in flat voxel order."""
    C = y.shape[0]
    M = ref_in_m(y, mask).reshape(-1)
    pf, yf = p[k].reshape(-1), y.reshape(C, -1)
    names = [("s0",)] + [("s1", c) for c in range(C)] + [("s2", c, d) for c in range(C) for d in range(c, C)]
    terms = [[] for _ in names]
    where = []
    for i in np.flatnonzero(M):
        pv = float(pf[i])
        yv = [float(yf[c, i]) for c in range(C)]
        row = [pv] + [pv * yv[c] for c in range(C)] + [(pv * yv[c]) * yv[d] for c in range(C) for d in range(c, C)]
        for t, v in zip(terms, row):
            t.append(v)
        where.append(int(i))
    return terms, where


def ref_tree(values, where, n_vox):
    """The tree of the moment sums, literally: lanes, waves, workgroups, passes.  `values[j]` is the term of flat voxel
    `where[j]`; voxels that are not listed are left out."""
    term = dict(zip(where, values))
    nb = -(-n_vox // 1024)
    groups = []
    for b in range(nb):
        lanes = []
        for t in range(256):
            acc = 0.0
            for j in range(4):
                i = 1024 * b + 256 * j + t
                if i < n_vox and i in term:
                    acc = acc + term[i]
            lanes.append(acc)
        waves = []
        for wv in range(4):
            v = lanes[64 * wv:64 * wv + 64]
            for s in (32, 16, 8, 4, 2, 1):
                v = [v[l] + v[l ^ s] for l in range(64)]
            waves.append(v[0])
        groups.append(((waves[0] + waves[1]) + waves[2]) + waves[3])
    vals = groups
    while True:
        out = []
        for b in range(-(-len(vals) // 256)):
            s = [vals[256 * b + t] if 256 * b + t < len(vals) else 0.0 for t in range(256)]
            h = 128
            while h >= 1:
                for t in range(h):
                    s[t] = s[t] + s[t + h]
                h //= 2
            out.append(s[0])
        vals = out
        if len(vals) == 1:
            return vals[0]


def ref_e_step(p_old, pi, y, mask, rows, live, beta):
    """Per voxel, per class, in the order of the definition."""
    K, C = p_old.shape[0], y.shape[0]
    Z, Y, X = y.shape[1:]
    M = ref_in_m(y, mask)
    out = np.zeros(p_old.shape, np.float32)
    nbrs = [(-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (0, 1, 0), (1, 0, 0)]
    for z, yy, x in np.argwhere(M):
        a = {}
        for k in range(K):
            if not live[k]:
                continue
            t = [float(y[c, z, yy, x]) - float(rows[k, c]) for c in range(C)]
            d, m = 0.0, C
            for c in range(C):
                for e in range(c, C):
                    d = d + (((1.0 if c == e else 2.0) * float(rows[k, m])) * t[c]) * t[e]
                    m += 1
            nb = 0.0
            for dz, dy, dx in nbrs:
                q = (z + dz, yy + dy, x + dx)
                if 0 <= q[0] < Z and 0 <= q[1] < Y and 0 <= q[2] < X and M[q]:
                    nb = nb + (1.0 - float(p_old[(k,) + q]))
            a[k] = (float(rows[k, m]) - 0.5 * d) - beta * nb
        top = max(a.values())
        q = {k: float(pi[k, z, yy, x]) * math.exp(a[k] - top) for k in a}
        s = 0.0
        for k in sorted(q):
            s = s + q[k]
        for k in q:
            out[k, z, yy, x] = np.float32(q[k] / s)
    return out


# ---- device shapes: the smallest at which each kernel can still go wrong ------------------------------------------------
# the E-step tile is 4 (z) x 4 (y) x 64 (x); the sums kernel takes 1024 voxels per workgroup, a reduce pass folds 256 of those
ESTEP_SHAPES = [(3, 5, 7), (3, 3, 63), (4, 4, 64), (5, 5, 65), (2, 9, 130)]
SUMS_SHAPES = [(3, 5, 7), (1, 11, 93), (1, 16, 64), (1, 25, 41), (4, 4, 64), (5, 5, 65)]  # 1023, 1024, 1025 voxels among them
TWO_PASS_SHAPE = (65, 64, 64)  # 266240 voxels: 260 workgroups, so a second reduce pass
CLASS_CHANNELS = [(2, 1), (3, 2), (8, 4)]
