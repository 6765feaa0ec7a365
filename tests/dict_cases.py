"""Inputs and references shared by test_dict_host.py and test_dict_gpu.py: small dictionaries and decays with the edge
cases of the dictionary fit, a brute-force matcher in Python floats, and an exact emulation of the ordered float32 fma
chain (what the matrix instruction computes) with the kernel's tile-by-tile candidate rule on top of it."""
import functools

import numpy as np

from fetal_t2mapping_amd import _dict

TE6 = np.array([80.0, 125.0, 170.0, 215.0, 260.0, 305.0])


def echo_times(n_te):
    return 60.0 + 37.0 * np.arange(n_te)


def atoms_for(n_atoms, n_te):
    """Mono-exponential atoms over 20 .. 2000 ms (a single atom: 150 ms)."""
    return _dict.monoexp(echo_times(n_te), _dict.log_grid(20.0, 2000.0, n_atoms) if n_atoms > 1 else [150.0])


def decays(n_te, n_vox, seed, noise=15.0, negate_every=0):
    """Noisy mono-exponential decays, float32 TE-major (n_te, n_vox); every `negate_every`-th voxel negated (all its scores
    are then negative: a padded atom of a ragged tile, which scores 0, would win if it competed)."""
    rng = np.random.default_rng(seed)
    te = echo_times(n_te)
    t2 = np.exp(rng.uniform(np.log(40.0), np.log(1000.0), n_vox))
    k = rng.uniform(300.0, 1500.0, n_vox)
    y = k[None, :] * np.exp(-te[:, None] / t2[None, :]) + noise * rng.standard_normal((n_te, n_vox))
    if negate_every:
        y[:, ::negate_every] = -np.abs(y[:, ::negate_every])
    return y.astype(np.float32)


def holes_mask(n_vox, seed):
    return (np.random.default_rng(seed).random(n_vox) < 0.7).astype(np.uint8)


def brute_force(y, atoms, mask=None):
    """The definition in Python floats (which are float64), one (voxel, atom) pair at a time."""
    a = np.asarray(atoms, np.float32)
    n_atoms, n_te = a.shape
    norm2, dh = [], []
    for j in range(n_atoms):
        s = 0.0
        for e in range(n_te):
            s += float(a[j, e]) * float(a[j, e])
        norm2.append(s)
        dh.append([float(np.float32(float(a[j, e]) / s ** 0.5)) for e in range(n_te)])
    n_vox = y.shape[1]
    index, scale, rmse = np.full(n_vox, -1, np.int32), np.zeros(n_vox, np.float32), np.zeros(n_vox, np.float32)
    for v in range(n_vox):
        yv = [float(y[e, v]) for e in range(n_te)]
        if (mask is not None and not mask[v]) or not all(np.isfinite(yv)):
            continue
        best, bj = None, -1
        for j in range(n_atoms):
            s = 0.0
            for e in range(n_te):
                s += dh[j][e] * yv[e]
            if best is None or s > best:
                best, bj = s, j
        num = 0.0
        for e in range(n_te):
            num += yv[e] * float(a[bj, e])
        q = num / norm2[bj]
        k = q if q > 0 else 0.0
        ss = 0.0
        for e in range(n_te):
            r = yv[e] - k * float(a[bj, e])
            ss += r * r
        index[v], scale[v], rmse[v] = bj, np.float32(k), np.float32((ss / n_te) ** 0.5)
    return index, scale, rmse


# ---- the float32 fma chain, exactly -----------------------------------------------------------------------------------

def fma32(a, b, c):
    """float32(a * b + c) with one rounding, for float32 arrays: the product of two float32 is exact in float64; the float64
    sum is rounded to odd (TwoSum gives its error), which makes the final rounding to float32 the rounding of the exact
    value (53 >= 2 * 24 + 2 bits)."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64)
    fix = (err != 0) & ((bits & 1) == 0) & np.isfinite(s)
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def chain32(dh, y, k_pad):
    """float32 (n_vox, A): s = fma(dh_e, y_e, s) over the echoes in ascending order from 0, padded with zeros to k_pad."""
    s = np.zeros((y.shape[1], dh.shape[0]), np.float32)
    for e in range(k_pad):
        if e < dh.shape[1]:
            s = fma32(np.broadcast_to(dh[None, :, e], s.shape), np.broadcast_to(y[e][:, None], s.shape), s)
        else:
            s = fma32(np.zeros_like(s), np.zeros_like(s), s)
    return s


def candidate_rule(s32, s64, band32, k_pad, chunk_floats=4096):
    """The kernel's rule on given float32 scores: tiles of 32 atoms visited chunk by chunk (chunk c holds the tiles c,
    c + n_chunks, ..), each half of a tile's rows (the two lanes of a voxel) with its own running float32 best, raised by
    the tile's own maximum first; every atom with s32 >= best - T is re-scored (s64) and competes on (score, lowest index).
    Returns (index (n_vox,), number of re-scores per voxel)."""
    n_vox, n_atoms = s32.shape
    n_tiles = (n_atoms + 31) // 32
    tpc = chunk_floats // (k_pad * 32)
    n_chunks = (n_tiles + tpc - 1) // tpc
    rows = [np.array([(r & 3) + 8 * (r >> 2) + 4 * h for r in range(16)]) for h in (0, 1)]
    best32 = np.full((2, n_vox), -np.inf, np.float32)
    best64 = np.full(n_vox, -np.inf)
    bestj = np.full(n_vox, np.iinfo(np.int32).max, np.int64)
    count = np.zeros(n_vox, np.int64)
    for c in range(n_chunks):
        for slot in range(tpc):
            tile = slot * n_chunks + c
            if tile >= n_tiles:
                break
            for h in (0, 1):
                js = tile * 32 + rows[h]
                js = js[js < n_atoms]
                if js.size == 0:
                    continue
                best32[h] = np.maximum(best32[h], s32[:, js].max(axis=1))
                cand = s32[:, js] >= (best32[h] - band32)[:, None]
                count += cand.sum(axis=1)
                for i, j in enumerate(js):
                    s = np.where(cand[:, i], s64[:, j], -np.inf)
                    better = (s > best64) | ((s == best64) & cand[:, i] & (j < bestj))
                    best64, bestj = np.where(better, s, best64), np.where(better, j, bestj)
    return bestj.astype(np.int32), count


@functools.lru_cache(maxsize=None)
def near_tie_case():
    """512 log-spaced atoms, 6 echoes, 2000 noisy voxels: the score is flat at its maximum, so the float32 argmax is not the
    float64 argmax on a few per cent of the voxels.  A kernel without the float64 re-score, or with a band T that is too
    small, cannot reproduce the statement here.  Returns (atoms (512, 6) float32, y (6, 2000) float32, index (2000,))."""
    d = _dict.monoexp(TE6, _dict.log_grid(20.0, 2000.0, 512))
    rng = np.random.default_rng(20260101)
    n_vox = 2000
    t2 = np.exp(rng.uniform(np.log(30.0), np.log(1500.0), n_vox))
    k = rng.uniform(200.0, 2000.0, n_vox)
    y = (k[None, :] * np.exp(-TE6[:, None] / t2[None, :]) + 20.0 * rng.standard_normal((6, n_vox))).astype(np.float32)
    dh, _, dmax = _dict.normalise(d.atoms)
    index = _dict.match(y, d.atoms)[0]
    s64 = _dict.scores(dh, y)
    s32 = chain32(dh, y, 6)
    band = _dict.band(y, dmax, 6)
    band32 = band.astype(np.float32)
    band32 = np.where(band32.astype(np.float64) < band, np.nextafter(band32, np.float32(np.inf)), band32)
    differ = int(np.sum(np.argmax(s32, axis=1) != index))
    assert differ >= 20, f"only {differ} voxels where the float32 chain picks another atom: the case does not bite"
    winner32 = s32[np.arange(n_vox), index]
    assert np.all(winner32.astype(np.float64) >= s32.max(axis=1).astype(np.float64) - band), "the bound T does not hold"
    got, count = candidate_rule(s32, s64, band32, 6)
    assert np.array_equal(got, index), "the tile-by-tile candidate rule misses the float64 argmax"
    y.setflags(write=False)
    index.setflags(write=False)
    return d.atoms, y, index, {"differ": differ, "rescored_mean": float(count.mean()), "rescored_max": int(count.max())}
