"""Inputs and references shared by test_dict_host.py and test_dict_gpu.py: small dictionaries and decays with the edge
cases of the dictionary fit, a brute-force matcher in Python floats, and an exact emulation of the ordered float32 fma
chain (what the matrix instruction computes: tests/test_dict_scores_gpu.py) with the kernel's tile-by-tile candidate rule
on top of it; the near-tie cases, the ties across chunks and the magnitude cases, each built once and read-only."""
import functools

import numpy as np

from fetal_t2mapping_amd import _dict

TE6 = np.array([80.0, 125.0, 170.0, 215.0, 260.0, 305.0])


def echo_times(n_te):
    return 60.0 + 37.0 * np.arange(n_te)


def atoms_for(n_atoms, n_te):
    """Mono-exponential atoms over 20 .. 2000 ms (a single atom: 150 ms)."""
    return _dict.monoexp(echo_times(n_te), _dict.log_grid(20.0, 2000.0, n_atoms) if n_atoms > 1 else [150.0])


def decays(n_te, n_vox, seed, noise=15.0, negate_every=0, scale=1.0):
    """Noisy mono-exponential decays, float32 TE-major (n_te, n_vox); every `negate_every`-th voxel negated (all its scores
    are then negative: a padded atom of a ragged tile, which scores 0, would win if it competed).  `scale` multiplies the
    float64 decays before their one rounding to float32 (1e35: next to the largest float; 1e-40: subnormal samples)."""
    rng = np.random.default_rng(seed)
    te = echo_times(n_te)
    t2 = np.exp(rng.uniform(np.log(40.0), np.log(1000.0), n_vox))
    k = rng.uniform(300.0, 1500.0, n_vox)
    y = k[None, :] * np.exp(-te[:, None] / t2[None, :]) + noise * rng.standard_normal((n_te, n_vox))
    if negate_every:
        y[:, ::negate_every] = -np.abs(y[:, ::negate_every])
    return (y * scale).astype(np.float32)


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


def chunks_of(n_atoms, n_te, chunk_floats=4096):
    """(tiles of a chunk, number of chunks) of the kernel's walk over a table."""
    k_pad = n_te + n_te % 2
    tpc = chunk_floats // (k_pad * 32)
    n_tiles = (n_atoms + 31) // 32
    return tpc, (n_tiles + tpc - 1) // tpc


def band32_of(y, dmax, k_pad):
    """The band T as float32 (n_vox,): _dict.band rounded up to float32."""
    band = _dict.band(y, dmax, k_pad)
    band32 = band.astype(np.float32)
    return band, np.where(band32.astype(np.float64) < band, np.nextafter(band32, np.float32(np.inf)), band32)


# (atoms, echoes, voxels, seed) of the near-tie cases whose tables need several chunks; atoms_for() and decays(noise=20).
# Chunks 2, 7, 9, 16, 32; 17 and 32 echoes run two groups per wave; 65536 atoms is T2FIT_DICT_MAX_ATOMS.
MULTI_CHUNK_CASES = ((1000, 6, 600, 1), (4096, 6, 400, 4), (2000, 17, 400, 9), (2000, 32, 400, 8), (65536, 2, 96, 11))


@functools.lru_cache(maxsize=None)
def near_tie_case(n_atoms=512, n_te=6, n_vox=2000, seed=None):
    """Log-spaced atoms and noisy voxels: the score is flat at its maximum, so the float32 argmax is not the float64 argmax
    on a few per cent of the voxels.  A kernel without the float64 re-score, or with a band T that is too small, cannot
    reproduce the statement here.  Without a seed: the first case (512 atoms at TE6, 2000 voxels, one chunk).  With a seed:
    atoms_for(n_atoms, n_te) and decays(n_te, n_vox, seed, noise=20); such a case must need at least two chunks, and the
    rule with T = 0 must miss the statement's atom somewhere.  Returns (atoms (A, n_te) float32, y (n_te, n_vox) float32,
    index (n_vox,), figures)."""
    if seed is None:
        assert (n_atoms, n_te, n_vox) == (512, 6, 2000)
        atoms = _dict.monoexp(TE6, _dict.log_grid(20.0, 2000.0, 512)).atoms
        rng = np.random.default_rng(20260101)
        t2 = np.exp(rng.uniform(np.log(30.0), np.log(1500.0), n_vox))
        k = rng.uniform(200.0, 2000.0, n_vox)
        y = (k[None, :] * np.exp(-TE6[:, None] / t2[None, :]) + 20.0 * rng.standard_normal((6, n_vox))).astype(np.float32)
    else:
        atoms = atoms_for(n_atoms, n_te).atoms
        y = decays(n_te, n_vox, seed, noise=20.0)
    k_pad = n_te + n_te % 2
    n_chunks = chunks_of(n_atoms, n_te)[1]
    dh, _, dmax = _dict.normalise(atoms)
    index = _dict.match(y, atoms)[0]
    s64 = _dict.scores(dh, y)
    s32 = chain32(dh, y, k_pad)
    band, band32 = band32_of(y, dmax, k_pad)
    differ = int(np.sum(np.argmax(s32, axis=1) != index))
    assert differ >= 20, f"only {differ} voxels where the float32 chain picks another atom: the case does not bite"
    winner32 = s32[np.arange(n_vox), index]
    assert np.all(winner32.astype(np.float64) >= s32.max(axis=1).astype(np.float64) - band), "the bound T does not hold"
    got, count = candidate_rule(s32, s64, band32, k_pad)
    assert np.array_equal(got, index), "the tile-by-tile candidate rule misses the float64 argmax"
    info = {"differ": differ, "rescored_mean": float(count.mean()), "rescored_max": int(count.max()), "n_chunks": n_chunks}
    if seed is not None:
        assert n_chunks >= 2, f"{n_atoms} atoms of {n_te} echoes fit one chunk"
        t0 = candidate_rule(s32, s64, np.zeros(n_vox, np.float32), k_pad)[0]
        info["t0_misses"] = int(np.sum(t0 != index))
        assert info["t0_misses"] >= 1, "the rule with T = 0 reproduces the statement: the case does not need the band"
    y.setflags(write=False)
    index.setflags(write=False)
    return atoms, y, index, info


# ---- ties across chunks -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cross_chunk_tie_case():
    """300 atoms of 32 echoes: 10 tiles, 4 to a chunk, so chunk 0 holds the tiles 0, 3, 6, 9 (9 is the ragged last tile: 12
    atoms), chunk 1 the tiles 1, 4, 7 and chunk 2 the tiles 2, 5, 8; the walk leaves the chunks 1 and 2 after three slots.
    Atom 40 (tile 1) is copied to 104 (tile 3, the same row and lane half): the copy is met first, a chunk earlier, and only
    the lower index of two equal scores brings 40 back.  Atom 110 (tile 3) is copied to 142 (tile 4): the lower index is met
    first and must stay.  Four voxels are exact multiples of atoms: of 40, of 110, of 295 (ragged last tile) and of 287 (last
    row of the last slot of chunk 2, after which the walk ends).  The other voxels are noisy decays.
    Returns (atoms, y, index of the statement, {name: (voxel, atom)})."""
    atoms = atoms_for(300, 32).atoms.copy()
    assert chunks_of(300, 32) == (4, 3)
    atoms[104] = atoms[40]
    atoms[142] = atoms[110]
    named = {"copy_met_first": (3, 40), "lower_met_first": (17, 110), "ragged_last_tile": (34, 295), "last_slot_before_the_break": (50, 287)}
    y = decays(32, 70, seed=41, noise=20.0)
    for (v, j), factor in zip(named.values(), (4.0, 0.5, 2.0, 8.0)):  # powers of two: the multiples are exact in float32
        y[:, v] = factor * atoms[j]
    dh, _, dmax = _dict.normalise(atoms)
    index = _dict.match(y, atoms)[0]
    for name, (v, j) in named.items():
        assert index[v] == j, (name, int(index[v]), j)
    s64 = _dict.scores(dh, y)
    assert s64[3, 40] == s64[3, 104] and s64[17, 110] == s64[17, 142]  # the ties are exact
    got, _ = candidate_rule(chain32(dh, y, 32), s64, band32_of(y, dmax, 32)[1], 32)
    assert np.array_equal(got, index), "the tile-by-tile candidate rule misses the float64 argmax"
    y.setflags(write=False)
    index.setflags(write=False)
    return atoms, y, index, named


# ---- magnitudes ---------------------------------------------------------------------------------------------------------

TINY_SCALES = (1e-38, 1e-40, 1e-41)
SMALLEST_NORMAL = 2.0 ** -126


def _statement_without_warnings(y, atoms):
    with np.errstate(over="raise", invalid="raise", divide="raise"):
        return _dict.match(y, atoms)


@functools.lru_cache(maxsize=None)
def huge_case():
    """Samples next to the largest float32 on the 512 x 6 table times 8 (so that the scale stays finite): on a share of the
    voxels between 20 % and 80 %, |y| dmax >= 1e38, where the kernel's band is infinite and every atom is re-scored; the
    others of the same groups keep a finite band.  Returns (atoms, y, share)."""
    atoms = (atoms_for(512, 6).atoms * np.float32(8.0)).astype(np.float32)
    y = decays(6, 300, seed=51, scale=1e35)
    assert np.all(np.isfinite(y))
    dmax = _dict.normalise(atoms)[2]
    nn = np.zeros(y.shape[1])
    for e in range(6):
        nn = nn + y[e].astype(np.float64) * y[e].astype(np.float64)
    share = float(np.mean(np.sqrt(nn) * float(dmax) >= 1e38))
    assert 0.2 <= share <= 0.8, share
    _, scale, rmse = _statement_without_warnings(y, atoms)
    assert np.all(np.isfinite(scale)) and np.all(np.isfinite(rmse)) and scale.max() > 1e36
    y.setflags(write=False)
    return atoms, y, share


@functools.lru_cache(maxsize=None)
def tiny_case(scale):
    """Samples scaled by 1e-38, 1e-40 or 1e-41 on the 512 x 6 table: none, some and nearly all of them subnormal.  From
    1e-40 down the rmse itself (noise 15 times the scale) is a subnormal float32 on some voxel, which is asserted: a
    subnormal output is compared.  Returns (atoms, y, {share of subnormal samples, voxels with a subnormal rmse})."""
    atoms = atoms_for(512, 6).atoms
    y = decays(6, 200, seed=52, scale=scale)
    sub = float(np.mean((y != 0) & (np.abs(y) < np.float32(SMALLEST_NORMAL))))
    rmse = _dict.match(y, atoms)[2]
    n_sub_rmse = int(np.sum((rmse > 0) & (rmse < np.float32(SMALLEST_NORMAL))))
    if scale <= 1e-40:
        assert sub > 0.05 and n_sub_rmse >= 1, (scale, sub, n_sub_rmse)
    else:
        assert sub < 0.01, (scale, sub)  # (a sample of a fast decay's last echoes at the most)
    y.setflags(write=False)
    return atoms, y, {"subnormal_samples": sub, "subnormal_rmse": n_sub_rmse}


F32_MAX = float(np.finfo(np.float32).max)


@functools.lru_cache(maxsize=None)
def special_rows_case():
    """Noisy decays on the 512 x 6 table with six rows replaced: all -0.0; zeros and one subnormal sample; zeros and one
    negative subnormal sample; float32 max / 8 in every echo; -+ float32 max / 8 in alternation (every score negative: scale
    0); +- float32 max / 8 in alternation (the fastest decay matches, and its scale is beyond float32: the statement rounds
    it to inf, and so must the device).  Returns (atoms, y, rows)."""
    atoms = atoms_for(512, 6).atoms
    y = decays(6, 80, seed=53)
    rows = {"minus_zero": 5, "one_subnormal": 9, "one_negative_subnormal": 38, "max_over_8": 13, "minus_plus_max_over_8": 44,
            "plus_minus_max_over_8": 71}
    y[:, rows["minus_zero"]] = -0.0
    y[:, rows["one_subnormal"]] = 0.0
    y[3, rows["one_subnormal"]] = 3 * 2.0 ** -149
    y[:, rows["one_negative_subnormal"]] = 0.0
    y[0, rows["one_negative_subnormal"]] = -(2.0 ** -149)
    y[:, rows["max_over_8"]] = F32_MAX / 8
    y[:, rows["minus_plus_max_over_8"]] = np.array([-1, 1, -1, 1, -1, 1]) * (F32_MAX / 8)
    y[:, rows["plus_minus_max_over_8"]] = np.array([1, -1, 1, -1, 1, -1]) * (F32_MAX / 8)
    assert np.all(np.signbit(y[:, 5])) and y[3, 9] > 0 and y[3, 9] < np.float32(SMALLEST_NORMAL) and np.all(np.isfinite(y))
    with np.errstate(over="ignore"):
        index, scale, rmse = _dict.match(y, atoms)
    assert index[5] == 0 and scale[5] == 0 and rmse[5] == 0 and not np.signbit(scale[5]) and not np.signbit(rmse[5])
    assert index[9] >= 0 and scale[38] == 0 and scale[44] == 0 and rmse[44] == np.float32(F32_MAX / 8) and scale[13] > 1e37
    assert np.isinf(scale[71]) and np.all(np.isfinite(np.delete(scale, 71))) and np.all(index >= 0)
    y.setflags(write=False)
    return atoms, y, rows


def scaled_atoms(factor):
    """The 512 x 6 table times 1e-18 or 1e18: atoms far from unit norm, whose squared norms stay finite and non-zero."""
    atoms = (atoms_for(512, 6).atoms.astype(np.float64) * factor).astype(np.float32)
    n2 = _dict.normalise(atoms)[1]
    assert np.all(np.isfinite(n2)) and np.all(n2 > 0) and np.all(atoms != 0)
    return atoms


