"""Dictionary-matching fit, stated in numpy: what ``t2fit_dict_pack_host`` writes and what ``t2fit_dict_match_dev`` computes
(include/t2fit.h), plus the dictionary builders that the device path shares.  Everything is float64 with one rounding per
operation in the order written; sums over the echoes run in ascending order from 0.0.  Used by the tests as the definition
and by nobody on the hot path."""
from __future__ import annotations

import struct
from dataclasses import dataclass

import numpy as np

MAX_ATOMS, MAX_TE, TILE = 65536, 32, 32
MAGIC = 0x54443254
HEADER_BYTES = 64


# ---- dictionaries -----------------------------------------------------------------------------------------------------

@dataclass
class Dictionary:
    """A signal model as a table: ``atoms`` float32 ``(A, nTE)`` (unnormalised decay curves), ``params`` float32 ``(A, P)``
    (what each atom stands for) and ``names``, the P column names.  A ``t2`` column is what ``fit_volume_dict`` maps to T2."""
    atoms: np.ndarray
    params: np.ndarray
    names: tuple

    def __post_init__(self):
        self.atoms = np.ascontiguousarray(self.atoms, dtype=np.float32)
        self.params = np.ascontiguousarray(self.params, dtype=np.float32)
        self.names = tuple(str(n) for n in self.names)
        if self.atoms.ndim != 2:
            raise ValueError(f"atoms must be (A, nTE), got shape {self.atoms.shape}")
        if self.params.ndim != 2 or self.params.shape[0] != self.atoms.shape[0]:
            raise ValueError(f"params must be (A, P) with A = {self.atoms.shape[0]}, got shape {self.params.shape}")
        if len(self.names) != self.params.shape[1] or len(set(self.names)) != len(self.names):
            raise ValueError(f"names must be {self.params.shape[1]} distinct column names, got {self.names}")
        check_atoms(self.atoms)

    @property
    def n_atoms(self):
        return self.atoms.shape[0]

    @property
    def n_te(self):
        return self.atoms.shape[1]

    def column(self, name):
        if name not in self.names:
            raise KeyError(f"the dictionary has no column {name!r} (it has {', '.join(self.names)})")
        return self.params[:, self.names.index(name)]

    def save(self, path):
        """One ``.npz``: ``atoms``, ``params``, ``names``."""
        with open(path, "wb") as f:
            np.savez(f, atoms=self.atoms, params=self.params, names=np.array(self.names))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as d:
            return cls(d["atoms"], d["params"], tuple(str(n) for n in d["names"]))


def log_grid(lo, hi, n):
    """``n`` values from ``lo`` to ``hi`` (both included), evenly spaced in the logarithm; float64."""
    lo, hi, n = float(lo), float(hi), int(n)
    if not (0 < lo <= hi) or n < 1 or (n == 1 and lo != hi):
        raise ValueError(f"log_grid needs 0 < lo <= hi and n >= 1 (n >= 2 when lo < hi), got {lo}, {hi}, {n}")
    if n == 1:
        return np.array([lo])
    g = np.exp(np.log(lo) + (np.log(hi) - np.log(lo)) * np.arange(n) / (n - 1))
    g[0], g[-1] = lo, hi
    return g


def monoexp(te, t2_values):
    """``exp(-te / T2)`` for every T2: one column, ``t2``."""
    te = np.asarray(te, np.float64).reshape(-1)
    t2 = np.asarray(t2_values, np.float64).reshape(-1)
    return Dictionary(np.exp(-te[None, :] / t2[:, None]).astype(np.float32), t2[:, None].astype(np.float32), ("t2",))


def biexp(te, t2_values, t2_long, fractions):
    """``(1 - f) exp(-te / T2) + f exp(-te / T2_long)`` for every (T2, f), T2 outermost: columns ``t2``, ``fraction``.  The
    long component (CSF) is fixed; ``fractions`` lie in [0, 1)."""
    te = np.asarray(te, np.float64).reshape(-1)
    t2 = np.asarray(t2_values, np.float64).reshape(-1)
    fr = np.asarray(fractions, np.float64).reshape(-1)
    if not (float(t2_long) > 0) or np.any(fr < 0) or np.any(fr >= 1):
        raise ValueError("biexp needs t2_long > 0 and fractions in [0, 1)")
    tt, ff = (a.reshape(-1) for a in np.meshgrid(t2, fr, indexing="ij"))
    atoms = (1.0 - ff)[:, None] * np.exp(-te[None, :] / tt[:, None]) + ff[:, None] * np.exp(-te[None, :] / float(t2_long))
    return Dictionary(atoms.astype(np.float32), np.stack([tt, ff], axis=1).astype(np.float32), ("t2", "fraction"))


# ---- packing ----------------------------------------------------------------------------------------------------------

def check_atoms(atoms):
    """The refusals of ``t2fit_dict_pack_host``; returns the atoms as contiguous float32 ``(A, nTE)``."""
    a = np.ascontiguousarray(atoms, dtype=np.float32)
    if a.ndim != 2 or not (1 <= a.shape[0] <= MAX_ATOMS) or not (2 <= a.shape[1] <= MAX_TE):
        raise ValueError(f"a dictionary is (A, nTE) with A in 1 .. {MAX_ATOMS} and nTE in 2 .. {MAX_TE}, got shape {a.shape}")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"atom {int(np.flatnonzero(~np.isfinite(a).all(axis=1))[0])} has a non-finite sample")
    if not np.all(np.any(a != 0, axis=1)):
        raise ValueError(f"atom {int(np.flatnonzero(~np.any(a != 0, axis=1))[0])} has norm 0")
    return a


def layout(n_atoms, n_te):
    """``(k_pad, n_tiles, off_tiles, off_atoms, off_norm2, bytes)`` of the packed block."""
    up16 = lambda v: (v + 15) // 16 * 16
    k_pad, n_tiles = (n_te + 1) // 2 * 2, (n_atoms + TILE - 1) // TILE
    off_tiles = HEADER_BYTES
    off_atoms = off_tiles + n_tiles * k_pad * TILE * 4
    off_norm2 = off_atoms + up16(n_atoms * n_te * 4)
    return k_pad, n_tiles, off_tiles, off_atoms, off_norm2, off_norm2 + up16(n_atoms * 8)


def normalise(atoms):
    """``(Dh float32 (A, nTE), n2 float64 (A,), dmax float32)``: the normalised atoms, the squared norms of the atoms as given,
    the largest norm of a normalised atom."""
    a = check_atoms(atoms)
    d = a.astype(np.float64)
    n2 = np.zeros(a.shape[0])
    for e in range(a.shape[1]):
        n2 = n2 + d[:, e] * d[:, e]
    dh = (d / np.sqrt(n2)[:, None]).astype(np.float32)
    h = dh.astype(np.float64)
    h2 = np.zeros(a.shape[0])
    for e in range(a.shape[1]):
        h2 = h2 + h[:, e] * h[:, e]
    return dh, n2, np.float32(np.max(np.sqrt(h2)))


def pack(atoms):
    """The packed dictionary as ``uint8`` bytes, byte for byte what ``t2fit_dict_pack_host`` writes (layout: include/t2fit.h)."""
    a = check_atoms(atoms)
    n_atoms, n_te = a.shape
    dh, n2, dmax = normalise(a)
    k_pad, n_tiles, off_tiles, off_atoms, off_norm2, nbytes = layout(n_atoms, n_te)
    out = np.zeros(nbytes, np.uint8)
    out[:HEADER_BYTES] = np.frombuffer(struct.pack("<IiiiifIIQQQQ", MAGIC, n_atoms, n_te, k_pad, n_tiles, float(dmax), 0, 0, off_tiles,
                                                   off_atoms, off_norm2, nbytes), np.uint8)
    tiles = np.zeros((n_tiles * TILE, k_pad), np.float32)
    tiles[:n_atoms, :n_te] = dh
    tiles = tiles.reshape(n_tiles, TILE, k_pad).transpose(0, 2, 1)  # [tile][echo][row]
    out[off_tiles:off_atoms] = np.ascontiguousarray(tiles).view(np.uint8).reshape(-1)
    out[off_atoms:off_atoms + a.nbytes] = a.view(np.uint8).reshape(-1)
    out[off_norm2:off_norm2 + n2.nbytes] = n2.view(np.uint8).reshape(-1)
    return out


# ---- matching ---------------------------------------------------------------------------------------------------------

def samples(echoes, n_te):
    """Echoes ``(nTE, ...)`` -> float32 ``(nTE, n_vox)`` and the spatial shape."""
    y = np.ascontiguousarray(echoes, dtype=np.float32)
    if y.ndim < 1 or y.shape[0] != n_te:
        raise ValueError(f"the echoes are TE-major with {y.shape[0] if y.ndim else 0} echoes, the dictionary has {n_te}")
    return y.reshape(n_te, -1), y.shape[1:]


def scores(dh, y):
    """float64 ``(n_vox, A)``: ``s_j = sum_e Dh_je y_e``, plain multiply and add in ascending e."""
    h, y = dh.astype(np.float64), y.astype(np.float64)
    s = np.zeros((y.shape[1], h.shape[0]))
    for e in range(h.shape[1]):
        s = s + h[None, :, e] * y[e][:, None]
    return s


def band(y, dmax, k_pad):
    """float64 ``(n_vox,)``: ``T = 2 (K + 2) 2^-24 |y|_2 dmax (1 + 2^-20)`` (the device rounds it up to
    float32 and never lets it fall below 2^-126)."""
    y = y.astype(np.float64)
    nn = np.zeros(y.shape[1])
    for e in range(y.shape[0]):
        nn = nn + y[e] * y[e]
    return 2.0 * (k_pad + 2) * 2.0 ** -24 * np.sqrt(nn) * float(dmax) * (1.0 + 2.0 ** -20)


def match(echoes, atoms, mask=None, chunk=4096):
    """``(index int32, scale float32, rmse float32)``, each of the echoes' spatial shape: the definition of
    ``t2fit_dict_match_dev``.  ``atoms``: a :class:`Dictionary` or a float32 ``(A, nTE)`` array."""
    a = check_atoms(atoms.atoms if isinstance(atoms, Dictionary) else atoms)
    n_atoms, n_te = a.shape
    y, spatial = samples(echoes, n_te)
    n_vox = y.shape[1]
    ok = np.all(np.isfinite(y), axis=0)
    if mask is not None:
        m = np.asarray(mask).reshape(-1) != 0
        if m.size != n_vox:
            raise ValueError("mask shape does not match the echoes")
        ok &= m
    dh, n2, _ = normalise(a)
    index = np.full(n_vox, -1, np.int32)
    scale = np.zeros(n_vox, np.float32)
    rmse = np.zeros(n_vox, np.float32)
    rows = np.flatnonzero(ok)
    d = a.astype(np.float64)
    for lo in range(0, rows.size, chunk):
        r = rows[lo:lo + chunk]
        yc = y[:, r]
        j = np.argmax(scores(dh, yc), axis=1)  # (the first of equal maxima: the lowest index)
        y64, dj = yc.astype(np.float64), d[j]
        num = np.zeros(r.size)
        for e in range(n_te):
            num = num + y64[e] * dj[:, e]
        q = num / n2[j]
        k = np.where(q > 0, q, 0.0)
        ss = np.zeros(r.size)
        for e in range(n_te):
            res = y64[e] - k * dj[:, e]
            ss = ss + res * res
        index[r], scale[r], rmse[r] = j, k.astype(np.float32), np.sqrt(ss / float(n_te)).astype(np.float32)
    return index.reshape(spatial), scale.reshape(spatial), rmse.reshape(spatial)


def lookup(dictionary, index):
    """``{name: float32 map}``: the parameter columns read off the table at ``index`` (numpy int array); 0 where index < 0."""
    idx = np.asarray(index)
    safe = np.where(idx >= 0, idx, 0)
    return {n: np.where(idx >= 0, dictionary.params[:, c][safe], np.float32(0)).astype(np.float32) for c, n in enumerate(dictionary.names)}
