"""Gibbs-ringing removal by local sub-voxel shifts (Kellner et al. 2016), stated in numpy: what ``t2fit_unring_tables_host``
writes and what ``t2fit_unring_split_dev``, ``t2fit_unring_rows_dev`` and ``t2fit_unring_dev`` compute (include/t2fit.h).
The tables are float64 rounded once to float32.  Every product of a table and data is a float32 fma chain over the
contracted index, ascending, from 0.0f (:func:`chain`: what ``v_mfma_f32_32x32x2_f32`` does); everything else is float32
with one rounding per operation, nothing fused.  Used by the tests as the definition and by nobody on the hot path."""
from __future__ import annotations

import struct

import numpy as np

MIN_N, MAX_N, MAX_K, MAX_W = 8, 512, 32, 8
MAGIC = 0x52553254
HEADER_BYTES = 128
DEFAULT_K, DEFAULT_MIN_W, DEFAULT_MAX_W = 20, 1, 3


def check_params(ny, nx, K=DEFAULT_K, min_w=DEFAULT_MIN_W, max_w=DEFAULT_MAX_W):
    """The refusals of the library for sizes and parameters."""
    ny, nx, K, min_w, max_w = int(ny), int(nx), int(K), int(min_w), int(max_w)
    if not (MIN_N <= nx <= MAX_N and MIN_N <= ny <= MAX_N):
        raise ValueError(f"unring: nx and ny must be {MIN_N} .. {MAX_N}, got nx {nx} and ny {ny}")
    if not 1 <= K <= MAX_K:
        raise ValueError(f"unring: K (shifts per side) must be 1 .. {MAX_K}, got {K}")
    if not 1 <= min_w <= max_w <= MAX_W:
        raise ValueError(f"unring: the window must be 1 <= min_w <= max_w <= {MAX_W}, got {min_w}, {max_w}")
    if min(nx, ny) < 2 * (max_w + 1) + 1:
        raise ValueError(f"unring: the window {min_w}, {max_w} needs rows of at least {2 * (max_w + 1) + 1} samples, got nx {nx} and ny {ny}")
    return ny, nx, K, min_w, max_w


# ---- tables -----------------------------------------------------------------------------------------------------------

def shifts(K):
    """float64 ``(2K+1,)``: s_0 = 0, s_j = j / (2K+1), s_{K+j} = -j / (2K+1) for j = 1 .. K."""
    j = np.arange(1, K + 1, dtype=np.float64)
    return np.concatenate([[0.0], j / (2 * K + 1), -j / (2 * K + 1)])


def dft_tables(n):
    """float32 ``(n, n)`` each: C[k, m] = cos(2 pi ((k m) mod n) / n) and S likewise."""
    km = (np.arange(n, dtype=np.int64)[:, None] * np.arange(n, dtype=np.int64)[None, :]) % n
    arg = 2.0 * np.pi * km.astype(np.float64) / n
    return np.cos(arg).astype(np.float32), np.sin(arg).astype(np.float32)


def filter_table(ny, nx):
    """float32 ``(ny, nx)``: G = cy / (cx + cy) (0.5 where cx + cy = 0), stored as float32(G / (nx ny))."""
    cx = 1.0 + np.cos(2.0 * np.pi * np.arange(nx, dtype=np.float64) / nx)[None, :]
    cy = 1.0 + np.cos(2.0 * np.pi * np.arange(ny, dtype=np.float64) / ny)[:, None]
    den = cx + cy
    g = np.where(den == 0.0, 0.5, cy / np.where(den == 0.0, 1.0, den))
    return (g / float(nx * ny)).astype(np.float32)


def taps(n, K):
    """float32 ``(2K+1, n)``: h_j[d] = (1/n) [1 + 2 sum_{k=1}^{ceil(n/2)-1} cos(2 pi k (d + s_j) / n) + (n even) cos(pi d) cos(pi s_j)];
    row 0 is the identity (1, 0, 0, ..), which no product reads."""
    s = shifts(K)
    d = np.arange(n, dtype=np.float64)
    u = d[None, :] + s[:, None]
    acc = np.ones((2 * K + 1, n))
    for k in range(1, (n + 1) // 2):
        acc = acc + 2.0 * np.cos(2.0 * np.pi * k * u / n)
    if n % 2 == 0:
        acc = acc + np.cos(np.pi * d)[None, :] * np.cos(np.pi * s)[:, None]
    h = (acc / n).astype(np.float32)
    h[0] = 0.0
    h[0, 0] = 1.0
    return h


def weights(K):
    """float32 ``(2, 2K+1)``: a_j = float32(1 - |s_j|), b_j = float32(|s_j|)."""
    s = np.abs(shifts(K))
    return np.stack([(1.0 - s).astype(np.float32), s.astype(np.float32)])


class Tables:
    """The tables of one (ny, nx, K): ``cx, sx`` (nx, nx), ``cy, sy`` (ny, ny), ``g`` (ny, nx), ``hx`` (2K+1, nx), ``hy``
    (2K+1, ny), ``ab`` (2, 2K+1), all float32; :meth:`pack` is the block the device calls read."""

    def __init__(self, ny, nx, K=DEFAULT_K):
        self.ny, self.nx, self.K = check_params(ny, nx, K, 1, 1)[:3]
        self.cx, self.sx = dft_tables(self.nx)
        self.cy, self.sy = dft_tables(self.ny)
        self.g = filter_table(self.ny, self.nx)
        self.hx, self.hy = taps(self.nx, self.K), taps(self.ny, self.K)
        self.ab = weights(self.K)

    def parts(self):
        return [("cx", self.cx), ("sx", self.sx), ("cy", self.cy), ("sy", self.sy), ("g", self.g), ("hx", self.hx), ("hy", self.hy),
                ("ab", self.ab)]

    def pack(self):
        """``uint8`` bytes, little endian (layout: include/t2fit.h): the 128-byte header, then the tables in the order of
        :meth:`parts`, each padded to a multiple of 16 bytes."""
        offs, off = [], HEADER_BYTES
        for _, a in self.parts():
            offs.append(off)
            off += (a.nbytes + 15) // 16 * 16
        out = np.zeros(off, np.uint8)
        out[:HEADER_BYTES] = np.frombuffer(struct.pack("<Iiii16x8QQ24x", MAGIC, self.nx, self.ny, self.K, *offs, off), np.uint8)
        for o, (_, a) in zip(offs, self.parts()):
            out[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        return out

    @classmethod
    def unpack(cls, blob):
        """The tables out of a packed block (of :meth:`pack` or of ``t2fit_unring_tables_host``)."""
        blob = np.ascontiguousarray(blob, np.uint8)
        f = struct.unpack("<Iiii16x8QQ24x", blob[:HEADER_BYTES].tobytes())
        if f[0] != MAGIC or f[-1] != blob.size:
            raise ValueError("not a packed unring table block")
        t = cls.__new__(cls)
        t.nx, t.ny, t.K = f[1], f[2], f[3]
        nj = 2 * t.K + 1
        shapes = [(t.nx, t.nx), (t.nx, t.nx), (t.ny, t.ny), (t.ny, t.ny), (t.ny, t.nx), (nj, t.nx), (nj, t.ny), (2, nj)]
        for name, off, shape in zip(("cx", "sx", "cy", "sy", "g", "hx", "hy", "ab"), f[4:12], shapes):
            n = int(np.prod(shape))
            setattr(t, name, blob[off:off + 4 * n].view(np.float32).reshape(shape).copy())
        return t


# ---- the float32 fma chain --------------------------------------------------------------------------------------------

def fma32(a, b, c):
    """float32(a * b + c) with one rounding, for float32 arrays: the product is exact in float64; the float64 sum is rounded to
    odd (TwoSum gives its error), so the final rounding to float32 is the rounding of the exact value."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    fix = (err != 0) & ((s.view(np.int64) & 1) == 0) & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def chain(table, data):
    """``table`` float32 (M, L), ``data`` float32 (..., L, N) -> float32 (..., M, N): out[m, c] = fma(table[m, k], data[k, c], out[m, c])
    for k = 0, 1, .., L-1 from 0.0f.  (An odd L is padded with an exact zero on the device: fma(0, 0, c) = c.)"""
    table, data = np.asarray(table, np.float32), np.asarray(data, np.float32)
    out = np.zeros(data.shape[:-2] + (table.shape[0], data.shape[-1]), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(table.shape[1]):
            out = fma32(np.broadcast_to(table[:, k, None], out.shape), np.broadcast_to(data[..., k, None, :], out.shape), out)
    return out


# ---- step 1: split ----------------------------------------------------------------------------------------------------

def split(x, tables):
    """``(I1, I2)`` float32 ``(S, ny, nx)``.  With P, Q, .. planes indexed [y or ky][x or kx] and the stacked operands always
    (cosine or real part first, sine or imaginary part second):
      row DFT      [P; Q][kx, y] = [Cx; Sx] . X^T                       (F = P - i Q; contracted: x)
      column DFT   [A; B] = [[Cy, -Sy], [Sy, Cy]] . [P; Q]              (F2 = A - i B; contracted: (part, y), P's rows first)
      filter       A, B <- fl(A G), fl(B G)
      inverse      [Vr; Vi] = [[Cy, Sy], [Sy, -Cy]] . [A; B]            (contracted: (part, ky))
      real part    I1[x, y] = [Cx, -Sx] . [Vr; Vi]^T                    (contracted: (part, kx))
      I2 = fl(X - I1)."""
    x = np.asarray(x, np.float32)
    t = tables
    if x.ndim != 3 or x.shape[1:] != (t.ny, t.nx):
        raise ValueError(f"split takes float32 (S, {t.ny}, {t.nx}), got shape {x.shape}")
    pq = chain(np.concatenate([t.cx, t.sx]), x.transpose(0, 2, 1))                      # (S, 2nx, ny): [part][kx][y]
    pq = np.concatenate([pq[:, :t.nx].transpose(0, 2, 1), pq[:, t.nx:].transpose(0, 2, 1)], axis=1)  # (S, 2ny, nx): [part][y][kx]
    ab = chain(np.block([[t.cy, -t.sy], [t.sy, t.cy]]), pq)                              # (S, 2ny, nx): [part][ky][kx]
    ab = ab * np.concatenate([t.g, t.g])[None]
    v = chain(np.block([[t.cy, t.sy], [t.sy, -t.cy]]), ab)                               # (S, 2ny, nx): [part][y][kx]
    v = np.concatenate([v[:, :t.ny].transpose(0, 2, 1), v[:, t.ny:].transpose(0, 2, 1)], axis=1)     # (S, 2nx, ny): [part][kx][y]
    i1 = np.ascontiguousarray(chain(np.concatenate([t.cx, -t.sx], axis=1), v).transpose(0, 2, 1))
    return i1, x - i1


# ---- step 2: rows -----------------------------------------------------------------------------------------------------

def circulant(h):
    """(J, n) taps -> (J, n, n): H_j[l, m] = h_j[(l - m) mod n]."""
    n = h.shape[1]
    idx = (np.arange(n)[:, None] - np.arange(n)[None, :]) % n
    return h[:, idx]


def shifted(rows, h):
    """float32 ``(J, R, n)``: Y_j of every row (R, n) for the taps h (J, n): the chain over m ascending."""
    rows = np.asarray(rows, np.float32)
    hc = circulant(np.asarray(h, np.float32))
    return np.stack([chain(hc[j], rows.T).T for j in range(hc.shape[0])])


def tv_of(y, min_w, max_w):
    """float32, the shape of y: min(tvl, tvr) along the last axis, circular, both sums ascending in t from 0.0f."""
    d = np.abs(y - np.roll(y, 1, axis=-1))
    tvl, tvr = np.zeros_like(d), np.zeros_like(d)
    for t in range(min_w, max_w + 1):
        tvl = tvl + np.roll(d, t, axis=-1)         # d[l - t]
        tvr = tvr + np.roll(d, -(t + 1), axis=-1)  # d[l + t + 1]
    return np.minimum(tvl, tvr)


def unring_rows(rows, h, ab, min_w=DEFAULT_MIN_W, max_w=DEFAULT_MAX_W):
    """``(out float32, shift int8, tv float32)``, each (R, n): the rows (R, n) unrung along their length with the taps h
    (2K+1, n) and the weights ab (2, 2K+1).  Shifts are visited in the order j = 0, 1, .., 2K; a shift replaces the running best
    only when its tv is strictly smaller."""
    rows = np.asarray(rows, np.float32)
    nj = h.shape[0]
    K = (nj - 1) // 2
    out, best = rows.copy(), tv_of(rows, min_w, max_w)
    shift = np.zeros(rows.shape, np.int8)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(1, nj):
            y = shifted(rows, h[j:j + 1])[0]
            tv = tv_of(y, min_w, max_w)
            other = np.roll(y, 1, axis=-1) if j <= K else np.roll(y, -1, axis=-1)  # Y_j[l - 1] for s_j > 0, Y_j[l + 1] for s_j < 0
            val = y * ab[0, j] + other * ab[1, j]
            better = tv < best
            out, best, shift = np.where(better, val, out), np.where(better, tv, best), np.where(better, np.int8(j), shift)
    return out, shift, best


def skipped_slices(x):
    """bool (S,), bool (S,): the slices with a non-finite sample (copied and counted), and those whose samples are all equal
    (copied, not counted: a constant slice comes back bit for bit)."""
    flat = np.asarray(x, np.float32).reshape(x.shape[0], -1)
    nonfinite = ~np.all(np.isfinite(flat), axis=1)
    return nonfinite, np.all(flat == flat[:, :1], axis=1) & ~nonfinite


def unring(x, tables, min_w=DEFAULT_MIN_W, max_w=DEFAULT_MAX_W, details=False):
    """``(out float32 (S, ny, nx), skipped)``: the whole stage.  out = unring_rows along x of I1 + unring_rows along y of I2, one
    float32 addition.  With ``details``: also shift int8 and tv float32, each (2, S, ny, nx) (axis x first); both are whatever
    the rows gave, also on copied slices."""
    x = np.asarray(x, np.float32)
    t = tables
    check_params(t.ny, t.nx, t.K, min_w, max_w)
    nonfinite, constant = skipped_slices(x)
    i1, i2 = split(x, t)
    s = x.shape[0]
    ox, jx, tx = (a.reshape(s, t.ny, t.nx) for a in unring_rows(i1.reshape(-1, t.nx), t.hx, t.ab, min_w, max_w))
    oy, jy, ty = (a.reshape(s, t.nx, t.ny).transpose(0, 2, 1)
                  for a in unring_rows(i2.transpose(0, 2, 1).reshape(-1, t.ny), t.hy, t.ab, min_w, max_w))
    with np.errstate(invalid="ignore", over="ignore"):
        out = ox + oy
    copy = nonfinite | constant
    out[copy] = x[copy]
    if details:
        return out, int(nonfinite.sum()), np.stack([jx, jy]), np.stack([tx, ty])
    return out, int(nonfinite.sum())
