"""Multi-component T2 spectra, stated in numpy: what ``t2fit_nnls_pack_host`` writes and what ``t2fit_nnls_dev`` computes
(include/t2fit.h), plus the basis builders that the device path shares.  A decay is decomposed into a non-negative
distribution over a grid of T2 values by Tikhonov-regularised non-negative least squares (Whittall & MacKay 1989),
``min |A x - y|^2 + mu^2 |x|^2, x >= 0``, solved by Lawson-Hanson's active-set method on the normal equations (Bro & de Jong
1997).  Everything is float64 with one rounding per operation in the order written, nothing fused; the device equals it bit
for bit.  Used by the tests as the definition and by nobody on the hot path.  The chi^2 rule at the end (``solve_voxel_chi2``,
``solve_chi2``: what ``t2fit_nnls_chi2_dev`` computes) chooses ``mu`` per voxel by a short, deterministic loop of such solves.

The passive set P is an ordered list (order of insertion) and the Cholesky factor L of G_PP is taken in that order.  Row r
of L reads only the rows before it, so the factor does not depend on whether a row is kept or recomputed: after a removal
the rows before the first removed position stay and the rest are recomputed (``reuse_rows``); refactoring from scratch gives
the same bits (tests/test_nnls_host.py).  Vector expressions below act on independent elements; every element sees exactly
the operations, in exactly the order, of the row-oriented formulas in include/t2fit.h (a substitution that subtracts one
product at a time in ascending k -- descending k for the transposed solve -- is the same whether it runs by rows or by
columns)."""
from __future__ import annotations

import math
import struct

import numpy as np

from ._dict import log_grid  # noqa: F401  (the T2 grid of a spectrum is the grid of a dictionary)

MAX_BASIS, MAX_TE, MAX_FUNC = 64, 32, 8
MAGIC = 0x4C4E3254
HEADER_BYTES = 64
ST_MASKED, ST_OK, ST_MAXITER, ST_BREAKDOWN, ST_NONFINITE = -1, 0, 1, 2, 3
TOL_REL, PIV_REL = 1e-10, 1e-12


# ---- bases ------------------------------------------------------------------------------------------------------------

class Basis:
    """A table ``A`` float64 ``(n_te, n_basis)``, the regularisation ``mu`` (absolute, in the units of A) and the functionals
    ``W`` float64 ``(n_func, n_basis)`` with their ``names``; ``t2_grid`` (or None) is what the columns stand for.  ``G`` is
    ``A^T A + mu^2 I`` as the packed block holds it."""

    def __init__(self, A, mu=0.0, W=None, names=(), t2_grid=None):
        self.A = np.ascontiguousarray(A, dtype=np.float64)
        self.mu = float(mu)
        n_basis = self.A.shape[1] if self.A.ndim == 2 else 0
        self.W = np.zeros((0, n_basis)) if W is None else np.ascontiguousarray(W, dtype=np.float64).reshape(-1, n_basis)
        self.names = tuple(str(n) for n in names)
        self.t2_grid = None if t2_grid is None else np.asarray(t2_grid, np.float64).reshape(-1)
        check_basis(self.A, self.mu, self.W)
        if len(self.names) != self.W.shape[0] or len(set(self.names)) != len(self.names):
            raise ValueError(f"names must be {self.W.shape[0]} distinct functional names, got {self.names}")
        if self.t2_grid is not None and self.t2_grid.size != n_basis:
            raise ValueError(f"t2_grid has {self.t2_grid.size} values, the basis has {n_basis} columns")
        self.G = gram(self.A, self.mu)

    @property
    def n_te(self):
        return self.A.shape[0]

    @property
    def n_basis(self):
        return self.A.shape[1]

    @property
    def n_func(self):
        return self.W.shape[0]

    def with_mu(self, mu):
        return Basis(self.A, mu, self.W, self.names, self.t2_grid)


def check_basis(A, mu, W):
    """The refusals of ``t2fit_nnls_pack_host``."""
    if A.ndim != 2 or not (2 <= A.shape[0] <= MAX_TE) or not (2 <= A.shape[1] <= MAX_BASIS):
        raise ValueError(f"a basis is (n_te, n_basis) with n_te in 2 .. {MAX_TE} and n_basis in 2 .. {MAX_BASIS}, got shape {A.shape}")
    if W.ndim != 2 or W.shape[1] != A.shape[1] or W.shape[0] > MAX_FUNC:
        raise ValueError(f"the functionals are (n_func, {A.shape[1]}) with n_func in 0 .. {MAX_FUNC}, got shape {W.shape}")
    if not (math.isfinite(mu) and mu >= 0):
        raise ValueError(f"mu must be finite and not negative, got {mu}")
    if not np.all(np.isfinite(A)) or not np.all(np.isfinite(W)):
        raise ValueError("the basis or a functional has a non-finite entry")


def monoexp_basis(te_ms, t2_grid):
    """float64 ``(n_te, n_basis)``: ``exp(-TE_i / T2_j)``."""
    te = np.asarray(te_ms, np.float64).reshape(-1)
    t2 = np.asarray(t2_grid, np.float64).reshape(-1)
    if not np.all(t2 > 0):
        raise ValueError("the T2 grid must be positive")
    return np.exp(-te[:, None] / t2[None, :])


def window_functionals(t2_grid, windows):
    """``(W, names)``: one 0 / 1 row per window ``{name: (lo, hi)}``, 1 where ``lo <= T2_j <= hi``."""
    t2 = np.asarray(t2_grid, np.float64).reshape(-1)
    rows, names = [], []
    for name, (lo, hi) in windows.items():
        if not (float(lo) <= float(hi)):
            raise ValueError(f"window {name!r} needs LO <= HI, got {lo}, {hi}")
        rows.append(((t2 >= float(lo)) & (t2 <= float(hi))).astype(np.float64))
        names.append(str(name))
    return (np.stack(rows) if rows else np.zeros((0, t2.size))), tuple(names)


def ln_t2_functional(t2_grid):
    """float64 ``(n_basis,)``: ``ln T2_j``; ``exp(func / amp)`` is then the geometric-mean T2."""
    return np.log(np.asarray(t2_grid, np.float64).reshape(-1))


def gram(A, mu):
    """``G = A^T A + mu^2 I``: every element an ascending-i sum from 0.0, then ``mu * mu`` added to the diagonal."""
    G = np.zeros((A.shape[1], A.shape[1]))
    for i in range(A.shape[0]):
        G = G + A[i][:, None] * A[i][None, :]
    m2 = float(mu) * float(mu)
    for j in range(A.shape[1]):
        G[j, j] = G[j, j] + m2
    return G


# ---- packing ----------------------------------------------------------------------------------------------------------

def layout(n_te, n_basis, n_func):
    """``(off_a, off_g, off_w, bytes)`` of the packed block."""
    up16 = lambda v: (v + 15) // 16 * 16
    off_a = HEADER_BYTES
    off_g = off_a + up16(n_te * n_basis * 8)
    off_w = off_g + up16(n_basis * n_basis * 8)
    return off_a, off_g, off_w, off_w + up16(n_func * n_basis * 8)


def pack(basis):
    """The packed basis as ``uint8`` bytes, byte for byte what ``t2fit_nnls_pack_host`` writes (layout: include/t2fit.h)."""
    n_te, n_basis, n_func = basis.n_te, basis.n_basis, basis.n_func
    off_a, off_g, off_w, nbytes = layout(n_te, n_basis, n_func)
    out = np.zeros(nbytes, np.uint8)
    out[:HEADER_BYTES] = np.frombuffer(struct.pack("<IiiidQQQQQ", MAGIC, n_te, n_basis, n_func, basis.mu, off_a, off_g, off_w, nbytes, 0),
                                       np.uint8)
    out[off_a:off_a + basis.A.nbytes] = basis.A.view(np.uint8).reshape(-1)
    out[off_g:off_g + basis.G.nbytes] = basis.G.view(np.uint8).reshape(-1)
    out[off_w:off_w + basis.W.nbytes] = basis.W.view(np.uint8).reshape(-1)
    return out


# ---- the factor -------------------------------------------------------------------------------------------------------

def factor_row(L, G, P, r, piv_rel):
    """Row r of the factor of G_PP in list order, from the rows before it: ``L[r][c] = (G[P_r][P_c] - sum_{k<c} L[r][k] L[c][k])
    / L[c][c]``, ``d = G[P_r][P_r] - sum_{k<r} L[r][k]^2``, products subtracted one at a time in ascending k.  False (and L
    untouched) unless ``d > piv_rel G[P_r][P_r]``."""
    pr = P[r]
    t = G[pr, P[:r + 1]].copy()
    for k in range(r):
        lk = t[k] / L[k, k]
        t[k] = lk
        t[k + 1:r] = t[k + 1:r] - L[k + 1:r, k] * lk
        t[r] = t[r] - lk * lk
    if not t[r] > piv_rel * G[pr, pr]:
        return False
    L[r, :r] = t[:r]
    L[r, r] = math.sqrt(t[r])
    return True


def solve_factor(L, b):
    """``L z = b`` with k ascending, then ``L^T s = z`` with k descending."""
    p = b.size
    t = b.copy()
    for k in range(p):
        t[k] = t[k] / L[k, k]
        t[k + 1:p] = t[k + 1:p] - L[k + 1:p, k] * t[k]
    for k in range(p - 1, -1, -1):
        t[k] = t[k] / L[k, k]
        t[:k] = t[:k] - L[k, :k] * t[k]
    return t


# ---- one voxel --------------------------------------------------------------------------------------------------------

def solve_voxel(y, basis, tol_rel=TOL_REL, piv_rel=PIV_REL, max_iter=0, reuse_rows=True, stats=None):
    """One voxel: ``(x float64 (n_basis,), P list, nit, status)``.  ``y``: float32 samples.  ``stats`` (a dict) receives
    ``removals`` (partial steps taken), ``bans``, ``max_p``, ``final_p`` and ``banned`` (the ban list at the end)."""
    A, G = basis.A, basis.G
    nb = basis.n_basis
    y = np.asarray(y, np.float32).astype(np.float64)
    x = np.zeros(nb)
    removals = bans = max_p = 0
    if not np.all(np.isfinite(y)):
        return x, [], 0, ST_NONFINITE
    h = np.zeros(nb)
    for i in range(basis.n_te):
        h = h + A[i] * y[i]
    tol = tol_rel * np.max(np.abs(h))
    limit = int(max_iter) if max_iter else 3 * nb
    P = np.zeros(nb, np.int64)
    xs = np.zeros(nb)
    p, nit, status = 0, 0, ST_OK
    in_p, banned = np.zeros(nb, bool), np.zeros(nb, bool)
    L = np.zeros((nb, nb))
    while True:
        w = h.copy()
        for k in range(p):
            w = w - G[:, P[k]] * xs[k]
        cand = ~in_p & ~banned & (w > tol)
        if not cand.any():
            break
        j = int(np.argmax(np.where(cand, w, -np.inf)))  # (the first of equal maxima: the lowest index)
        if nit == limit:
            status = ST_MAXITER
            break
        nit += 1
        P[p], xs[p] = j, 0.0
        if not factor_row(L, G, P, p, piv_rel):
            banned[j] = True
            bans += 1
            continue
        p += 1
        in_p[j] = True
        banned[:] = False
        max_p = max(max_p, p)
        while True:
            s = solve_factor(L, h[P[:p]])
            if np.all(s > 0):
                xs[:p] = s
                break
            removals += 1
            alpha, q = np.inf, -1
            for r in range(p):
                if not s[r] > 0:
                    a = xs[r] / (xs[r] - s[r])
                    if a != a:  # 0 / 0: a new entry whose solution is exactly 0 does not move
                        a = 0.0
                    if a < alpha:
                        alpha, q = a, r
            xn = xs[:p] + alpha * (s - xs[:p])
            xn[q] = 0.0
            keep = xn > 0
            first = int(np.argmin(keep))
            in_p[P[:p][~keep]] = False
            kept = int(keep.sum())
            P[:kept], xs[:kept] = P[:p][keep], xn[keep]
            xs[kept:] = 0.0
            p = kept
            if p == 0:
                break
            ok = True
            for r in range(first if reuse_rows else 0, p):
                if not factor_row(L, G, P, r, piv_rel):
                    ok = False
                    break
            if not ok:
                status = ST_BREAKDOWN
                break
        if status == ST_BREAKDOWN:
            break
    x[P[:p]] = xs[:p]
    if stats is not None:
        stats.update(removals=removals, bans=bans, max_p=max_p, final_p=p, banned=[int(j) for j in np.flatnonzero(banned)])
    return x, [int(v) for v in P[:p]], nit, status


def outputs_voxel(y, basis, x, P):
    """``(func float32 (n_func,), amp float32, rmse float32)`` of a solved voxel."""
    A, W = basis.A, basis.W
    y = np.asarray(y, np.float32).astype(np.float64)
    func = np.zeros(basis.n_func)
    amp = 0.0
    for j in range(basis.n_basis):
        func = func + W[:, j] * x[j]
        amp = amp + x[j]
    r = y.copy()
    for k in P:
        r = r - A[:, k] * x[k]
    ss = 0.0
    for i in range(basis.n_te):
        ss = ss + r[i] * r[i]
    with np.errstate(over="ignore"):
        return func.astype(np.float32), np.float32(amp), np.float32(math.sqrt(ss / float(basis.n_te)))


# ---- a volume ---------------------------------------------------------------------------------------------------------

def solve(echoes, basis, mask=None, tol_rel=TOL_REL, piv_rel=PIV_REL, max_iter=0, stats=None):
    """The definition of ``t2fit_nnls_dev``: a dict of ``x`` float32 ``(n_basis, ...)``, ``func`` float32 ``(n_func, ...)``,
    ``amp``, ``rmse`` float32 and ``nit``, ``status`` int32 of the echoes' spatial shape.  Outside the mask everything is 0
    and the status -1; a voxel with a non-finite sample has everything 0 and the status NONFINITE.  ``stats`` (a list)
    receives one dict per fitted voxel."""
    y = np.ascontiguousarray(echoes, dtype=np.float32)
    if y.ndim < 1 or y.shape[0] != basis.n_te:
        raise ValueError(f"the echoes are TE-major with {y.shape[0] if y.ndim else 0} echoes, the basis has {basis.n_te}")
    spatial = y.shape[1:]
    y = y.reshape(basis.n_te, -1)
    n_vox = y.shape[1]
    m = np.ones(n_vox, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    if m.size != n_vox:
        raise ValueError("mask shape does not match the echoes")
    out = {"x": np.zeros((basis.n_basis, n_vox), np.float32), "func": np.zeros((basis.n_func, n_vox), np.float32),
           "amp": np.zeros(n_vox, np.float32), "rmse": np.zeros(n_vox, np.float32), "nit": np.zeros(n_vox, np.int32),
           "status": np.full(n_vox, ST_MASKED, np.int32)}
    for v in np.flatnonzero(m):
        st = {} if stats is not None else None
        x, P, nit, status = solve_voxel(y[:, v], basis, tol_rel, piv_rel, max_iter, stats=st)
        out["status"][v] = status
        if status == ST_NONFINITE:
            continue
        with np.errstate(over="ignore"):
            out["x"][:, v] = x.astype(np.float32)
        out["func"][:, v], out["amp"][v], out["rmse"][v] = outputs_voxel(y[:, v], basis, x, P)
        out["nit"][v] = nit
        if stats is not None:
            stats.append(st)
    for k in out:
        out[k] = out[k].reshape(out[k].shape[:-1] + spatial)
    return out


# ---- the chi^2 rule: the regularisation chosen per voxel ----------------------------------------------------------------

RULE_NONE, RULE_FOUND, RULE_EXACT, RULE_LOW, RULE_HIGH = -1, 0, 1, 2, 3
CHI2_DEFAULTS = {"factor": 1.02, "mu_first": 1e-3, "grow": 4.0, "n_grow": 6, "n_bisect": 5, "exact_rel": 1e-12, "mu_exact": 0.03}


def misfit(y, basis, x, P):
    """``sum_i r_i^2`` exactly as :func:`outputs_voxel` forms it for the RMSE: ``r = y - sum_{k in P, list order} A[:, k] x_k``,
    one product at a time, then the squares summed with i ascending from 0.0."""
    A = basis.A
    r = np.asarray(y, np.float32).astype(np.float64)
    for k in P:
        r = r - A[:, k] * x[k]
    ss = 0.0
    for i in range(basis.n_te):
        ss = ss + r[i] * r[i]
    return float(ss)


def check_chi2(factor, mu_first, grow, n_grow, n_bisect, exact_rel, mu_exact):
    """The refusals of ``t2fit_nnls_chi2_dev`` for the rule's numbers."""
    if not (math.isfinite(factor) and factor > 1):
        raise ValueError(f"factor must be finite and above 1, got {factor}")
    if not (math.isfinite(grow) and grow > 1):
        raise ValueError(f"grow must be finite and above 1, got {grow}")
    if not (math.isfinite(mu_first) and mu_first > 0):
        raise ValueError(f"mu_first must be finite and above 0, got {mu_first}")
    if not (math.isfinite(exact_rel) and exact_rel >= 0) or not (math.isfinite(mu_exact) and mu_exact >= 0):
        raise ValueError(f"exact_rel and mu_exact must be finite and not negative, got {exact_rel} and {mu_exact}")
    if not (0 <= int(n_grow) <= 64 and 0 <= int(n_bisect) <= 64):
        raise ValueError(f"n_grow and n_bisect must be 0 .. 64, got {n_grow} and {n_bisect}")


def solve_voxel_chi2(y, basis, tol_rel=TOL_REL, piv_rel=PIV_REL, max_iter=0, factor=1.02, mu_first=1e-3, grow=4.0, n_grow=6, n_bisect=5,
                     exact_rel=1e-12, mu_exact=0.03, stats=None):
    """One voxel under the chi^2 rule (Whittall & MacKay 1989; include/t2fit.h writes the steps out): ``(x, P, nit, status, mu,
    ratio, solves, rule)`` with ``x``, ``P`` of the final solve, ``nit`` summed and ``status`` the largest over the ``solves``
    runs of :func:`solve_voxel`, ``mu`` the chosen weight and ``ratio`` its misfit over the unregularised one (float64 both;
    0 for EXACT).  ``basis`` must have ``mu == 0``.  ``stats`` (a dict) receives ``ss0``, ``target``, the final bracket ``lo``,
    ``hi`` and ``trace``, the ``(mu, ss)`` of every run in order."""
    if basis.mu != 0:
        raise ValueError(f"the rule owns the weight: the basis must have mu 0, got {basis.mu}")
    check_chi2(factor, mu_first, grow, n_grow, n_bisect, exact_rel, mu_exact)
    y32 = np.asarray(y, np.float32)
    y = y32.astype(np.float64)
    if not np.all(np.isfinite(y)):
        return np.zeros(basis.n_basis), [], 0, ST_NONFINITE, 0.0, 0.0, 0, RULE_NONE
    runs = []

    def S(mu):
        x, P, nit, status = solve_voxel(y32, basis.with_mu(mu), tol_rel, piv_rel, max_iter)
        runs.append((mu, misfit(y32, basis, x, P), x, P, nit, status))
        return runs[-1][1]

    ss0 = S(0.0)
    yy = 0.0
    for i in range(basis.n_te):
        yy = yy + y[i] * y[i]
    target, lo, hi = float("nan"), 0.0, 0.0
    if not ss0 > exact_rel * yy:
        rule, mu = RULE_EXACT, float(mu_exact)
        S(mu)
    else:
        target = factor * ss0
        mu, hit, g = float(mu_first), False, 0
        for g in range(int(n_grow) + 1):
            if S(mu) >= target:
                hit = True
                break
            lo = mu
            if g < n_grow:
                mu = mu * grow
        if not hit:
            rule = RULE_HIGH
        elif g == 0:
            rule = RULE_LOW
        else:
            rule, hi = RULE_FOUND, mu
            for _ in range(int(n_bisect)):
                mid = math.sqrt(lo * hi)
                if S(mid) < target:
                    lo = mid
                else:
                    hi = mid
            mu = math.sqrt(lo * hi)
            S(mu)
    _, ss, x, P = runs[-1][:4]
    if stats is not None:
        stats.update(ss0=ss0, target=target, lo=lo, hi=hi, trace=[(r[0], r[1]) for r in runs])
    return (x, P, sum(r[4] for r in runs), max(r[5] for r in runs), mu, 0.0 if rule == RULE_EXACT else ss / ss0, len(runs), rule)


def solve_chi2(echoes, basis, mask=None, tol_rel=TOL_REL, piv_rel=PIV_REL, max_iter=0, stats=None, **chi2):
    """The definition of ``t2fit_nnls_chi2_dev``: the dict of :func:`solve` (from each voxel's final solve; ``nit`` summed and
    ``status`` the largest over its solves) plus ``mu``, ``ratio`` float32 and ``solves``, ``rule`` int32.  Outside the mask
    and for a non-finite sample everything is 0, the status MASKED / NONFINITE and the rule -1.  ``chi2``: the rule's numbers
    (``CHI2_DEFAULTS``).  ``stats`` (a list) receives one dict per fitted voxel."""
    y = np.ascontiguousarray(echoes, dtype=np.float32)
    if y.ndim < 1 or y.shape[0] != basis.n_te:
        raise ValueError(f"the echoes are TE-major with {y.shape[0] if y.ndim else 0} echoes, the basis has {basis.n_te}")
    unknown = set(chi2) - set(CHI2_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown numbers of the rule: {sorted(unknown)}")
    spatial = y.shape[1:]
    y = y.reshape(basis.n_te, -1)
    n_vox = y.shape[1]
    m = np.ones(n_vox, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    if m.size != n_vox:
        raise ValueError("mask shape does not match the echoes")
    out = {"x": np.zeros((basis.n_basis, n_vox), np.float32), "func": np.zeros((basis.n_func, n_vox), np.float32),
           "amp": np.zeros(n_vox, np.float32), "rmse": np.zeros(n_vox, np.float32), "nit": np.zeros(n_vox, np.int32),
           "status": np.full(n_vox, ST_MASKED, np.int32), "mu": np.zeros(n_vox, np.float32), "ratio": np.zeros(n_vox, np.float32),
           "solves": np.zeros(n_vox, np.int32), "rule": np.full(n_vox, RULE_NONE, np.int32)}
    for v in np.flatnonzero(m):
        st = {} if stats is not None else None
        x, P, nit, status, mu, ratio, solves, rule = solve_voxel_chi2(y[:, v], basis, tol_rel, piv_rel, max_iter, stats=st, **chi2)
        out["status"][v] = status
        if status == ST_NONFINITE:
            continue
        with np.errstate(over="ignore"):
            out["x"][:, v] = x.astype(np.float32)
            out["mu"][v], out["ratio"][v] = np.float32(mu), np.float32(ratio)
        out["func"][:, v], out["amp"][v], out["rmse"][v] = outputs_voxel(y[:, v], basis, x, P)
        out["nit"][v], out["solves"][v], out["rule"][v] = nit, solves, rule
        if stats is not None:
            stats.append(st)
    for k in out:
        out[k] = out[k].reshape(out[k].shape[:-1] + spatial)
    return out


def derived(func, amp, names):
    """The maps the binding forms from the functionals, float64 then rounded to float32: ``gmt2 = exp(func_lnT2 / amp)`` for a
    functional named ``lnT2`` and ``<name>fraction = func_name / amp`` for every other; 0 where ``amp`` is not above 0."""
    amp64 = np.asarray(amp, np.float64)
    ok = amp64 > 0
    safe = np.where(ok, amp64, 1.0)
    out = {}
    for m, name in enumerate(names):
        ratio = np.asarray(func[m], np.float64) / safe
        if name == "lnT2":
            out["gmt2"] = np.where(ok, np.exp(ratio), 0.0).astype(np.float32)
        else:
            out[name + "fraction"] = np.where(ok, ratio, 0.0).astype(np.float32)
    return out
