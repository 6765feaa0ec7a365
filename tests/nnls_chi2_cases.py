"""Shared cases of the chi^2 rule of the T2-spectrum fit (tests/test_nnls_chi2_host.py, tests/test_nnls_chi2_gpu.py): the
parameter sets that reach each rule code, decays with an exact fit, and the statement's outputs of a set of distinct voxels,
computed once per (case, parameter set) and tiled to any voxel count.  Bases, noisy decays and edge voxels are those of
tests/nnls_cases.py."""
import functools

import numpy as np

import nnls_cases as K
from fetal_t2mapping_amd import _nnls as N

# name -> the rule's numbers that differ from the defaults, and the rule code the 8 x 40 decays then reach (None: several)
PARAMS = {
    "default": ({}, N.RULE_FOUND),
    "low": ({"mu_first": 0.5}, N.RULE_LOW),
    "high": ({"mu_first": 1e-6, "n_grow": 1}, N.RULE_HIGH),
    "no_bisect": ({"n_bisect": 0}, N.RULE_FOUND),
    "no_grow": ({"n_grow": 0}, None),
    "other": ({"factor": 1.1, "grow": 2.5, "n_grow": 12, "n_bisect": 3, "mu_first": 3e-4, "exact_rel": 1e-9, "mu_exact": 0.1}, N.RULE_FOUND),
}
OUTPUTS = ("x", "func", "amp", "rmse", "nit", "status", "mu", "ratio", "solves", "rule")


def exact_decays(n_te, n_basis, n_vox, seed):
    """float32 ``(n_te, n_vox)``: two columns of ``K.basis(n_te, n_basis, 0)`` with positive weights, rounded to float32: the
    unregularised misfit is what the rounding leaves, about 1e-15 of ``sum y^2``."""
    rng = np.random.default_rng(seed)
    A = K.basis(n_te, n_basis, 0.0).A
    ja = rng.integers(0, n_basis // 2, n_vox)
    jb = rng.integers(n_basis // 2, n_basis, n_vox)
    return (rng.uniform(300.0, 3000.0, n_vox) * A[:, ja] + rng.uniform(100.0, 900.0, n_vox) * A[:, jb]).astype(np.float32)


def voxels(n_te, kind, n_unique, seed):
    """float32 ``(n_te, n_unique)`` distinct voxels: ``noisy`` (sigma 10), ``noisier`` (sigma 50), ``exact`` (for 40 basis
    functions), ``edge`` (K.edge_voxels, then noisy ones)."""
    if kind == "noisy":
        return K.decays(n_te, n_unique, seed)
    if kind == "noisier":
        return K.decays(n_te, n_unique, seed, sigma=50.0)
    if kind == "exact":
        return exact_decays(n_te, 40, n_unique, seed)
    edge = K.edge_voxels(n_te)[0]
    return np.concatenate([edge, K.decays(n_te, n_unique - edge.shape[1], seed)], axis=1)


@functools.lru_cache(maxsize=None)
def reference(n_te, n_basis, kind, n_unique, seed, params="default", max_iter=0, n_func=4):
    """``(unique_y, ref, stats)``: the statement on ``n_unique`` distinct voxels, once; the arrays are read-only."""
    y = voxels(n_te, kind, n_unique, seed)
    stats = []
    ref = N.solve_chi2(y, K.basis(n_te, n_basis, 0.0, n_func), None, max_iter=max_iter, stats=stats, **PARAMS[params][0])
    y.setflags(write=False)
    for v in ref.values():
        v.setflags(write=False)
    return y, ref, stats


def tiled(n_vox, mask=None, **case):
    """``(y, want)`` for ``n_vox`` voxels that repeat the distinct voxels of ``reference(**case)``: the statement is a
    function of the voxel alone.  Outside ``mask`` everything is 0, the status MASKED and the rule -1."""
    unique_y, ref, _ = reference(**case)
    idx = np.arange(n_vox) % unique_y.shape[1]
    want = {k: np.ascontiguousarray(v[..., idx]) for k, v in ref.items()}
    if mask is not None:
        off = np.asarray(mask).reshape(-1) == 0
        for k, v in want.items():
            v[..., off] = {"status": N.ST_MASKED, "rule": N.RULE_NONE}.get(k, 0)
    return np.ascontiguousarray(unique_y[:, idx]), want
