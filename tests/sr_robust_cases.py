"""Cases shared by tests/test_sr_robust_host.py and tests/test_sr_robust_gpu.py: the outlier weighting of the
super-resolution loop written from the definition in include/t2fit.h with Python floats, sample by sample and lane by lane
(nothing of fetal_t2mapping_amd._sr), residuals that exercise every branch of it, and the phantom with corrupted slices."""
import math

import numpy as np

import sr_cases as K
import sr_slice_cases as KS

LANES, WAVE = 256, 64
DEFAULTS = {"slice_threshold": 1.5, "huber": 2.5, "min_count": 16, "sigma_floor": 0.0}


# ---- the definition, in Python floats ------------------------------------------------------------------------------------
def _tree(lanes):
    """256 lane values -> the xor butterfly 32 .. 1 inside each wave of 64, then ((w0 + w1) + w2) + w3."""
    v = list(lanes)
    for s in (32, 16, 8, 4, 2, 1):
        v = [v[i] + v[i ^ s] for i in range(LANES)]
    return ((v[0] + v[WAVE]) + v[2 * WAVE]) + v[3 * WAVE]


def _counted(r, n, m):
    return n > 0.0 and (m is None or m != 0) and math.isfinite(r)


def ref_step(r, N, masks, params):
    """``(weighted r, slice weights, sigma2, sums)`` as ``_sr.robust_step`` returns them, from the definition alone."""
    p = {**DEFAULTS, **(params or {})}
    n_vol = r[0].shape[0]
    lz = [v.shape[1] for v in r]
    n_slices = sum(lz)
    sums = np.zeros((n_vol, n_slices, 2), np.float64)
    for e in range(n_vol):
        k = 0
        for s, rs in enumerate(r):
            plane = rs.shape[2] * rs.shape[3]
            flat_r = rs[e].reshape(lz[s], plane)
            flat_n = np.asarray(N[s], np.float64).reshape(lz[s], plane)
            flat_m = None if masks[s] is None else np.asarray(masks[s]).reshape(lz[s], plane)
            for z in range(lz[s]):
                c, q2 = [0.0] * LANES, [0.0] * LANES
                for i in range(plane):
                    v = float(flat_r[z, i])
                    if _counted(v, float(flat_n[z, i]), None if flat_m is None else int(flat_m[z, i])):
                        q2[i % LANES] = q2[i % LANES] + v * v
                        c[i % LANES] = c[i % LANES] + 1.0
                sums[e, k] = (_tree(c), _tree(q2))
                k += 1
    tt, floor2 = p["slice_threshold"] * p["slice_threshold"], p["sigma_floor"] * p["sigma_floor"]
    weights, sigma2 = np.ones((n_vol, n_slices), np.float64), np.zeros(n_vol, np.float64)
    for e in range(n_vol):
        m = [float(sums[e, k, 1]) / float(sums[e, k, 0]) if sums[e, k, 0] >= p["min_count"] else None for k in range(n_slices)]
        v = sorted(x for x in m if x is not None)
        n = len(v)
        if n == 0:
            continue
        s2 = max(0.5 * (v[(n - 1) // 2] + v[n // 2]), floor2)
        if not s2 > 0.0:
            continue
        sigma2[e] = s2
        for k in range(n_slices):
            if m[k] is not None and not m[k] <= tt * s2:
                weights[e, k] = (tt * s2) / m[k]
    out = [v.copy() for v in r]
    for e in range(n_vol):
        if not sigma2[e] > 0.0:
            continue
        delta = p["huber"] * math.sqrt(float(sigma2[e]))
        k0 = 0
        for s, rs in enumerate(r):
            nz, ny, nx = rs.shape[1:]
            for z in range(nz):
                q = float(weights[e, k0 + z])
                for y in range(ny):
                    for x in range(nx):
                        v = float(rs[e, z, y, x])
                        if _counted(v, float(N[s][z, y, x]), None if masks[s] is None else int(masks[s][z, y, x])):
                            w = 1.0 if abs(v) <= delta else delta / abs(v)
                            out[s][e, z, y, x] = np.float32((q * w) * v)
                        else:
                            out[s][e, z, y, x] = np.float32(0.0)
            k0 += nz
    edges = np.cumsum([0] + lz)
    return out, [weights[:, edges[s]:edges[s + 1]].copy() for s in range(len(r))], sigma2, sums


# ---- residuals -------------------------------------------------------------------------------------------------------------
def residuals(shapes, n_vol, seed, masked=(), loud_slices=(), zero_n=0.1):
    """``(r, N, masks)``: per stack float32 normal residuals of scale 10 ``(n_vol, lz, ly, lx)`` with a few samples 30 times
    larger (the Huber branch) and the slices ``loud_slices`` (stack, slice) 4 times larger (the slice branch); ``N`` positive
    with a fraction ``zero_n`` of zeros; a mask with holes for the stacks in ``masked``, None for the others."""
    rng = np.random.default_rng(seed)
    r, N, masks = [], [], []
    for s, shape in enumerate(shapes):
        v = rng.normal(0.0, 10.0, (n_vol,) + tuple(shape))
        v = np.where(rng.random(v.shape) < 0.04, 30.0 * v, v)
        for (ss, z) in loud_slices:
            if ss == s:
                v[:, z] *= 4.0
        r.append(v.astype(np.float32))
        n = rng.uniform(0.5, 3.0, shape)
        n[rng.random(shape) < zero_n] = 0.0
        N.append(n)
        masks.append((rng.random(shape) > 0.2).astype(np.uint8) if s in masked else None)
    return r, N, masks


def _six():
    # slices of 1, 35 (less than a wave), 256 (one sample per lane), 257 (one lane takes two) and 21 x 19 samples; lz from 1;
    # 5 echoes: not a multiple of the echo chunk; min_count 1, so that even a one-sample slice is eligible
    shapes = [(3, 1, 1), (2, 5, 7), (1, 16, 16), (2, 1, 257), (5, 19, 21), (4, 8, 8)]
    r, N, masks = residuals(shapes, 5, 71, masked=(1, 4), loud_slices=((4, 2), (5, 0), (1, 1)), zero_n=0.05)
    N[0][:] = 1.0
    return r, N, masks, {"min_count": 1}


def _parity(lz2, seed):
    def make():
        r, N, masks = residuals([(5, 19, 21), (lz2, 16, 16)], 1, seed, masked=(0,), loud_slices=((0, 1),))
        return r, N, masks, None
    return make


def _edges():
    """Echo 0: a slice with no counted sample, one with ``min_count - 1`` and one with ``min_count`` of them, two identical
    slices (a tie in the median), NaN / +inf / -inf samples.  Echo 1: every residual zero (one of them -0.0) except a NaN:
    robustness is off and the echo stays bit for bit as it was."""
    shapes = [(7, 16, 16), (3, 19, 21)]
    r, N, masks = residuals(shapes, 2, 73, masked=(0, 1), loud_slices=((1, 2),), zero_n=0.0)
    m = masks[0]
    m[0] = 0                      # c = 0
    m[1] = 0
    m[1].reshape(-1)[:15] = 1     # c = 15 = min_count - 1
    m[2] = 0
    m[2].reshape(-1)[100:116] = 1  # c = 16 = min_count
    m[3] = 1
    m[4] = 1
    m[5] = 1
    m[6] = 1
    r[0][0, 4] = r[0][0, 3]       # a tie
    r[0][0, 5, 3, 3] = np.nan
    r[0][0, 5, 3, 4] = np.inf
    r[0][0, 6, 0, 0] = -np.inf
    r[1][0, 0, 2, 2] = np.nan
    for v in r:
        v[1] = 0.0
    r[0][1, 3, 1, 1] = -0.0
    r[0][1, 3, 1, 2] = np.nan
    return r, N, masks, None


def _floor():
    r, N, masks = residuals([(4, 16, 16), (3, 19, 21)], 2, 74, masked=(1,), loud_slices=((0, 1),))
    return r, N, masks, {"sigma_floor": 100.0}  # the medians are a few thousand: the floor's 10000 takes over


def _none_eligible():
    r, N, masks = residuals([(4, 16, 16), (3, 5, 7)], 1, 75)
    return r, N, masks, {"min_count": 1000}


def _tuned():
    r, N, masks = residuals([(4, 16, 16), (5, 19, 21), (1, 35, 1)], 3, 76, masked=(0, 2), loud_slices=((0, 0), (1, 4)))
    return r, N, masks, {"slice_threshold": 1.1, "huber": 1.3, "min_count": 20, "sigma_floor": 2.0}


CASES = {"six_stacks": _six, "odd": _parity(4, 72), "even": _parity(3, 77), "edges": _edges, "floor": _floor,
         "none_eligible": _none_eligible, "tuned": _tuned}
_BUILT = {}


def case(name):
    """``(r, N, masks, params, reference)`` of a case, built and referenced once; treat as read-only."""
    if name not in _BUILT:
        r, N, masks, params = CASES[name]()
        _BUILT[name] = (r, N, masks, params, ref_step(r, N, masks, params))
    return _BUILT[name]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the phantom with corrupted slices -------------------------------------------------------------------------------------
CORRUPTED = {"ax": (3, 8), "cor": (5,), "sag": (6,)}
_PHANTOM = {}


def corrupt(stacks):
    """ax slices 3 and 8 and cor slice 5 dimmed to 0.3 x, sag slice 6 with + 400 on ``[10:30, 10:30]``; all echoes."""
    out = {o: np.array(v, np.float32) for o, v in stacks.items()}
    out["ax"][..., 3, :, :] *= np.float32(0.3)
    out["ax"][..., 8, :, :] *= np.float32(0.3)
    out["cor"][..., 5, :, :] *= np.float32(0.3)
    out["sag"][..., 6, 10:30, 10:30] += np.float32(400.0)
    return out


def corrupted_phantom():
    """``(clean stacks, corrupted stacks, geoms, truth, grid)`` of ``sr_cases.phantom()``."""
    if "p" not in _PHANTOM:
        stacks, geoms, truth, grid = K.phantom()[:4]
        _PHANTOM["p"] = (stacks, corrupt(stacks), geoms, truth, grid)
    return _PHANTOM["p"]


def check_phantom_conditions(rmse_plain_clean, rmse_plain_bad, rmse_robust_clean, rmse_robust_bad, slice_weights, order):
    """The four conditions on the corrupted phantom; ``slice_weights``: per stack of ``order`` ``(n_vol, lz)`` arrays."""
    print(f"interior RMSE: plain clean {rmse_plain_clean:.2f}, plain corrupted {rmse_plain_bad:.2f}, "
          f"robust clean {rmse_robust_clean:.2f}, robust corrupted {rmse_robust_bad:.2f}")
    bad = np.concatenate([np.asarray(slice_weights[s])[:, list(CORRUPTED[o])].ravel() for s, o in enumerate(order)])
    good = np.concatenate([np.delete(np.asarray(slice_weights[s]), list(CORRUPTED[o]), axis=1).ravel() for s, o in enumerate(order)])
    print(f"slice weights: corrupted max {bad.max():.3f}, clean min {good.min():.3f}")
    assert abs(rmse_robust_bad - rmse_plain_clean) < abs(rmse_robust_bad - rmse_plain_bad)
    assert rmse_robust_clean <= 1.05 * rmse_plain_clean
    assert bad.max() < 0.5
    assert good.min() >= 0.75


def moved_corrupted(n_te=1):
    """``sr_slice_cases.moved_phantom`` with one corrupted slice (cor slice 5 dimmed to 0.3 x): ``(stacks, geoms, poses)``."""
    key = ("m", n_te)
    if key not in _PHANTOM:
        stacks, geoms, _, _, poses = KS.moved_phantom(n_te=n_te)
        stacks = {o: np.array(v, np.float32) for o, v in stacks.items()}
        stacks["cor"][..., 5, :, :] *= np.float32(0.3)
        _PHANTOM[key] = (stacks, geoms, poses)
    return _PHANTOM[key]
