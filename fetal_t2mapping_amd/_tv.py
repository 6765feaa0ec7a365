"""Chambolle's projection algorithm for the ROF total-variation model, restated in numpy: the executable statement of
the definition in include/t2fit.h (t2fit_tv_denoise_dev), which is scikit-image 0.22's ``denoise_tv_chambolle`` on a
float image (what the reference's ``run_denoising`` calls slice by slice).  Every elementwise operation is one rounding
in the working precision, in the order written; the two energy sums are accumulated in float64 (skimage sums them in
the image's precision, so on a float32 image its stop can fall one iteration away when ``|E_prev - E|`` lies within
float32 rounding of the threshold).  The second half states the vector-valued (joint) form across the channels of a stack
(t2fit_tv_joint_denoise_dev) from the same steps.  Host code for tests and baselines: the product path is the HIP kernel."""
from __future__ import annotations

import numpy as np

DEFAULT_WEIGHT, DEFAULT_EPS, DEFAULT_MAX_ITER = 0.1, 2e-4, 200


def _lo(n, a):
    """The voxels whose neighbour x - e_a is inside."""
    return tuple(slice(1, None) if b == a else slice(None) for b in range(n))


def _hi(n, a):
    """The voxels whose neighbour x + e_a is inside."""
    return tuple(slice(0, -1) if b == a else slice(None) for b in range(n))


def step_sizes(n, weight, T):
    """``(tau, tau / weight)``: each formed in float64 and rounded to the working precision once."""
    return T(1.0 / (2.0 * n)), T((1.0 / (2.0 * n)) / float(weight))


def divergence(p):
    """``d = ((-(p_0 + .. + p_{n-1})) + p_0[x - e_0]) + p_1[x - e_1] ..``, a term dropped where ``x - e_a`` is outside."""
    n = len(p)
    s = p[0] + p[1]
    if n == 3:
        s = s + p[2]
    d = -s
    for a in range(n):
        d[_lo(n, a)] = d[_lo(n, a)] + p[a][_hi(n, a)]
    return d


def gradient(out):
    """The forward differences of ``out`` along every axis, 0 where ``x + e_a`` is outside."""
    n = out.ndim
    g = []
    for a in range(n):
        ga = np.zeros(out.shape, out.dtype)
        ga[_hi(n, a)] = out[_lo(n, a)] - out[_hi(n, a)]
        g.append(ga)
    return g


def energy(d, nrm, weight):
    """``(sum d^2 + weight sum |g|) / N``: squares and norms in the working precision, the two sums in float64."""
    return (float(np.sum((d * d).astype(np.float64))) + float(weight) * float(np.sum(nrm.astype(np.float64)))) / d.size


def update(p, g, nrm, tau, tw):
    """``p_a = (p_a - tau g_a) / (1 + (tau / weight) |g|)``."""
    den = tau.dtype.type(1.0) + tw * nrm
    return [(p[a] - tau * g[a]) / den for a in range(len(p))]


def tv_problem(f, weight=DEFAULT_WEIGHT, eps=DEFAULT_EPS, max_iter=DEFAULT_MAX_ITER, dtype=np.float32, history=None):
    """One problem: ``f`` is a 2-D slice or a 3-D volume, iterated in ``dtype``.  Returns ``(out, n_iter, E)`` with ``out``
    in ``dtype``, ``n_iter`` the number of updates of p the result reflects and ``E`` the energy of the last iteration.
    ``history``: a list that receives the energy of every iteration.
    The steps are the module's functions above, looked up at every call (tests/denoise_cases.py replaces them one at a
    time with wrong variants to show that its reference notices)."""
    T = np.dtype(dtype).type
    f = np.asarray(f).astype(T)
    n = f.ndim
    if n not in (2, 3):
        raise ValueError("a problem is a 2-D slice or a 3-D volume")
    tau, tw = step_sizes(n, weight, T)
    p = [np.zeros(f.shape, T) for _ in range(n)]
    e_init = e_prev = e = 0.0
    out = f
    n_iter = 0
    with np.errstate(all="ignore"):
        for i in range(int(max_iter)):
            d = np.zeros(f.shape, T) if i == 0 else divergence(p)
            out = f + d
            g = gradient(out)
            sq = g[0] * g[0] + g[1] * g[1]
            if n == 3:
                sq = sq + g[2] * g[2]
            nrm = np.sqrt(sq)
            e = energy(d, nrm, weight)
            if history is not None:
                history.append(e)
            p = update(p, g, nrm, tau, tw)
            n_iter = i
            if i == 0:
                e_init = e_prev = e
            elif abs(e_prev - e) < eps * e_init:
                break
            else:
                e_prev = e
    return out, n_iter, e


def denoise_tv(stack, weight=DEFAULT_WEIGHT, eps=DEFAULT_EPS, max_iter=DEFAULT_MAX_ITER, dims=2, precision="f32"):
    """The whole call on the host: ``stack`` is ``(Z, Y, X)`` or ``(n, Z, Y, X)`` float32; ``dims=2`` takes every
    ``(Y, X)`` slice as a problem, ``dims=3`` every volume.  Returns ``(out float32 like stack, n_iter int32 per problem,
    energy float64 per problem)``, problems in memory order."""
    a = np.ascontiguousarray(stack, dtype=np.float32)
    if a.ndim not in (3, 4):
        raise ValueError("stack must be (Z, Y, X) or (n, Z, Y, X)")
    if dims not in (2, 3):
        raise ValueError("dims must be 2 or 3")
    dtype = {"f32": np.float32, "f64": np.float64}[precision]
    v = a.reshape((-1,) + a.shape[-3:])
    probs = v.reshape((-1,) + v.shape[-2:]) if dims == 2 else v
    out = np.empty(probs.shape, np.float32)
    n_iter = np.zeros(len(probs), np.int32)
    energy = np.zeros(len(probs), np.float64)
    for k, f in enumerate(probs):
        o, n_iter[k], energy[k] = tv_problem(f, weight, eps, max_iter, dtype)
        out[k] = o.astype(np.float32)
    return out.reshape(a.shape), n_iter, energy


# ---- vector-valued (joint) TV across the channels of a stack: include/t2fit.h, t2fit_tv_joint_denoise_dev ---------------------
def joint_norm(g):
    """``sqrt(S)``, ``S = sq_0; S = S + sq_c`` for c ascending, ``sq_c`` the scalar definition's sum of squares of channel
    c's differences ``g[c]``: one norm per voxel, shared by all channels."""
    s = None
    for gc in g:
        sq = gc[0] * gc[0] + gc[1] * gc[1]
        if len(gc) == 3:
            sq = sq + gc[2] * gc[2]
        s = sq if s is None else s + sq
    return np.sqrt(s)


def joint_energy(d, nrm, weight):
    """``(sum_c sum_x d_c^2 + weight sum_x nrm) / N``, ``N = C`` times the voxels of a channel: squares and norms in the
    working precision, the sums in float64, channels ascending."""
    sd = float(np.sum((d[0] * d[0]).astype(np.float64)))
    for dc in d[1:]:
        sd = sd + float(np.sum((dc * dc).astype(np.float64)))
    return (sd + float(weight) * float(np.sum(nrm.astype(np.float64)))) / (len(d) * d[0].size)


def tv_joint_problem(f, weight=DEFAULT_WEIGHT, eps=DEFAULT_EPS, max_iter=DEFAULT_MAX_ITER, dtype=np.float32, history=None):
    """One joint problem: ``f`` is ``(C, Y, X)`` or ``(C, Z, Y, X)``; the C channels keep a dual field each and share one
    gradient norm per voxel, ``sqrt(sum_c |grad u_c|^2)``.  Returns ``(out like f in dtype, n_iter, E)`` as
    :func:`tv_problem` does; with ``C = 1`` every byte, ``n_iter`` and ``E`` are :func:`tv_problem`'s.  The weight is not
    rescaled by C: the joint norm of pure noise is about ``sqrt(C)`` times a channel's.  The steps are the module's
    functions, looked up at every call."""
    T = np.dtype(dtype).type
    f = np.asarray(f).astype(T)
    n = f.ndim - 1
    if n not in (2, 3):
        raise ValueError("a joint problem is (C, Y, X) or (C, Z, Y, X)")
    chans = range(f.shape[0])
    tau, tw = step_sizes(n, weight, T)
    p = [[np.zeros(f.shape[1:], T) for _ in range(n)] for _ in chans]
    e_init = e_prev = e = 0.0
    out = f
    n_iter = 0
    with np.errstate(all="ignore"):
        for i in range(int(max_iter)):
            d = [np.zeros(f.shape[1:], T) if i == 0 else divergence(p[c]) for c in chans]
            out = np.stack([f[c] + d[c] for c in chans])
            g = [gradient(out[c]) for c in chans]
            nrm = joint_norm(g)
            e = joint_energy(d, nrm, weight)
            if history is not None:
                history.append(e)
            p = [update(p[c], g[c], nrm, tau, tw) for c in chans]
            n_iter = i
            if i == 0:
                e_init = e_prev = e
            elif abs(e_prev - e) < eps * e_init:
                break
            else:
                e_prev = e
    return out, n_iter, e


def denoise_tv_joint(stack, weight=DEFAULT_WEIGHT, eps=DEFAULT_EPS, max_iter=DEFAULT_MAX_ITER, dims=2, precision="f32"):
    """The joint call on the host: ``stack`` is ``(C, Z, Y, X)`` float32; ``dims=2`` takes slice z of all channels as a
    problem (Z problems), ``dims=3`` the whole stack as one.  Returns ``(out float32 like stack, n_iter int32 per problem,
    energy float64 per problem)``."""
    a = np.ascontiguousarray(stack, dtype=np.float32)
    if a.ndim != 4:
        raise ValueError("stack must be (C, Z, Y, X)")
    if dims not in (2, 3):
        raise ValueError("dims must be 2 or 3")
    dtype = {"f32": np.float32, "f64": np.float64}[precision]
    out = np.empty(a.shape, np.float32)
    if dims == 3:
        o, n, e = tv_joint_problem(a, weight, eps, max_iter, dtype)
        out[...] = o.astype(np.float32)
        return out, np.array([n], np.int32), np.array([e], np.float64)
    n_iter = np.zeros(a.shape[1], np.int32)
    energy = np.zeros(a.shape[1], np.float64)
    for z in range(a.shape[1]):
        o, n_iter[z], energy[z] = tv_joint_problem(a[:, z], weight, eps, max_iter, dtype)
        out[:, z] = o.astype(np.float32)
    return out, n_iter, energy
