"""Named cases of the TV-Chambolle denoiser and two INDEPENDENT references, written from the mathematical
definition and not from the kernel or the numpy statement (fetal_t2mapping_amd/_tv.py): Chambolle's iteration point by
point in extended precision (np.pad + np.diff, no slice tables), and the exact minimiser of the 1-D problem from the
dual by bounded least squares (no Chambolle at all).  Shared by tests/test_denoise_host.py and tests/test_denoise_gpu.py."""
import contextlib
import functools

import numpy as np

from fetal_t2mapping_amd import _tv

LD = np.longdouble
DTYPE = {"f32": np.float32, "f64": np.float64}
EPS = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
WEIGHT = 25.0           # the weight of every case of the table: about one sigma of the noise
KS = (1, 2, 7, 40)      # numbers of updates of p the references are held at

# (n_vol, nz, ny, nx), the dims the entry is for, the input ("picture": the blocks and disc of `picture`; "field": steps
# plus noise, where the picture degenerates).  The pass kernel tiles a problem 32 x 64 (2-D) or 4 x 8 x 64 (3-D) in quads
# of four x, fetches the column x0 + 64 point by point, and takes 128-bit accesses when nx % 4 == 0.
SHAPES = [((2, 1, 64, 64), (2, 3), "picture"),    # one full x tile, vector path
          ((2, 5, 37, 53), (2, 3), "picture"),    # odd sizes, scalar path, a ragged last quad
          ((1, 3, 256, 256), (2, 3), "picture"),  # 32 tiles per 2-D problem; 4 x tiles, vector path
          ((2, 16, 17, 1), (2, 3), "picture"),    # nx = 1
          ((2, 2, 3, 2), (2, 3), "field"),        # nx = 2: half a quad
          ((2, 2, 3, 3), (2, 3), "field"),        # nx = 3
          ((2, 2, 3, 4), (2, 3), "field"),        # nx = 4: one quad, vector path
          ((2, 2, 3, 5), (2, 3), "field"),        # nx = 5: a second quad of one voxel
          ((2, 2, 3, 65), (2, 3), "field"),       # one voxel in the second x tile: the halo column is its only content
          ((2, 2, 3, 67), (2, 3), "field"),       # a ragged quad in the second x tile, scalar path across the tile edge
          ((2, 3, 2, 68), (2, 3), "field"),       # vector path, one quad in the second x tile
          ((2, 2, 3, 130), (2, 3), "field"),      # three x tiles, two halo columns of real data, scalar path
          ((2, 2, 2, 132), (2, 3), "field"),      # the same on the vector path
          ((2, 3, 1, 9), (2, 3), "field"),        # ny = 1: no y difference anywhere
          ((2, 1, 32, 5), (2,), "field"),         # 2-D: ny exactly one tile
          ((2, 1, 33, 5), (2,), "field"),         # 2-D: one row in the second y tile; the halo row is real data
          ((2, 1, 1, 9), (3,), "field"),          # 3-D: nz = 1 and ny = 1
          ((2, 4, 8, 6), (3,), "field"),          # 3-D: nz and ny exactly one tile
          ((2, 5, 9, 7), (3,), "field"),          # 3-D: one plane and one row past a tile
          ((2, 4, 9, 6), (3,), "field"),          # 3-D: ny one past, nz exact
          ((2, 5, 8, 6), (3,), "field"),          # 3-D: nz one past, ny exact
          ((1, 1, 1, 1), (2, 3), "field"),        # one voxel: E = 0, the loop runs out, out == f
          ((1, 1, 1025, 65), (2,), "field"),      # 2-D: 33 x 2 = 66 tiles, the second round of the reduce kernel's lane loop
          ((2, 33, 57, 5), (3,), "field")]        # 3-D: 9 x 8 x 1 = 72 tiles, over 64 and no multiple of 64
CASES = [(shape, dims) for shape, dim_list, _ in SHAPES for dims in dim_list]
KIND = {shape: kind for shape, _, kind in SHAPES}
SEVERAL_X_TILES_RAGGED = (2, 2, 3, 67)  # the entry the stop-rule test adds to its own stack


def case_id(c):
    shape, dims = c
    return "x".join(map(str, shape)) + f"-{dims}d"


def tiles(shape, dims):
    """Tiles of one problem: the arithmetic of tv_plan (csrc/t2fit_denoise.hip), restated."""
    _, nz, ny, nx = shape

    def cdiv(a, b):
        return -(-a // b)

    return cdiv(ny, 32) * cdiv(nx, 64) if dims == 2 else cdiv(nz, 4) * cdiv(ny, 8) * cdiv(nx, 64)


assert tiles((1, 1, 1025, 65), 2) == 66 and 65 <= tiles((2, 33, 57, 5), 3) <= 127
assert tiles((1, 3, 256, 256), 2) == 32

# max |statement - reference| <= TOL_p * eps_p * max |f| for `out`, |E - E_ref| <= TOL_p * eps_p * E_ref for the energy
# (eps_f32 = 2^-24, eps_f64 = 2^-53).  16 times the largest ratio the statement shows over CASES and KS
# (test_denoise_host.py prints every case's).  MEASURED_RATIO[p] = (out's largest, the energy's largest).
# Both of out's are reached on WORST_OUT at k = 40; on every other case out's ratio stays below 5 at every k, except the
# other 2-D case of many tiles, (1, 1, 1025, 65), with 47.  On the 256 x 256 picture the ratio is below 2.3 up to k = 15 and
# then doubles about every ten updates, inside the bright disc, in both precisions alike: tau = 1 / (2 dims) is the edge
# of the linear part's stability (the checkerboard mode of I - tau grad grad^T has eigenvalue -1), so on a large flat
# region a rounding error is carried along and not damped.  It is the iteration's own sensitivity, not an error of
# either side: a wrong term shows at k = 1 or 2 already, where the ratios are below 2 (MUTATIONS below).
# The energy's are reached on WORST_ENERGY, 2-D: columns of 17 voxels of background (25) around a few of 1500, where E
# is small against weight * eps * max |f|, the absolute error of one |g|.
MEASURED_RATIO = {"f32": (200.2, 79.8), "f64": (309.7, 71.7)}
WORST_OUT, WORST_ENERGY = ((1, 3, 256, 256), 2), ((2, 16, 17, 1), 2)
TOL = {p: 16 * max(MEASURED_RATIO[p]) for p in MEASURED_RATIO}


def picture(shape, seed, sigma=20.0):
    """Piecewise-constant slices (blocks of 300 / 900 / 1500 over a zero background) under Rician noise, and the clean
    slices."""
    rng = np.random.default_rng(seed)
    n, z, y, x = shape
    yy, xx = np.meshgrid(np.arange(y), np.arange(x), indexing="ij")
    clean = np.zeros(shape)
    for v in range(n):
        for k in range(z):
            img = np.where((yy > y // 5) & (xx > x // 6), 300.0, 0.0)
            img = np.where((yy > y // 2) & (xx < x // 2 + k), 900.0 + 50.0 * v, img)
            img = np.where((yy - y / 2) ** 2 + (xx - x / 2) ** 2 < (min(y, x) / 5 + k) ** 2, 1500.0, img)
            clean[v, k] = img
    noisy = np.hypot(clean + rng.normal(scale=sigma, size=shape), rng.normal(scale=sigma, size=shape))
    return noisy.astype(np.float32), clean


def field(shape, seed, sigma=20.0):
    """Steps along every axis plus noise, all values in the hundreds (float32 rounding matters at every voxel), another
    level in every volume."""
    rng = np.random.default_rng(seed)
    n, nz, ny, nx = shape
    v, z, y, x = np.meshgrid(np.arange(n), np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    clean = 300.0 + 600.0 * (2 * x >= nx) + 400.0 * (2 * y >= ny) + 200.0 * (z % 2) + 50.0 * v
    return (clean + rng.normal(scale=sigma, size=shape)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def stack(shape):
    """The input of a case of the table, float32 (n_vol, nz, ny, nx), read-only."""
    a = picture(shape, seed=11)[0] if KIND[shape] == "picture" else field(shape, seed=sum(shape) * 7919)
    a.setflags(write=False)
    return a


def problems(a, dims):
    """The problems of a stack, in memory order."""
    a = np.asarray(a)
    return a.reshape((-1,) + a.shape[-2:]) if dims == 2 else a.reshape((-1,) + a.shape[-3:])


# ---- reference 1: Chambolle's iteration from the point-wise definition, in extended precision ------------------------------
# ROF: minimise 0.5 |u - f|^2 + weight TV(u), TV(u) = sum_x |(grad u)(x)|, (grad u)_a(x) = u(x + e_a) - u(x), 0 where x + e_a
# is outside.  With div = -grad^T, (div p)(x) = sum_a p_a(x) - p_a(x - e_a) with p_a(x - e_a) = 0 outside, the minimiser is
# u = f - div p for the dual field p with |p(x)| <= weight that Chambolle's projection iteration finds:
#   p <- (p - tau grad u) / (1 + (tau / weight) |grad u|),  u = f - div p,  p = 0 at the start,  tau = 1 / (2 dims).
# The energy scikit-image monitors at an iteration is (sum (div p)^2 + weight sum |grad u|) / N.
def ref_grad(u):
    """Forward differences: pad every axis by its own last sample, so the difference past the edge is 0."""
    return np.stack([np.diff(np.pad(u, [(0, int(b == a)) for b in range(u.ndim)], mode="edge"), axis=a)
                     for a in range(u.ndim)])


def ref_div(p):
    """Backward differences of p_a along a, p_a = 0 before the first sample, summed over the axes."""
    n = p.shape[0]
    return sum(np.diff(np.pad(p[a], [(int(b == a), 0) for b in range(n)], mode="constant"), axis=a) for a in range(n))


def ref_run(f, weight, ks):
    """{k: (u after k updates of p, the energy of iteration k)} in longdouble, for every k of ``ks``."""
    f = np.asarray(f).astype(LD)
    w, tau = LD(weight), LD(1) / LD(2 * f.ndim)
    p = np.zeros((f.ndim,) + f.shape, LD)
    found = {}
    for k in range(max(ks) + 1):
        div = ref_div(p)
        u = f - div
        g = ref_grad(u)
        norm = np.sqrt((g * g).sum(axis=0))
        if k in ks:
            found[k] = (u, ((div * div).sum() + w * norm.sum()) / LD(f.size))
        p = (p - tau * g) / (LD(1) + (tau / w) * norm)
    return found


def ref_updates(f, weight, k):
    """``u = f - div p`` after ``k`` updates of p."""
    return ref_run(f, weight, (k,))[k][0]


def ref_energy(f, weight, k):
    """The energy ``(sum d^2 + weight sum |g|) / N`` of iteration ``k`` (p updated ``k`` times before it)."""
    return ref_run(f, weight, (k,))[k][1]


@functools.lru_cache(maxsize=None)
def ref_case(shape, dims):
    """ref_run at KS for every problem of a case of the table (the same for both precisions: computed once)."""
    return [ref_run(f, WEIGHT, KS) for f in problems(stack(shape), dims)]


def statement_ratios(shape, dims, precision):
    """The statement's largest error ratios against the reference over the problems of a case and KS:
    ``(max |out - ref| / (eps max |f|), max |E - E_ref| / (eps E_ref))``."""
    eps = LD(EPS[precision])
    worst_out = worst_e = 0.0
    for f, ref in zip(problems(stack(shape), dims), ref_case(shape, dims)):
        top = LD(np.max(np.abs(f)))
        for k in KS:
            out, n_iter, e = _tv.tv_problem(f, WEIGHT, 0.0, k + 1, DTYPE[precision])
            assert n_iter == k and out.dtype == DTYPE[precision]
            u, e_ref = ref[k]
            worst_out = max(worst_out, float(np.max(np.abs(out.astype(LD) - u)) / (eps * top)))
            if e_ref == 0:
                assert e == 0.0  # one voxel, or a flat problem
            else:
                worst_e = max(worst_e, float(abs(LD(e) - e_ref) / (eps * e_ref)))
    return worst_out, worst_e


def check_statement(shape, dims, precision):
    r_out, r_e = statement_ratios(shape, dims, precision)
    assert r_out <= TOL[precision] and r_e <= TOL[precision], (shape, dims, precision, r_out, r_e, TOL[precision])
    return r_out, r_e


# ---- reference 2: the exact minimiser in one dimension -----------------------------------------------------------------------
# A problem of shape (n, 1), (1, n) or (n, 1, 1) is 1-D total variation: minimise 0.5 |u - f|^2 + weight sum |u[i+1] - u[i]|.
# Its dual: u = f - D^T z with z the minimiser of |f - D^T z|^2 over |z| <= weight (D the (n - 1) x n difference matrix),
# a bounded least-squares problem that an active-set solver settles exactly up to rounding.
ONE_D = [(33, 5.0), (48, 20.0), (48, 60.0)]
KKT = 1e-9


def one_d_signal(n):
    """Three steps (300 / 900 / 500) under noise of sigma 20; float32, as the device takes it."""
    i = np.arange(n)
    clean = np.where(i < n // 3, 300.0, np.where(i < 2 * n // 3, 900.0, 500.0))
    return (clean + np.random.default_rng(1000 + n).normal(scale=20.0, size=n)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def exact_1d(n, weight):
    """(f float32, the exact minimiser u float64) of a case; asserts the KKT conditions on the solver's own result."""
    from scipy.optimize import lsq_linear

    f = one_d_signal(n)
    d = np.diff(np.eye(n), axis=0)
    res = lsq_linear(d.T, f.astype(np.float64), bounds=(-weight, weight), method="bvls", tol=1e-15, max_iter=10 * n)
    z = res.x
    u = f.astype(np.float64) - d.T @ z
    jump = d @ u
    assert res.status > 0 and np.all(np.abs(z) <= weight + KKT)
    at = np.abs(jump) > KKT                     # where u jumps, z sits on the bound of the jump's sign ..
    assert at.any() and np.all(np.abs(z[at] - weight * np.sign(jump[at])) <= KKT)
    assert np.all(np.abs(jump[np.abs(z) < weight - KKT]) <= KKT)  # .. and u is flat where z is strictly inside
    for a in (f, u):
        a.setflags(write=False)
    return f, u


ONE_D_FORMS = {"column": (2, lambda n: (1, 1, n, 1)), "row": (2, lambda n: (1, 1, 1, n)), "volume": (3, lambda n: (1, n, 1, 1))}

# K: the smallest max_iter at which the float64 statement (eps = 0) is within 1e-6 of the exact u on every case of ONE_D in
# every form; at K - 1 one of them is not.  STATEMENT_DISTANCE: the largest distance at K, float64 (the reference's own
# distance from the exact minimiser) and float32 (the device's float32 bar is twice that).  After 20000 iterations the
# float64 statement is within ONE_D_CONVERGED of the exact u.  Measured on the CPU (test_denoise_host.py keeps them current).
# K is set by (48, 60.0) as a volume (tau = 1 / 6); as a row or column it is within 1e-6 from 4052 on; (33, 5.0) from 254
# (378 as a volume), (48, 20.0) from 1478 (2219).  The solution for twice or half the weight lies 5 to 15 intensity units
# away from u on every case: a wrong scaling of the weight cannot pass.
K = 6077
STATEMENT_DISTANCE = {"f64": 9.985e-7, "f32": 3.445e-4}
ONE_D_CONVERGED = 1.54e-12


@functools.lru_cache(maxsize=None)
def statement_1d(n, weight, form, max_iter, precision="f64"):
    """The statement on a 1-D case: (result as a vector in the working precision, its distance from the exact u)."""
    f, u = exact_1d(n, weight)
    dims, shape = ONE_D_FORMS[form]
    out, n_iter, _ = _tv.tv_problem(f.reshape(shape(n)[-dims:]), weight, 0.0, max_iter, DTYPE[precision])
    assert n_iter == max_iter - 1
    out = out.reshape(-1)
    out.setflags(write=False)
    return out, float(np.max(np.abs(out.astype(np.float64) - u)))


# ---- the stop rule's cases -----------------------------------------------------------------------------------------------------
STOP_WEIGHTS = (0.1, 10.0, 20.0, 40.0)
STOP_MARGIN = 1e-9  # | |E_prev - E| - eps E_init | >= STOP_MARGIN * E_init; the kernel's sums differ from np.sum by ~1e-12


@functools.lru_cache(maxsize=None)
def stop_stacks():
    """The stacks of the stop-rule test: the picture, and an entry of the table with several x tiles and a ragged quad."""
    a = picture((2, 6, 96, 80), seed=5)[0]
    b = np.array(stack(SEVERAL_X_TILES_RAGGED))
    for s in (a, b):
        s.setflags(write=False)
    return a, b


def stop_margins(a, weight, dims, precision, eps=_tv.DEFAULT_EPS, max_iter=_tv.DEFAULT_MAX_ITER):
    """By the statement: (n_iter of every problem, the smallest | |E_prev - E| - eps E_init | / E_init over every
    iteration of every problem)."""
    n_iter, margin = [], np.inf
    for f in problems(a, dims):
        hist = []
        _, n, _ = _tv.tv_problem(f, weight, eps, max_iter, DTYPE[precision], history=hist)
        n_iter.append(n)
        e_prev = hist[0]
        for e in hist[1:]:  # e_prev moves at every iteration that does not stop, and the stopping one is the last
            margin = min(margin, abs(abs(e_prev - e) - eps * hist[0]) / hist[0])
            e_prev = e
    return np.array(n_iter), margin


# ---- mutations of the statement: each must miss a bar above on the case named beside it ----------------------------------------
_step_sizes, _divergence, _gradient, _update, _energy = _tv.step_sizes, _tv.divergence, _tv.gradient, _tv.update, _tv.energy


def _gradient_halo_column_zero(out):
    g = _gradient(out)
    xs = np.arange(63, out.shape[-1] - 1, 64)
    g[-1][..., xs] = 0 - out[..., xs]
    return g


def _divergence_without_x_term_at_tile_start(p):
    d = _divergence(p)
    xs = np.arange(64, d.shape[-1], 64)
    d[..., xs] = d[..., xs] - p[-1][..., xs - 1]
    return d


def _update_skips_ragged_quad(p, g, nrm, tau, tw):
    new = _update(p, g, nrm, tau, tw)
    nx = nrm.shape[-1]
    if nx % 4:
        for a in range(len(p)):
            new[a][..., nx // 4 * 4:] = p[a][..., nx // 4 * 4:]
    return new


def _steps_tau_times_weight(n, weight, T):
    return _step_sizes(n, weight, T)[0], T((1.0 / (2.0 * n)) * float(weight))


def _steps_half_weight(n, weight, T):
    return _step_sizes(n, 0.5 * weight, T)


def _gradient_backward(out):
    g = []
    for a in range(out.ndim):
        ga = np.zeros(out.shape, out.dtype)
        ga[_tv._lo(out.ndim, a)] = out[_tv._lo(out.ndim, a)] - out[_tv._hi(out.ndim, a)]
        g.append(ga)
    return g


def _gradient_last_not_zeroed(out):
    return [np.roll(out, -1, axis=a) - out for a in range(out.ndim)]


def _energy_over_n_minus_1(d, nrm, weight):
    return _energy(d, nrm, weight) * d.size / (d.size - 1)


# name: (the attribute of _tv, the wrong variant, the case of the table, or "1d" for the exact minimiser, that notices)
MUTATIONS = {"halo_column_read_as_zero": ("gradient", _gradient_halo_column_zero, ((2, 2, 3, 65), 2)),
             "x_term_of_d_dropped_at_a_tile_start": ("divergence", _divergence_without_x_term_at_tile_start, ((2, 2, 3, 65), 3)),
             "ragged_last_quad_left_unchanged": ("update", _update_skips_ragged_quad, ((2, 2, 3, 67), 2)),
             "tau_times_weight": ("step_sizes", _steps_tau_times_weight, "1d"),
             "weight_halved_in_the_update": ("step_sizes", _steps_half_weight, "1d"),
             "gradient_taken_backward": ("gradient", _gradient_backward, ((2, 2, 3, 5), 3)),
             "last_difference_not_zeroed": ("gradient", _gradient_last_not_zeroed, ((2, 2, 3, 5), 2)),
             "energy_over_n_minus_1": ("energy", _energy_over_n_minus_1, ((2, 5, 9, 7), 3))}


@contextlib.contextmanager
def mutated(name):
    attr, fn, _ = MUTATIONS[name]
    saved = getattr(_tv, attr)
    setattr(_tv, attr, fn)
    try:
        yield
    finally:
        setattr(_tv, attr, saved)


def check_1d(max_iter, bar):
    """The float64 statement within ``bar`` of the exact minimiser on every 1-D case and form."""
    worst = 0.0
    for n, weight in ONE_D:
        for form in ONE_D_FORMS:
            dist = statement_1d(n, weight, form, max_iter)[1]
            assert dist <= bar, (n, weight, form, max_iter, dist, bar)
            worst = max(worst, dist)
    return worst
