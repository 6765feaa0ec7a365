"""Slice-to-volume registration, restated in numpy: the executable statement of t2fit_svr_sums_dev (include/t2fit.h) and the
host code -- transform model, table packing, lockstep descent, driver -- that the statement and the device path both run.
It finds the per-slice poses ``reconstruct_sr(..., slice_transforms=)`` takes: every slice of every stack is registered
rigidly onto the current volume with the correlation metric of :mod:`_register`, all slices at once.

**Per slice.**  The fixed image is plane ``k`` of a stack with the stack's mask plane, the moving image the volume; ``A_k``
maps the slice index ``(ix, iy, k)`` to a continuous index of the volume.  What a voxel adds to the 43 sums is literally
``_register._terms(stack, mask, volume, volume_mask, A_k, k, 1)``: the counting rule, ``m``, ``g_a``, the flat rule and the
rounding order of the volume registration, with ``u_z = k``.

**The slice tree** (a function of ``(ly, lx)`` alone; it differs from the volume's because a slice has no z to walk before
the cross-lane exchange).  Bricks of ``SBX x SBY = 64 x 32`` voxels, padded with zeros.  In a brick, column ``x`` of row
group ``w`` adds its rows ``y = 32 by + 8 w + r``, ``r = 0..7``, in order from 0.0; the 64 columns of a row group are added
by halving; the 4 row groups by halving, ``(w0 + w2) + (w1 + w3)``.  The slabs, in ``(by, bx)`` order, go through
:func:`_register.reduce_slabs`.  The device pads every slice of a batch with slabs of +0.0 up to the largest slab count,
which changes no bit.

**Batch.**  ``K`` records ``(A, stack, slice, active)`` in any order give ``(K, 43)``; an inactive record, or one whose
stack or slice index is out of range, gives a row of +0.0, and so does a non-finite ``A`` (it counts no voxel).

**Transform model.**  For slice ``k`` of stack ``s`` with stack transform ``T_s`` (fixed point -> stack point) the optimized
map is ``F_k(p) = inv(T_s) compose(p, c_k)`` (stack point -> volume point), ``p`` as in :func:`_register.compose``, ``c_k``
the physical centroid of the slice's mask voxels, the scales those of :func:`_register.mask_centre_and_scales` over that
slice's mask alone; ``A_k = index_affine(stack geometry, H, F_k(p))``; ``p = 0`` is the stack's own pose; the pose
``reconstruct_sr`` takes is ``inv(F_k(p))``."""
from __future__ import annotations

import numpy as np

from . import _register, _resample, _sr

SBX, SBY, ROWS = 64, 32, 8
_ROW_ORDER = tuple(range(ROWS))  # the order in which a lane adds its rows: part of the definition
N_SUMS = _register.N_SUMS
RECORD_BYTES = 128
MAX_STACKS = _sr.MAX_STACKS
STEP, MIN_STEP, MAX_ITER, GRAD_TOL, MIN_COUNT = 1.0, 1e-3, 60, 1e-6, 64


# ---- the sums ------------------------------------------------------------------------------------------------------------
def slice_brick_counts(ly, lx):
    """(bricks_y, bricks_x) of a slice of ``ly x lx`` voxels."""
    return -(-int(ly) // SBY), -(-int(lx) // SBX)


def workspace_bytes(lo_shapes, n_slices):
    """What t2fit_svr_workspace_bytes returns: every pass's input over ``43 n_slices`` rows, each rounded up to 256 bytes;
    the slab count is the largest of any stack."""
    n0 = max(int(np.prod(slice_brick_counts(s[1], s[2]))) for s in lo_shapes)
    return sum((N_SUMS * 8 * int(n_slices) * n + 255) // 256 * 256 for n in _register.pass_sizes(n0))


def slice_slabs(stack, mask, volume, volume_mask, A, k):
    """float64 ``(43, n_slabs)``: the slab of every brick of slice ``k`` of ``stack`` ``(lz, ly, lx)``, bricks in
    ``(by, bx)`` order.  ``mask`` / ``volume_mask``: uint8 arrays of the shapes of ``stack`` / ``volume``."""
    _, ly, lx = stack.shape
    nby, nbx = slice_brick_counts(ly, lx)
    a = np.asarray(A, np.float64).reshape(3, 4)
    if not np.all(np.isfinite(a)):  # the inside test is false for NaN: no voxel counts
        return np.zeros((N_SUMS, nby * nbx), np.float64)
    with np.errstate(all="ignore"):
        t = _register._terms(stack, mask, volume, volume_mask, a, int(k), 1)[:, 0]
        pad = np.zeros((N_SUMS, nby * SBY, lx), np.float64)
        pad[:, :ly] = t
        pad = pad.reshape(N_SUMS, nby, SBY // ROWS, ROWS, lx)
        acc = np.zeros((N_SUMS, nby, SBY // ROWS, lx), np.float64)
        for r in _ROW_ORDER:
            acc = acc + pad[:, :, :, r]
        cols = np.zeros((N_SUMS, nby, SBY // ROWS, nbx * SBX), np.float64)
        cols[..., :lx] = acc
        groups = _register._halve(cols.reshape(N_SUMS, nby, SBY // ROWS, nbx, SBX))  # the 64 columns of a row group
        out = _register._halve(np.moveaxis(groups, 2, -1))                             # the 4 row groups
    return out.reshape(N_SUMS, -1)


def _check_stacks(stacks, masks):
    stacks = [np.asarray(v, np.float32) for v in stacks]
    if not 1 <= len(stacks) <= MAX_STACKS:
        raise ValueError(f"between 1 and {MAX_STACKS} stacks, got {len(stacks)}")
    if any(v.ndim != 3 for v in stacks):
        raise ValueError("a stack is a (Z, Y, X) volume")
    masks = [None] * len(stacks) if masks is None else list(masks)
    if len(masks) != len(stacks):
        raise ValueError("one mask (or None) per stack")
    out = []
    for v, m in zip(stacks, masks):
        m = np.ones(v.shape, np.uint8) if m is None else (np.asarray(m) != 0).astype(np.uint8)
        if m.shape != v.shape:
            raise ValueError("a mask has the shape of its stack")
        out.append(m)
    return stacks, out


def check_records(A, stack, slice_, active):
    """``(A (K, 3, 4) float64, stack int32, slice int32, active uint8)`` after the shape refusals."""
    a = np.ascontiguousarray(A, np.float64)
    if a.ndim < 2 or a.shape[0] < 1 or a[0].size != 12:
        raise ValueError(f"one 3 x 4 affine per record, (K, 3, 4) with K >= 1, got shape {a.shape}")
    a = a.reshape(-1, 3, 4)
    s, k = np.ascontiguousarray(stack, np.int32).ravel(), np.ascontiguousarray(slice_, np.int32).ravel()
    act = np.ones(len(a), np.uint8) if active is None else np.ascontiguousarray(np.asarray(active) != 0).view(np.uint8).ravel()
    if not len(s) == len(k) == len(act) == len(a):
        raise ValueError("A, stack, slice and active have one entry per record")
    return a, s, k, act


def slice_sums(stacks, volume, A, stack, slice_, *, active=None, stack_masks=None, volume_mask=None):
    """float64 ``(K, 43)``: the sums of record ``r`` = slice ``slice_[r]`` of ``stacks[stack[r]]`` sampled from ``volume`` at
    ``A[r]`` (module docstring).  ``stacks``: a list of float32 ``(Z, Y, X)``; masks None: all ones.  The statement of
    ``t2map.register.slice_sums``."""
    stacks, masks = _check_stacks(stacks, stack_masks)
    volume = np.asarray(volume, np.float32)
    if volume.ndim != 3:
        raise ValueError("volume is a (Z, Y, X) volume")
    vmask = np.ones(volume.shape, np.uint8) if volume_mask is None else (np.asarray(volume_mask) != 0).astype(np.uint8)
    if vmask.shape != volume.shape:
        raise ValueError("a mask has the shape of its volume")
    a, s, k, act = check_records(A, stack, slice_, active)
    out = np.zeros((len(a), N_SUMS), np.float64)
    for r in range(len(a)):
        if act[r] and 0 <= s[r] < len(stacks) and 0 <= k[r] < stacks[s[r]].shape[0]:
            out[r] = _register.reduce_slabs(slice_slabs(stacks[s[r]], masks[s[r]], volume, vmask, a[r], k[r]))
    return out


def pack_table(A, stack, slice_, active, lo_shapes):
    """The table of t2fit_svr_table_host in numpy: uint8 ``[128 K]``, per record ``A[12]`` float64, int32 stack, slice,
    active, 5 zero words.  Refuses what the entry point refuses: a non-finite ``A``, an index out of range."""
    a, s, k, act = check_records(A, stack, slice_, active)
    if not 1 <= len(lo_shapes) <= MAX_STACKS or any(len(v) != 3 or min(v) < 1 for v in lo_shapes):
        raise ValueError(f"between 1 and {MAX_STACKS} stacks of sizes >= 1")
    if not np.all(np.isfinite(a)):
        raise ValueError("A has a non-finite entry")
    if np.any(s < 0) or np.any(s >= len(lo_shapes)):
        raise ValueError("a stack index is outside 0 .. n_stacks - 1")
    if np.any(k < 0) or np.any(k >= np.array([v[0] for v in lo_shapes], np.int64)[s]):
        raise ValueError("a slice index is outside its stack")
    table = np.zeros((len(a), RECORD_BYTES), np.uint8)
    table[:, :96] = a.reshape(len(a), 12).view(np.uint8)
    table[:, 96:108] = np.stack([s, k, act.astype(np.int32)], axis=1).astype(np.int32).view(np.uint8)
    return table.reshape(-1)


# ---- transform model -------------------------------------------------------------------------------------------------------
def _inverse(t):
    return np.linalg.inv(np.asarray(t, np.float64))


class SliceModel:
    """The transform model of the slices of one stack: ``centres (lz, 3)``, ``scales (lz, 6)``, ``valid (lz,)`` (the slice's
    mask is not empty; an empty slice keeps the physical centre of its plane and unit scales so that its pose stays
    defined), and the affines, poses and gradients of a parameter vector."""

    def __init__(self, stack_geom, mask, volume_geom, transform=None):
        self.geom = _resample.as_geometry(stack_geom, np.asarray(mask).shape)
        self.volume_geom = _resample.as_geometry(volume_geom)
        t = np.eye(4) if transform is None else np.asarray(transform, np.float64)
        if t.shape != (4, 4) or not np.all(np.isfinite(t)):
            raise ValueError("a stack transform must be a finite 4 x 4 matrix")
        self.inv_t = _inverse(t)
        # inv(T_s) folded into the moving geometry: direction and origin of H moved by T_s, so that
        # _register.parameter_gradient applies unchanged
        m, o = _resample._index_to_point(self.volume_geom)
        spacing = np.asarray(self.volume_geom.GetSpacing(), np.float64)
        self.moved = _resample.Geometry(self.volume_geom.GetSize(), spacing, t[:3, :3] @ o + t[:3, 3], (t[:3, :3] @ m) / spacing[None, :])
        mask = np.asarray(mask) != 0
        lz, ly, lx = mask.shape
        ms, os_ = _resample._index_to_point(self.geom)
        self.centres, self.scales, self.valid = np.zeros((lz, 3)), np.ones((lz, 6)), np.zeros(lz, bool)
        for k in range(lz):
            if mask[k].any():
                only = np.zeros(mask.shape, np.uint8)
                only[k] = mask[k]
                self.centres[k], self.scales[k] = _register.mask_centre_and_scales(only, self.geom)
                self.valid[k] = True
            else:
                self.centres[k] = os_ + ms @ np.array([(lx - 1) / 2.0, (ly - 1) / 2.0, float(k)])

    def forward(self, k, p):
        """``F_k(p)``, 4 x 4, stack point -> volume point."""
        return self.inv_t @ _register.compose(p, self.centres[k])

    def affine(self, k, p):
        return _resample.index_affine(self.geom, self.volume_geom, self.forward(k, p))

    def pose(self, k, p):
        """``inv(F_k(p))``, fixed point -> stack point: an entry of ``slice_transforms``."""
        return _inverse(self.forward(k, p))

    def gradient(self, k, p, dc_da):
        """The scaled gradient ``(dC/dp_i) / scale_i``."""
        return _register.parameter_gradient(dc_da, p, self.centres[k], self.geom, self.moved) / self.scales[k]


# ---- descent -----------------------------------------------------------------------------------------------------------
STATUSES = ("gradient", "step", "iterations", "rejected", "lost")


def _evaluate(sums, min_count):
    """``(C, dC/dA)`` of a row of sums, or None where there is no metric: fewer than ``min_count`` voxels count, or
    :func:`_register.metric` is undefined."""
    if not sums[0] >= float(min_count):
        return None
    try:
        return _register.metric(sums)
    except ValueError:
        return None


def descend(evaluate, models, records, init, *, step=STEP, min_step=MIN_STEP, max_iter=MAX_ITER, grad_tol=GRAD_TOL,
            min_count=MIN_COUNT):
    """The regular-step descent of :func:`_register.optimize` for every record ``(s, k)`` independently, all in lockstep:
    one call ``evaluate(A (K, 3, 4), active (K,)) -> (K, 43)`` per iteration; a finished slice is inactive from then on.
    Returns ``(p (K, 6), metric (K,), iterations (K,), status list)``.  Nothing a slice does raises: no metric at the
    first evaluation is 'rejected' (``p`` stays ``init``), no metric later is 'lost' (``p`` goes back to the last one that
    had a metric)."""
    n = len(records)
    p = np.array(init, np.float64).reshape(n, 6)
    steps, prev, n_it = np.full(n, float(step)), [None] * n, np.zeros(n, np.int64)
    last_p, cost, status = p.copy(), np.full(n, np.nan), [None] * n
    for r, (s, k) in enumerate(records):
        if not models[s].valid[k]:
            status[r] = "rejected"
    a = np.zeros((n, 3, 4), np.float64)
    while any(v is None for v in status):
        active = np.array([v is None for v in status], np.uint8)
        for r, (s, k) in enumerate(records):
            if active[r]:
                a[r] = models[s].affine(k, p[r])
        sums = np.asarray(evaluate(a, active), np.float64)
        for r, (s, k) in enumerate(records):
            if not active[r]:
                continue
            found = _evaluate(sums[r], min_count)
            if found is None:
                status[r] = "rejected" if n_it[r] == 0 else "lost"
                p[r] = last_p[r]
                continue
            cost[r], last_p[r] = found[0], p[r]
            g = models[s].gradient(k, p[r], found[1])
            norm = float(np.sqrt(np.sum(g * g)))
            if not norm >= grad_tol:  # (a NaN gradient ends the slice too)
                status[r] = "gradient"
                continue
            if prev[r] is not None and float(np.sum(g * prev[r])) < 0.0:
                steps[r] *= _register.RELAX
            if steps[r] < min_step:
                status[r] = "step"
                continue
            if n_it[r] >= max_iter:
                status[r] = "iterations"
                continue
            p[r] = p[r] - (steps[r] / norm) * g
            prev[r], n_it[r] = g, n_it[r] + 1
    return p, cost, n_it, status


class SliceRegistration:
    """Per stack name: ``transforms (lz, 4, 4)`` (fixed point -> stack point, what ``reconstruct_sr(slice_transforms=)``
    and ``recon.py --sr_slice_transforms`` read), ``parameters (lz, 6)`` about ``centres (lz, 3)``, ``metric (lz,)`` at the
    returned parameters (NaN where a slice never had one), ``iterations (lz,)`` and ``status`` (a list per stack of
    'gradient', 'step', 'iterations', 'rejected' or 'lost')."""

    def __init__(self, transforms, parameters, centres, metric, iterations, status):  # noqa: A002
        self.transforms, self.parameters, self.centres = transforms, parameters, centres
        self.metric, self.iterations, self.status = metric, iterations, status

    def __repr__(self):
        return "SliceRegistration(" + ", ".join(
            f"{o}: {len(v)} slices, {sum(s in ('rejected', 'lost') for s in v)} without a pose" for o, v in self.status.items()) + ")"


def check_init(init, names, lzs):
    """``{name: (lz, 6)}`` -> the parameters of every record, stack by stack; None: zeros."""
    out = []
    init = init or {}
    unknown = [o for o in init if o not in names]
    if unknown:
        raise ValueError(f"init is given per stack {list(names)}, got {unknown}")
    for o, lz in zip(names, lzs):
        q = np.zeros((lz, 6)) if o not in init else np.asarray(init[o], np.float64)
        if q.shape != (lz, 6) or not np.all(np.isfinite(q)):
            raise ValueError(f"init of stack {o!r} must be finite (lz, 6) = ({lz}, 6), got shape {q.shape}")
        out.append(q)
    return np.concatenate(out)


def check_options(max_iter, step, min_step, min_count):
    if int(max_iter) < 0 or not (float(step) > 0.0 and np.isfinite(step)) or not float(min_step) >= 0.0 or int(min_count) < 1:
        raise ValueError("max_iter >= 0, step finite and > 0, min_step >= 0, min_count >= 1")


def register_with(evaluate, names, geoms, masks, volume_geom, transforms, init, **options):
    """The host half of ``register_slices``: models, records (stack by stack, slice by slice), descent, result.  ``masks``:
    host uint8 arrays, one per stack of ``names``."""
    transforms = transforms or {}
    unknown = [o for o in transforms if o not in names]
    if unknown:
        raise ValueError(f"transforms are given per stack {list(names)}, got {unknown}")
    models = [SliceModel(geoms[o], m, volume_geom, transforms.get(o)) for o, m in zip(names, masks)]
    lzs = [int(np.asarray(m).shape[0]) for m in masks]
    records = [(s, k) for s, lz in enumerate(lzs) for k in range(lz)]
    p, cost, n_it, status = descend(evaluate, models, records, check_init(init, names, lzs), **options)
    at = np.concatenate([[0], np.cumsum(lzs)])
    cut = lambda v, s: v[at[s]:at[s + 1]]
    return SliceRegistration(
        {o: np.stack([models[s].pose(k, cut(p, s)[k]) for k in range(lzs[s])]) for s, o in enumerate(names)},
        {o: cut(p, s).copy() for s, o in enumerate(names)}, {o: models[s].centres.copy() for s, o in enumerate(names)},
        {o: cut(cost, s).copy() for s, o in enumerate(names)}, {o: cut(n_it, s).copy() for s, o in enumerate(names)},
        {o: list(cut(status, s)) for s, o in enumerate(names)})


def _stack_names(stacks, geoms):
    names = [o for o in geoms if o in stacks]
    if not 1 <= len(names) <= MAX_STACKS:
        raise ValueError(f"between 1 and {MAX_STACKS} stacks, got {len(names)}")
    return names


def register_slices(stacks, geoms, volume, volume_geom, *, transforms=None, stack_masks=None, volume_mask=None, echo=0, init=None,
                    max_iter=MAX_ITER, step=STEP, min_step=MIN_STEP, min_count=MIN_COUNT):
    """Register every slice of every stack onto ``volume`` (module docstring).  ``stacks`` / ``geoms``: {name: float32
    ``(Z, Y, X)`` or ``(nTE, Z, Y, X)``, of which ``echo`` is used} and their geometries; ``volume``: float32 ``(Z, Y, X)``
    on ``volume_geom``; ``transforms``: {name: 4 x 4, fixed point -> stack point}; ``stack_masks``: {name: ``(Z, Y, X)``},
    a stack without one gets :func:`_register.build_mask`; ``init``: {name: ``(lz, 6)``}.  Returns a
    :class:`SliceRegistration`.  The statement of ``t2map.register.register_slices``."""
    check_options(max_iter, step, min_step, min_count)
    names = _stack_names(stacks, geoms)
    ys = []
    for o in names:
        v = np.asarray(stacks[o], np.float32)
        if v.ndim not in (3, 4):
            raise ValueError(f"stack {o!r} must be (Z, Y, X) or (nTE, Z, Y, X), got shape {v.shape}")
        ys.append(v if v.ndim == 3 else v[int(echo)])
    stack_masks = stack_masks or {}
    masks = [_register.build_mask(y) if stack_masks.get(o) is None else stack_masks[o] for o, y in zip(names, ys)]
    ys, masks = _check_stacks(ys, masks)
    volume = np.asarray(volume, np.float32)
    s_of = np.array([s for s, y in enumerate(ys) for _ in range(y.shape[0])], np.int32)
    k_of = np.array([k for y in ys for k in range(y.shape[0])], np.int32)

    def evaluate(a, active):
        return slice_sums(ys, volume, a, s_of, k_of, active=active, stack_masks=masks, volume_mask=volume_mask)

    return register_with(evaluate, names, geoms, masks, _resample.as_geometry(volume_geom, volume.shape), transforms, init,
                         max_iter=int(max_iter), step=float(step), min_step=float(min_step), min_count=int(min_count))


# ---- driver ------------------------------------------------------------------------------------------------------------
def drive(reconstruct, register, stacks, geoms, rounds, echo, slice_masks, volume_mask, options, sr):
    """The loop ``reconstruct_svr`` runs on either path: ``x <- merge`` (``reconstruct`` with no iteration), then per round
    ``found <- register(x[echo])`` warm-started from the last round and ``x <- reconstruct(slice_transforms=found.transforms)``."""
    if int(rounds) < 1:
        raise ValueError("rounds must be >= 1")
    if sr.get("slice_transforms") is not None or sr.get("return_info"):
        raise ValueError("reconstruct_svr finds the slice transforms itself and returns (x, H, found)")
    sr = {k: v for k, v in sr.items() if k not in ("slice_transforms", "return_info")}
    x, hi = reconstruct(stacks, geoms, **{**sr, "n_iter": 0})
    found = None
    for _ in range(int(rounds)):
        moving = x if len(x.shape) == 3 else x[int(echo)]
        # (the stack transforms the registration starts from are those reconstruct_sr was given; the fixed stack has none)
        found = register(stacks, geoms, moving, hi, transforms=dict(sr.get("transforms") or {}), stack_masks=slice_masks,
                         volume_mask=volume_mask, echo=echo, init=None if found is None else found.parameters, **options)
        x, hi = reconstruct(stacks, geoms, slice_transforms=found.transforms, **sr)
    return x, hi, found


def reconstruct_svr(stacks, geoms, *, rounds=2, echo=0, slice_masks=None, volume_mask=None, max_iter=MAX_ITER, step=STEP,
                    min_step=MIN_STEP, min_count=MIN_COUNT, **sr):
    """Motion-corrected super-resolution on the host: ``rounds`` of :func:`register_slices` against the current volume and
    :func:`_sr.reconstruct_sr` with the poses found, from the merge; every other keyword is ``reconstruct_sr``'s.
    ``slice_masks``: {name: mask} of the registration (None: ``build_mask``).  Returns ``(x, Geometry of H, found)``.  The
    statement of ``t2map.sr.reconstruct_svr``."""
    check_options(max_iter, step, min_step, min_count)
    return drive(_sr.reconstruct_sr, register_slices, stacks, geoms, rounds, echo, slice_masks, volume_mask,
                 dict(max_iter=max_iter, step=step, min_step=min_step, min_count=min_count), sr)
