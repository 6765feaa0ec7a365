"""Slice-to-volume registration without a device: the numpy statement (fetal_t2mapping_amd/_svr.py) against the
from-definition reference of tests/register_cases.py, the slice tree against math.fsum and against a lane-by-lane restatement
in Python floats (with three mutations of the statement that must fail), the parameter gradient against differences of the
statement's own metric, identity, independence of the records, inactive and out-of-range records, the status of slices that
cannot be registered, the table layout and every refusal of the four entry points through ctypes, and the recovery of the
poses of ``sr_slice_cases.moved_phantom()``.  tests/test_svr_gpu.py holds the device to the statement bit for bit."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import register_cases as RC
import sr_cases as K
import sr_slice_cases as L
import svr_cases as W
from fetal_t2mapping_amd import _abi
from fetal_t2mapping_amd import _register as G
from fetal_t2mapping_amd import _resample as R
from fetal_t2mapping_amd import _sr as S
from fetal_t2mapping_amd import _svr as V


def _same(a, b):
    return np.array_equal(RC.bits(a), RC.bits(b))


def _sums(b, **kw):
    return V.slice_sums(b.stacks, b.volume, b.A, b.stack, b.slice, stack_masks=b.masks, volume_mask=b.volume_mask, **kw)


def _within_reference(b, sums, with_masks=True):
    """N exact, every other sum within 16 x 4.6e-16 x sum |terms| (the bar of the volume registration); returns the
    largest ratio seen."""
    worst = 0.0
    for r in range(len(b.A)):
        ref, scale = b.reference(r, with_masks)
        assert sums[r][0] == ref[0], (r, sums[r][0], ref[0])
        assert np.array_equal(sums[r][scale == 0], ref[scale == 0]) and sums[r][42] == 0.0 and not np.signbit(sums[r][42])
        bad = np.flatnonzero(~(np.abs(sums[r] - ref) <= RC.TOL * scale))
        assert bad.size == 0, (r, bad, sums[r][bad], ref[bad], scale[bad])
        worst = max(worst, float(np.max(np.abs(sums[r] - ref)[scale > 0] / scale[scale > 0], initial=0.0)))
    return worst


def _check_statement_against_reference():
    b = W.mixed_batch()
    sums = _sums(b)
    n = sums[:, 0]
    # what the case is for: the exact pose and the rotated slice count, one slice is wholly off the grid, one partly, one
    # fully masked; slices k > 0 carry u_z = k
    assert n[0] > 200 and n[1] > 100 and n[2] == 0 and 0 < n[3] < n[0] and n[4] == 0 and np.all(n[5:] > 0)
    worst = _within_reference(b, sums)
    unmasked = V.slice_sums(b.stacks, b.volume, b.A, b.stack, b.slice)
    worst = max(worst, _within_reference(b, unmasked, with_masks=False))
    for name, e in W.edge_batch():
        s = _sums(e)
        assert s[1, 0] > 0, name
        worst = max(worst, _within_reference(e, s))
        if name == "edges":  # ix = 0 sits exactly on -0.5 and counts; ix = 5 and iy = 3 sit exactly on n - 0.5 and do not
            only = V.slice_sums(e.stacks, e.volume, e.A[1:2], [0], [1])
            assert only[0, 0] == 5 * 3, only[0, 0]
    return worst


def test_statement_is_within_the_bar_of_the_from_definition_reference():
    """Largest |s - ref| / sum |terms| measured over all cases: 2.8e-16, below the statement ratio 4.6e-16 of the volume
    registration; the bar is 16 times that ratio (register_cases.TOL)."""
    worst = _check_statement_against_reference()
    print(f"largest |s - ref| / scale {worst:.3g}")


TREE_SHAPES = {(1, 1): (1, [1]), (33, 65): (4, [4]), (8224, 3): (257, [257, 2]), (32, 64): (1, [1])}


def _check_tree(shapes=TREE_SHAPES):
    rng = np.random.default_rng(5)
    for (ly, lx), (n_slabs, passes) in shapes.items():
        assert int(np.prod(V.slice_brick_counts(ly, lx))) == n_slabs and G.pass_sizes(n_slabs) == passes
        assert V.workspace_bytes([(3, ly, lx)], 7) == sum((43 * 8 * 7 * n + 255) // 256 * 256 for n in passes)
        stack = rng.normal(500, 200, (2, ly, lx)).astype(np.float32)
        volume = rng.normal(500, 200, (4, 5, 6)).astype(np.float32)
        a = np.array([[4.0 / lx, 0, 0, 0.3], [0, 3.0 / ly, 0.1, 0.2], [0.01, 0, 1.0, 0.6]])  # the whole slice lands inside
        ones, vones = np.ones(stack.shape, np.uint8), np.ones(volume.shape, np.uint8)
        terms = G._terms(stack, ones, volume, vones, a, 1, 1)[:, 0]
        got = G.reduce_slabs(V.slice_slabs(stack, ones, volume, vones, a, 1))
        assert got[0] == ly * lx
        for q in range(43):
            exact, scale = math.fsum(terms[q].ravel().tolist()), math.fsum(np.abs(terms[q]).ravel().tolist())
            assert abs(got[q] - exact) <= 1e-12 * scale, ((ly, lx), q, got[q], exact)
        for q in ((2, 5, 23, 41) if ly * lx > 4000 else range(43)):  # bit for bit against the lane-by-lane tree
            by_hand, counted = W.tree_by_hand(terms[q])
            assert counted == n_slabs and _same(got[q], by_hand), ((ly, lx), q, got[q], by_hand)


def test_slice_tree_equals_fsum_and_the_lane_by_lane_tree():
    _check_tree()


def test_mutations_of_the_statement_fail(monkeypatch):
    """Rows added in another order, the ragged last group of a pass dropped, u_z = 0 instead of k: each must fail the tree
    test or the reference test."""
    with monkeypatch.context() as m:
        m.setattr(V, "_ROW_ORDER", tuple(reversed(range(V.ROWS))))
        with pytest.raises(AssertionError):
            _check_tree({(33, 65): TREE_SHAPES[33, 65]})
    whole = G.reduce_slabs

    def ragged_dropped(v):
        v = np.asarray(v, np.float64)
        return whole(v[:, :v.shape[1] // 256 * 256] if v.shape[1] > 256 else v)

    with monkeypatch.context() as m:
        m.setattr(G, "reduce_slabs", ragged_dropped)
        with pytest.raises(AssertionError):
            _check_tree({(8224, 3): TREE_SHAPES[8224, 3]})
    terms = G._terms

    def uz_zero(fixed, fmask, moving, mmask, a, z0, nzc):
        shifted = np.array(a, np.float64)
        shifted[:, 3] = shifted[:, 3] + shifted[:, 2] * z0
        return terms(fixed[z0:z0 + nzc], fmask[z0:z0 + nzc], moving, mmask, shifted, 0, nzc)

    with monkeypatch.context() as m:
        m.setattr(G, "_terms", uz_zero)
        with pytest.raises(AssertionError):
            _check_statement_against_reference()
    _check_tree({(33, 65): TREE_SHAPES[33, 65]})  # (the patches are gone)


def _metric_of(model, stack, mask, volume, k, p):
    s = V.slice_sums([stack], volume, model.affine(k, p)[None], [0], [k], stack_masks=[mask])[0]
    return G.metric(s), s[0]


def test_parameter_gradient_equals_central_differences_of_the_statements_metric():
    """dC/dp of slices of stack 'b' of ``svr_cases.problem()`` (oblique grids, a non-identity stack transform folded into
    the moving geometry) against central differences with h = 1e-5 of the statement's own metric; N stays constant.
    Measured: the largest |analytic - numeric| / max |numeric| over the slices and parameters is 5.5e-9; the bar is ten
    times that."""
    c = W.problem()
    o, h, worst = "b", 1e-5, 0.0
    model, stack, mask = c.models[o], c.stacks[o], c.masks[o]
    assert not np.allclose(model.inv_t, np.eye(4))
    for k in range(stack.shape[0]):
        p = c.true[o][k] + np.array([0.02, -0.015, 0.01, 0.5, -0.4, 0.3])
        (_, dc), n = _metric_of(model, stack, mask, c.volume, k, p)
        assert n == np.count_nonzero(mask[k])
        analytic = model.gradient(k, p, dc) * model.scales[k]
        numeric = np.zeros(6)
        for i in range(6):
            e = np.zeros(6)
            e[i] = h
            (cp, _), n_p = _metric_of(model, stack, mask, c.volume, k, p + e)
            (cm, _), n_m = _metric_of(model, stack, mask, c.volume, k, p - e)
            assert n_p == n_m == n
            numeric[i] = (cp - cm) / (2 * h)
        worst = max(worst, float(np.max(np.abs(analytic - numeric)) / np.max(np.abs(numeric))))
    print(f"largest relative gradient error {worst:.3g}")
    assert worst <= 5.5e-8


def test_slices_at_their_true_poses_stay_there():
    c = W.problem()
    found = V.register_slices(c.stacks, c.geoms, c.volume, c.hr, transforms=c.transforms, stack_masks=c.masks, init=c.true)
    for o in c.geoms:
        assert np.max(np.abs(found.parameters[o] - c.true[o])) <= 1e-9, (o, found.parameters[o] - c.true[o], found.status[o])
        assert np.max(np.abs(found.metric[o] + 1.0)) <= 1e-12, (o, found.metric[o])
        for k in range(c.geoms[o].shape[0]):
            assert np.allclose(found.transforms[o][k], np.linalg.inv(c.models[o].forward(k, c.true[o][k])), atol=1e-12)
    assert found.transforms["a"].shape == (5, 4, 4) and found.centres["b"].shape == (4, 3)


def test_slices_away_from_their_poses_come_back():
    c = W.problem()
    found = V.register_slices(c.stacks, c.geoms, c.volume, c.hr, transforms=c.transforms, stack_masks=c.masks)
    for o in c.geoms:
        assert all(s in ("step", "gradient", "iterations") for s in found.status[o])
        before, after = W_error(c, o, np.zeros_like(c.true[o])), W_error(c, o, found.parameters[o])
        print(o, "mean displacement error", before, "->", after, found.iterations[o].tolist())
        assert after < before


def W_error(c, o, params):
    """Mean distance [mm] between the images of the mask voxels of every slice under ``params`` and the true parameters."""
    m, og = R._index_to_point(c.geoms[o])
    out = []
    for k in range(c.geoms[o].shape[0]):
        idx = np.argwhere(c.masks[o][k])[:, ::-1].astype(np.float64)
        pts = np.concatenate([idx, np.full((len(idx), 1), float(k))], axis=1) @ m.T + og
        a, b = c.models[o].forward(k, params[k]), c.models[o].forward(k, c.true[o][k])
        d = pts @ (a[:3, :3] - b[:3, :3]).T + (a[:3, 3] - b[:3, 3])
        out.append(np.mean(np.sqrt(np.sum(d * d, axis=1))))
    return float(np.mean(out))


def test_records_are_independent_and_inactive_or_out_of_range_ones_give_zeros():
    b = W.mixed_batch()
    sums = _sums(b)
    order = np.random.default_rng(3).permutation(len(b.A))
    again = V.slice_sums(b.stacks, b.volume, b.A[order], b.stack[order], b.slice[order], stack_masks=b.masks, volume_mask=b.volume_mask)
    assert _same(again, sums[order])
    few = [7, 1, 7, 10]  # other slices removed, one given twice
    part = V.slice_sums(b.stacks, b.volume, b.A[few], b.stack[few], b.slice[few], stack_masks=b.masks, volume_mask=b.volume_mask)
    assert _same(part, sums[few])
    active = np.ones(len(b.A), np.uint8)
    active[[0, 6]] = 0
    stack, slice_ = b.stack.copy(), b.slice.copy()
    stack[1], stack[7], slice_[8], slice_[9] = 3, -1, 4, -1
    got = V.slice_sums(b.stacks, b.volume, b.A, stack, slice_, active=active, stack_masks=b.masks, volume_mask=b.volume_mask)
    zero = [0, 6, 1, 7, 8, 9]
    assert _same(got[zero], np.zeros((6, 43))) and not np.any(np.signbit(got[zero]))
    keep = [r for r in range(len(b.A)) if r not in zero]
    assert _same(got[keep], sums[keep])
    bad = b.A.copy()
    bad[5, 1, 2] = np.nan
    bad[10, 0, 0] = np.inf
    got = V.slice_sums(b.stacks, b.volume, bad, b.stack, b.slice, stack_masks=b.masks, volume_mask=b.volume_mask)
    assert not np.any(got[[5, 10]]) and _same(got[[6, 11]], sums[[6, 11]])


def status_case():
    """``(c, stack, mask, vmask, n3)`` on stack 'a' of ``svr_cases.problem()``: slice 0 with an empty mask, slice 1 constant;
    ``vmask`` is a volume mask set only at the nearest nodes of the ``n3`` mask voxels of slice 3 at ``p = 0``, so that with
    ``min_count = n3`` the first evaluation of slice 3 counts and any move that takes a voxel to another node does not."""
    c = W.problem()
    stack, mask = c.stacks["a"].copy(), c.masks["a"].copy()
    mask[0] = 0
    stack[1] = 123.0
    coords = R._coords(c.models["a"].affine(3, np.zeros(6)), (1,) + mask.shape[1:], (0, 0, 3))
    q = np.stack([np.floor(ck[0][mask[3] != 0] + 0.5).astype(int) for ck in coords], axis=1)
    vmask = np.zeros(c.volume.shape, np.uint8)
    vmask[q[:, 2], q[:, 1], q[:, 0]] = 1
    return c, stack, mask, vmask, int(np.count_nonzero(mask[3]))


def check_status(register, plain):
    """``register`` / ``plain``: register_slices of either path / the result on the untouched stack 'a'."""
    c, stack, mask, vmask, n3 = status_case()
    found = register({"a": stack}, {"a": c.geoms["a"]}, c.volume, c.hr, stack_masks={"a": mask})
    assert found.status["a"][:2] == ["rejected", "rejected"] and not np.any(found.parameters["a"][:2])
    assert found.iterations["a"][:2].tolist() == [0, 0] and np.all(np.isnan(found.metric["a"][:2]))
    assert np.array_equal(found.transforms["a"][:2], np.repeat(np.eye(4)[None], 2, axis=0))
    for k in (2, 3, 4):  # the other slices of the call are unaffected, bit for bit
        assert _same(found.parameters["a"][k], plain.parameters["a"][k]) and found.status["a"][k] == plain.status["a"][k]
        assert found.status["a"][k] in ("gradient", "step", "iterations")
    lost = register({"a": stack}, {"a": c.geoms["a"]}, c.volume, c.hr, stack_masks={"a": mask}, volume_mask=vmask, min_count=n3)
    assert lost.status["a"][3] == "lost" and lost.iterations["a"][3] >= 1, (lost.status, lost.iterations)
    assert not np.any(lost.parameters["a"][3]) and np.isfinite(lost.metric["a"][3]) and np.all(np.isfinite(lost.transforms["a"]))
    assert lost.status["a"][:3] == ["rejected"] * 3 and lost.status["a"][4] == "rejected"  # (fewer than n3 voxels count there)
    return found, lost


def test_status_of_slices_that_cannot_be_registered():
    c = W.problem()
    plain = V.register_slices({"a": c.stacks["a"]}, {"a": c.geoms["a"]}, c.volume, c.hr, stack_masks={"a": c.masks["a"]})
    _, stack, mask, vmask, n3 = status_case()
    first = V.slice_sums([stack], c.volume, c.models["a"].affine(3, np.zeros(6))[None], [0], [3], stack_masks=[mask], volume_mask=vmask)
    assert first[0, 0] == n3
    check_status(V.register_slices, plain)


@pytest.fixture(scope="module")
def lib():
    from fetal_t2mapping_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        from fetal_t2mapping_amd import build

        build.build()
    return _lib.load()


def _err(lib):
    return lib.t2fit_last_error().decode()


def test_library_packs_the_table_and_refuses_bad_arguments_without_a_device(lib):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "t2fit.h")).read()
    names = [n for n, _, _ in _abi.SYMBOLS]
    older = (_abi.ADDITIVE + _abi.REGISTER_SYMBOLS + _abi.ATLAS_SYMBOLS + _abi.N4_SYMBOLS + _abi.MI_SYMBOLS + _abi.SR_SYMBOLS
             + _abi.SR_SLICE_SYMBOLS)
    assert len(_abi.SVR_SYMBOLS) == 4
    for name in _abi.SVR_SYMBOLS:
        assert hasattr(lib, name) and name in names and name + "(" in header and name in _abi.LOOKED_UP and name not in older
    assert lib.t2fit_abi_version() == 5 and "#define T2FIT_SVR_RECORD_BYTES 128" in header and _abi.SVR_RECORD_BYTES == V.RECORD_BYTES == 128
    D = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    I = lambda a: (C.c_int32 * np.size(a))(*[int(v) for v in np.ravel(a)])
    U = lambda a: (C.c_uint8 * np.size(a))(*[int(v) for v in np.ravel(a)])
    b = W.mixed_batch()
    n, shapes = len(b.A), [g.shape for g in b.geoms]
    lo = I(shapes)
    need = C.c_size_t(0)
    assert lib.t2fit_svr_table_bytes(n, C.byref(need)) == 0 and need.value == 128 * n
    assert lib.t2fit_svr_table_bytes(0, C.byref(need)) == _abi.E_INVALID and ">= 1" in _err(lib)
    assert lib.t2fit_svr_table_bytes(n, None) == _abi.E_INVALID and "NULL" in _err(lib)
    # the layout, byte for byte: A, stack, slice, active (0 / 1), five zero words; nothing beyond the table is written
    active = (np.arange(n) % 3 != 1).astype(np.uint8) * 7
    raw = np.full(128 * n + 16, 0xAB, np.uint8)
    assert lib.t2fit_svr_table_host(n, D(b.A), I(b.stack), I(b.slice), U(active), 3, lo, raw.ctypes.data_as(C.c_void_p), 128 * n) == 0, _err(lib)
    assert np.all(raw[128 * n:] == 0xAB)
    assert np.array_equal(raw[:128 * n], V.pack_table(b.A, b.stack, b.slice, active, shapes))
    for r in (0, 5, n - 1):
        rec = raw[128 * r:128 * (r + 1)]
        assert np.array_equal(rec[:96].view(np.float64).reshape(3, 4), b.A[r])
        assert tuple(rec[96:128].view(np.int32)) == (b.stack[r], b.slice[r], int(active[r] != 0), 0, 0, 0, 0, 0)
    # refusals; a bad record leaves the table untouched
    raw = np.full(128 * n, 0xAB, np.uint8)
    nan, bad_stack, bad_slice = b.A.copy(), b.stack.copy(), b.slice.copy()
    nan[4, 2, 1] = np.nan
    bad_stack[6], bad_slice[9] = 3, 4

    def pack(n=n, A=b.A, stack=b.stack, slice_=b.slice, active=active, n_stacks=3, lo=lo, table=raw.ctypes.data_as(C.c_void_p), nbytes=128 * n):
        return lib.t2fit_svr_table_host(n, None if A is None else D(A), None if stack is None else I(stack),
                                        None if slice_ is None else I(slice_), None if active is None else U(active), n_stacks, lo, table,
                                        nbytes)

    for kw, text in (({"A": None}, "NULL"), ({"stack": None}, "NULL"), ({"slice_": None}, "NULL"), ({"active": None}, "NULL"),
                     ({"lo": None}, "NULL"), ({"table": None}, "NULL"), ({"n": 0}, "n_slices"), ({"n_stacks": 0}, "n_stacks"),
                     ({"n_stacks": 7}, "n_stacks"), ({"lo": I([(5, 19, 21), (3, 0, 19), (4, 33, 70)])}, ">= 1"),
                     ({"nbytes": 128 * n - 1}, "smaller"), ({"A": nan}, "record 4: A has a non-finite"),
                     ({"stack": bad_stack}, "record 6: the stack index"), ({"slice_": bad_slice}, "record 9: the slice index"),
                     ({"slice_": -b.slice - 1}, "record 0: the slice index")):
        assert pack(**kw) == _abi.E_INVALID, kw
        assert text in _err(lib), (kw, _err(lib))
        assert np.all(raw == 0xAB), kw
    # the workspace arithmetic
    for shp, k in (([(3, 1, 1)], 1), ([(2, 33, 65), (9, 32, 64)], 11), ([(1, 8224, 3)], 1), (shapes, n), ([(57, 256, 256)] * 3, 171)):
        assert lib.t2fit_svr_workspace_bytes(len(shp), I(shp), k, C.byref(need)) == 0, _err(lib)
        assert need.value == V.workspace_bytes(shp, k), (shp, k)
    assert V.workspace_bytes([(57, 256, 256)] * 3, 171) == 43 * 8 * 171 * 32  # 32 slabs a slice, one pass
    for args, text in (((3, None, n, C.byref(need)), "NULL"), ((3, lo, n, None), "NULL"), ((0, lo, n, C.byref(need)), "n_stacks"),
                       ((3, lo, 0, C.byref(need)), "n_slices"), ((1, I([(1, 2 ** 20, 2 ** 21)]), 1, C.byref(need)), "2^40"),
                       ((1, I([(1, 2 ** 19, 2 ** 20)]), 2 ** 20, C.byref(need)), "workgroups")):
        assert lib.t2fit_svr_workspace_bytes(*args) == _abi.E_INVALID, args
        assert text in _err(lib), (args, _err(lib))
    # the sums: the pointers are never dereferenced, every call is refused first
    P = lambda *v: (C.c_void_p * len(v))(*v)
    ws = V.workspace_bytes(shapes, n)

    def sums(n_stacks=3, fixed=P(0x1000, 0x2000, 0x3000), masks=P(0x4000, None, 0x5001), lo=lo, moving=0x6000, mmask=0x7001, m=(25, 23, 27),
             table=0x8000, n=n, out=0x9000, wsp=0x10000, nbytes=ws):
        return lib.t2fit_svr_sums_dev(n_stacks, fixed, masks, lo, moving, mmask, *m, table, n, out, wsp, nbytes, None)

    for kw, text in (({"fixed": None}, "NULL"), ({"lo": None}, "NULL"), ({"moving": None}, "NULL"), ({"table": None}, "NULL"),
                     ({"out": None}, "NULL"), ({"wsp": None}, "NULL"), ({"fixed": P(0x1000, None, 0x3000)}, "a stack pointer is NULL"),
                     ({"n_stacks": 0}, "n_stacks"), ({"n_stacks": 7}, "n_stacks"), ({"n": 0}, "n_slices"), ({"m": (25, 0, 27)}, ">= 1"),
                     ({"m": (2 ** 14, 2 ** 14, 2 ** 14)}, "2^40"), ({"lo": I([(5, 19, 21), (3, 40, -19), (4, 33, 70)])}, ">= 1"),
                     ({"fixed": P(0x1000, 0x2002, 0x3000)}, "aligned to 4"), ({"moving": 0x6001}, "aligned to 4"),
                     ({"out": 0x9004}, "aligned to 8"), ({"table": 0x8004}, "aligned to 8"), ({"wsp": 0x10080}, "aligned to 256"),
                     ({"nbytes": ws - 1}, "too small")):
        assert sums(**kw) == _abi.E_INVALID, kw
        assert text in _err(lib), (kw, _err(lib))


def test_python_refusals():
    b = W.mixed_batch()
    shapes = [g.shape for g in b.geoms]
    nan = b.A.copy()
    nan[3, 0, 0] = np.inf
    for kw in ({"A": nan}, {"stack": np.where(b.stack == 2, 3, b.stack)}, {"slice_": b.slice + 3}, {"slice_": b.slice[:-1]}, {"A": b.A[0, 0]}):
        args = {"A": b.A, "stack": b.stack, "slice_": b.slice, "active": None, "lo_shapes": shapes, **kw}
        with pytest.raises(ValueError):
            V.pack_table(**args)
    with pytest.raises(ValueError, match="between 1 and 6"):
        V.slice_sums([b.stacks[0]] * 7, b.volume, b.A, b.stack, b.slice)
    with pytest.raises(ValueError, match="shape of its"):
        V.slice_sums(b.stacks, b.volume, b.A, b.stack, b.slice, stack_masks=[b.masks[1], None, None])
    c = W.problem()
    for kw in ({"init": {"a": np.zeros((4, 6))}}, {"init": {"zz": np.zeros((5, 6))}}, {"init": {"a": np.full((5, 6), np.nan)}},
               {"transforms": {"zz": np.eye(4)}}, {"transforms": {"a": np.eye(3)}}, {"step": 0.0}, {"min_count": 0}, {"max_iter": -1}):
        with pytest.raises(ValueError):
            V.register_slices(c.stacks, c.geoms, c.volume, c.hr, stack_masks=c.masks, **kw)
    stacks, geoms = L.moved_phantom()[:2]
    for kw in ({"rounds": 0}, {"slice_transforms": {}}, {"return_info": True}):
        with pytest.raises(ValueError):
            V.reconstruct_svr(stacks, geoms, **kw)


SVR_RATIO = 0.9145  # measured with the statement: see the docstring below


def check_recovery(one, two, hi, found_one, found_two, merge, plain, ratio_bar):
    """The inequalities of the recovery test on volumes ``(1, 48, 48, 48)`` and the poses found after one and two rounds."""
    stacks, geoms, truth, grid, _ = L.moved_phantom()
    for found in (found_one, found_two):
        if found is not None:
            assert all(s in ("gradient", "step", "iterations") for o in geoms for s in found.status[o]), found.status
    before, e1 = W.displacement_error(None), W.displacement_error(found_one.transforms)
    print("mean slice displacement error [mm]: before", before, "round 1", e1)
    for o in geoms:
        assert e1[o] < before[o], (o, before, e1)
    rmse = {k: K.interior_rmse(np.asarray(v).reshape(1, 48, 48, 48), truth, grid, hi.GetOrigin())
            for k, v in (("one", one), ("two", two), ("merge", merge), ("plain", plain)) if v is not None}
    print("interior RMSE", rmse)
    last = "two" if two is not None else "one"
    assert rmse[last] < rmse["merge"] and rmse[last] < rmse["plain"]
    if found_two is not None:
        e2 = W.displacement_error(found_two.transforms)
        print("round 2", e2, "ratio", rmse["two"] / rmse["merge"])
        for o in geoms:
            assert e2[o] < before[o], (o, before, e2)
        assert rmse["two"] / rmse["merge"] <= ratio_bar
    return rmse


def test_the_slice_poses_of_the_moved_phantom_are_recovered():
    """``sr_slice_cases.moved_phantom()`` (48^3, three stacks of 12 slices of 4 mm, +-4 degrees / +-2 mm a slice, Rician sigma
    15), masks ``stack > 60``, 4 iterations of 10 prox iterations per reconstruction.  Measured with this statement: mean
    slice displacement error ax / cor / sag 2.42 / 2.09 / 2.08 mm before, 1.50 / 1.48 / 1.47 after round 1, 1.32 / 1.29 / 1.27
    after round 2; interior RMSE merge 246.19, reconstruct_sr without poses 244.17, found poses 226.28 after round 1 and
    225.13 after round 2: ratio to the merge 0.9145 (the reconstructions are short: with 10 iterations the same loop gives
    209.9 and 199.6, ratio 0.81).  The bound is that ratio + 0.05, the allowance of the test with the true poses
    (tests/test_sr_slice_host.py)."""
    stacks, geoms = L.moved_phantom()[:2]
    one, hi, found_one = W.phantom_statement(1)
    two, hi2, found_two = W.phantom_statement(2)
    assert hi.GetOrigin() == hi2.GetOrigin() and two.shape == (1, 48, 48, 48) and two.dtype == np.float32
    merge = R.reconstruct(stacks, geoms)[0]
    plain = S.reconstruct_sr(stacks, geoms, n_iter=W.SVR_N_ITER, prox_iter=W.SVR_PROX_ITER)[0]
    check_recovery(one, two, hi, found_one, found_two, merge, plain, SVR_RATIO + 0.05)


def test_command_line_flags_parse_and_are_refused(tmp_path):
    from fetal_t2mapping_amd import cli, recon

    base = ["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo", "--lf"]
    plain = {"weight": S.DEFAULT_WEIGHT, "n_iter": S.DEFAULT_N_ITER, "profile": "box", "thickness": None}
    assert recon.parse_arguments(base + ["--recon_method", "sr"]).sr_args == plain  # off by default: nothing changes
    assert recon.parse_arguments(base).sr_args is None
    args = recon.parse_arguments(base + ["--recon_method", "sr", "--sr_estimate_slices", "2", "--sr_write_slice_transforms", "poses"])
    assert args.sr_args == dict(plain, estimate_slices=2, write_slice_transforms_dir="poses")
    assert recon.parse_arguments(base + ["--recon_method", "sr", "--sr_estimate_slices=1"]).sr_args == dict(plain, estimate_slices=1)
    for bad in (["--sr_estimate_slices", "2"], ["--recon_method", "average", "--sr_estimate_slices", "2"],
                ["--sr_write_slice_transforms", "poses"], ["--recon_method", "sr", "--sr_write_slice_transforms", "poses"],
                ["--recon_method", "sr", "--sr_estimate_slices", "0"],
                ["--recon_method", "sr", "--sr_estimate_slices", "2", "--sr_slice_transforms", "poses"]):
        with pytest.raises(SystemExit):
            recon.parse_arguments(base + bad)
    fit = base + ["--gaussian", "--sim", "s"]
    args = cli.parse_arguments(fit + ["--reconstruct", "--recon_method", "sr", "--recon_sr_estimate_slices", "3",
                                      "--recon_sr_write_slice_transforms", "poses"])
    assert args.reconstruct_args["sr"]["estimate_slices"] == 3 and args.reconstruct_args["sr"]["write_slice_transforms_dir"] == "poses"
    for bad in (["--reconstruct", "--recon_sr_estimate_slices", "2"], ["--recon_sr_estimate_slices", "2"],
                ["--reconstruct", "--recon_method", "sr", "--recon_sr_estimate_slices", "2", "--recon_sr_slice_transforms", "poses"]):
        with pytest.raises(SystemExit):
            cli.parse_arguments(fit + bad)


def test_found_poses_are_written_where_the_slice_transforms_flag_reads_them(tmp_path):
    from fetal_t2mapping_amd import recon

    c = W.problem()
    found = V.register_slices(c.stacks, c.geoms, c.volume, c.hr, transforms=c.transforms, stack_masks=c.masks, max_iter=2)
    acq = {"sub": "sub-001", "ses": "ses-01", "EchoTime": 0.114}
    names = {"a": "ax", "b": "cor"}  # the files are named after the three orientations
    recon.save_slice_transforms(str(tmp_path), acq, {names[o]: t for o, t in found.transforms.items()})
    back = recon.load_slice_transforms(str(tmp_path), acq, {names[o]: g for o, g in c.geoms.items()})
    for o in c.geoms:
        assert _same(back[names[o]], found.transforms[o])
