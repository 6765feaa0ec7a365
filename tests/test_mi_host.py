"""Mattes mutual information, host side: the numpy statement (fetal_t2mapping_amd/_register.py: joint_histogram,
mattes_metric, mi_gradient_sums) against a plain per-voxel loop written from the words of include/t2fit.h, against the
counts of the correlation ratio's sums, the window at its clamps, the gradient sums against an exact reference, the metric
against its formula, the gradient against differences, recovery of a known transform across contrasts against the other
two costs, the options, the ABI without a device, and recon.py's flags.  tests/test_mi_gpu.py holds the device to the
statement."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest

import atlas_cases as AC
import mi_cases as MC
import register_cases as K
from fetal_t2mapping_amd import _abi
from fetal_t2mapping_amd import _register as G
from fetal_t2mapping_amd import _resample as R


# ---- 1. the definition as a loop -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _counted(name):
    """``[(ix, iy, iz, m, (gx, gy, gz))]`` of the voxels that count, in Python floats (IEEE doubles, one rounding per
    operation) from the header's words: the coordinate, the inside test, the nearest mask node, the interpolant with its
    zero-weight rule and the node gradient with its flat rule."""
    _, moving, a, fmask, mmask = MC.inputs(name, 64)
    a = np.asarray(a, np.float64).reshape(3, 4).tolist()
    v, fm, mm = moving.tolist(), np.asarray(fmask).tolist(), np.asarray(mmask).tolist()
    fz, fy, fx = fmask.shape
    n = moving.shape[::-1]
    floor = math.floor

    def lerp(p, q, w):
        return p if w == 0.0 else p + w * (q - p)

    out = []
    for iz in range(fz):
        for iy in range(fy):
            for ix in range(fx):
                if not fm[iz][iy][ix]:
                    continue
                c = [((r[0] * ix + r[1] * iy) + r[2] * iz) + r[3] for r in a]
                if not (-0.5 <= c[0] < n[0] - 0.5 and -0.5 <= c[1] < n[1] - 0.5 and -0.5 <= c[2] < n[2] - 0.5):
                    continue
                near = [min(max(floor(c[k] + 0.5), 0), n[k] - 1) for k in range(3)]
                if not mm[near[2]][near[1]][near[0]]:
                    continue
                lo = [min(max(floor(c[k]), 0), n[k] - 1) for k in range(3)]
                d = [max(c[k] - lo[k], 0.0) for k in range(3)]
                hi = [min(lo[k] + 1, n[k] - 1) for k in range(3)]
                t = [[[v[z][y][x] for x in (lo[0], hi[0])] for y in (lo[1], hi[1])] for z in (lo[2], hi[2])]
                row = [[lerp(t[z][y][0], t[z][y][1], d[0]) for y in (0, 1)] for z in (0, 1)]
                plane = [lerp(row[z][0], row[z][1], d[1]) for z in (0, 1)]
                m = lerp(plane[0], plane[1], d[2])
                gx = lerp(lerp(t[0][0][1] - t[0][0][0], t[0][1][1] - t[0][1][0], d[1]),
                          lerp(t[1][0][1] - t[1][0][0], t[1][1][1] - t[1][1][0], d[1]), d[2])
                gy = lerp(row[0][1] - row[0][0], row[1][1] - row[1][0], d[2])
                gz = plane[1] - plane[0]
                g = [0.0 if (hi[k] == lo[k] or c[k] < 0.0) else gk for k, gk in enumerate((gx, gy, gz))]
                out.append((ix, iy, iz, m, g))
    return out


def _window(m, lo_m, scale_m, n_m):
    """``(i0, w [4], w' [4])`` of one sample, in the header's order of operations."""
    t = (m - lo_m) * scale_m + 2.0
    t = t if t >= 2.0 else 2.0
    t = t if t <= n_m - 2 else float(n_m - 2)
    i0 = min(math.floor(t), n_m - 3)
    u = t - i0
    v = 1.0 - u
    u2, v2 = u * u, v * v
    u3, v3 = u2 * u, v2 * v
    w = [v3 / 6.0, ((3.0 * u3 - 6.0 * u2) + 4.0) / 6.0, (((-3.0 * u3 + 3.0 * u2) + 3.0 * u) + 1.0) / 6.0, u3 / 6.0]
    dw = [-(v2 * 0.5), 1.5 * u2 - 2.0 * u, (-1.5 * u2 + u) + 0.5, u2 * 0.5]
    return i0, w, dw


def _loop_hist(name, n_f, n_m):
    bins = MC.inputs(name, n_f)[0]
    lo_m, scale_m = MC.moving_range(name, n_m)
    h = [[0] * n_m for _ in range(n_f)]
    for ix, iy, iz, m, _ in _counted(name):
        b = min(int(bins[iz, iy, ix]), n_f - 1)
        i0, w, _ = _window(m, lo_m, scale_m, n_m)
        assert 2 <= i0 <= n_m - 3
        for j in range(4):
            h[b][i0 - 1 + j] += math.floor(w[j] * 1073741824.0 + 0.5)
    return h


@pytest.mark.parametrize("name", MC.HOST_CASES)
def test_joint_histogram_equals_the_per_voxel_loop(name):
    for n_f, n_m in MC.BIN_PAIRS:
        got = MC.statement_hist(name, n_f, n_m)
        assert got.dtype == np.uint64 and got.shape == (n_f, n_m)
        want = _loop_hist(name, n_f, n_m)
        assert got.tolist() == want, (name, n_f, n_m)
        if name == "nothing":
            assert not got.any()
        else:
            assert got.any() and not got[:, 0].any()  # bin 0 is padding no window reaches
    assert (len(_counted(name)) == 0) == (name == "nothing") and len(_counted(name)) == K.statement_sums(name)[0]
    if name == "capped2_thin":  # the thinned mask keeps voxels that count in the bricks past the kernel's 2048 workgroups
        brick = MC.brick_index(MC.inputs(name, 64)[0].shape)
        late = sum(1 for ix, iy, iz, _, _ in _counted(name) if brick[iz, iy, ix] >= MC.HIST_GRID)
        assert late > 100 and late == K.counted_per_slab(name)[MC.HIST_GRID:].sum()


@pytest.mark.parametrize("name", MC.CAPPED)
def test_capped_cases_have_more_bricks_than_workgroups_and_their_late_bricks_count(name):
    """The conditions tests/test_mi_gpu.py relies on, with the statement alone (mi_cases.check_capped)."""
    assert MC.check_capped(name) == {"capped2": 9 * 258, "capped5": 33 * 258}[name]
    n = MC.counted(name)
    for n_f, n_m in ((32, 32), (1, 5)):  # the total the device test asserts: four roundings of half a unit per voxel
        assert abs(sum(int(v) for v in MC.statement_hist(name, n_f, n_m).ravel().tolist()) - n * MC.ONE) <= 2 * n


# ---- 2. the tie to the correlation ratio's counts --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["prime", "bricks", "half_rim", "integer"])
def test_rows_add_up_to_the_counts_of_binned_sums(name):
    """A voxel's four weights add up to 1 before they are rounded to units of 2^-30: four roundings of at most half a unit
    each, so a row differs from N_b 2^30 by at most 2 N_b."""
    for n_f, n_m in MC.BIN_PAIRS:
        bins, moving, a, fmask, mmask = MC.inputs(name, n_f)
        n_b = (AC.statement(name, n_f)[0] if n_f in AC.N_BINS else G.binned_sums(bins, moving, a, n_f, fmask, mmask))[:n_f]
        rows = [sum(r) for r in MC.statement_hist(name, n_f, n_m).tolist()]
        worst = max(abs(r - int(c) * MC.ONE) - 2 * int(c) for r, c in zip(rows, n_b))
        print(f"{name} {n_f} x {n_m}: N {n_b.sum():.0f}, largest |row - N_b 2^30| - 2 N_b = {worst}")
        assert worst <= 0 and n_b.sum() == K.statement_sums(name)[0]


# ---- 3. the clamps -----------------------------------------------------------------------------------------------------------
def test_window_at_the_ends_of_the_range_and_beyond():
    sixth, two_thirds = round(MC.ONE / 6), round(MC.ONE * 2 / 3)
    n_m = 9
    moving = np.array([[[100.0, 356.0, 228.0, 500.0, -40.0]]], np.float32)  # lo_m, hi_m, the middle, beyond either end
    mask = np.array([[[1, 1, 1, 0, 0]]], np.uint8)
    lo_m, scale_m = G.moving_bin_range(moving, mask, n_m)
    assert (lo_m, scale_m) == (100.0, 5.0 / 256.0)
    eye = np.eye(3, 4)

    def hist_of(x, **kw):
        only = np.zeros((1, 1, 5), np.uint8)
        only[0, 0, x] = 1
        return G.joint_histogram(np.zeros((1, 1, 5), np.uint8), moving, eye, 1, n_m, kw.get("lo", lo_m), kw.get("scale", scale_m), only,
                                 np.ones((1, 1, 5), np.uint8))[0].tolist()

    at_lo, at_hi = [0, sixth, two_thirds, sixth, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, sixth, two_thirds, sixth]
    assert hist_of(0) == at_lo           # m = lo_m: t = 2, i0 = 2, u = 0: bins 1 .. 4 get 1/6, 4/6, 1/6, 0
    assert hist_of(1) == at_hi           # m = hi_m: t = n_m - 2, i0 = n_m - 3, u = 1: bins n_m - 4 .. n_m - 1 get 0, 1/6, 4/6, 1/6
    assert hist_of(3) == at_hi and hist_of(4) == at_lo  # beyond the range: the end bins, not outside the table
    mid = hist_of(2)                     # t = 4.5: i0 = 4, u = 1/2: 1/48, 23/48, 23/48, 1/48 on bins 3 .. 6
    assert mid == [0, 0, 0, round(MC.ONE / 48), round(MC.ONE * 23 / 48), round(MC.ONE * 23 / 48), round(MC.ONE / 48), 0, 0]
    assert hist_of(1, scale=0.0) == at_lo and hist_of(2, scale=0.0) == at_lo  # hi_m == lo_m: everything at t = 2
    assert G.moving_bin_range(np.full((2, 2, 2), 7.0), np.ones((2, 2, 2)), 32) == (7.0, 0.0)
    i0, w, dw = G.parzen_window(np.array([np.nan, 100.0, 356.0, 228.0]), lo_m, scale_m, n_m)
    assert i0.tolist() == [2, 2, 6, 4] and [float(x[3]) for x in dw] == [-0.125, -0.625, 0.625, 0.125]
    assert all(abs(sum(float(x[k]) for x in w) - 1.0) < 1e-15 and abs(sum(float(x[k]) for x in dw)) < 1e-15 for k in range(4))
    with pytest.raises(ValueError, match="empty"):
        G.moving_bin_range(moving, np.zeros(moving.shape), n_m)


# ---- 4. the gradient sums against an exact reference -----------------------------------------------------------------------
# The reference: the per-voxel terms of the loop above (the definition's own roundings), added by math.fsum -- exact up to
# its one rounding -- so what is measured is the summation tree.  The statement's largest |s - ref| / sum |terms| over the
# cases and bin pairs below is 6.41e-17; the bar is 16 times that, the precedent of register_cases.TOL.  A dropped or
# doubled slab is an error of the order of 1 / (number of slabs) >= 1e-3.
GRADIENT_SUMS_RATIO = 6.41e-17
GRADIENT_SUMS_TOL = 16 * GRADIENT_SUMS_RATIO
REFERENCE_CASES = ("prime", "bricks", "empty_bricks", "outside", "fixed_1x1x1", "fixed_9x6x65", "half_rim", "integer")


def _reference_gradient(name, n_f, n_m, kind):
    bins = MC.inputs(name, n_f)[0]
    lo_m, scale_m = MC.moving_range(name, n_m)
    table = MC.table(name, n_f, n_m, kind).tolist()
    terms = [[] for _ in range(12)]
    for ix, iy, iz, m, g in _counted(name):
        i0, _, dw = _window(m, lo_m, scale_m, n_m)
        row = table[min(int(bins[iz, iy, ix]), n_f - 1)]
        c = 0.0
        for j in range(4):
            c = c + row[i0 - 1 + j] * dw[j]
        for k in range(3):
            cg = c * g[k]
            for j, u in enumerate((float(ix), float(iy), float(iz))):
                terms[4 * k + j].append(cg * u)
            terms[4 * k + 3].append(cg)
    return np.array([math.fsum(t) for t in terms]), np.array([math.fsum(abs(x) for x in t) for t in terms])


@pytest.mark.parametrize("name", REFERENCE_CASES)
def test_gradient_sums_against_the_exact_sum_of_the_same_terms(name):
    for (n_f, n_m), kind in (((32, 32), "normal"), ((7, 9), "normal"), ((32, 32), "metric")):
        got = MC.statement_gradient(name, n_f, n_m, kind)
        ref, scale = _reference_gradient(name, n_f, n_m, kind)
        assert got.shape == (12,) and np.all(np.isfinite(got)) and np.array_equal(got[scale == 0], ref[scale == 0])
        ratio = float(np.max(np.abs(got - ref)[scale > 0] / scale[scale > 0], initial=0.0))
        print(f"{name} {n_f} x {n_m} {kind}: largest |s - ref| / scale {ratio:.3g}")
        assert ratio <= GRADIENT_SUMS_TOL
        if kind == "normal" and len(_counted(name)) > 100:
            assert np.count_nonzero(got) >= 8  # (a thin volume has u_j = 0 along an axis)


def test_gradient_sums_of_no_voxel_are_zeros():
    assert MC.statement_gradient("nothing", 32, 32, "normal").tobytes() == np.zeros(12).tobytes()
    with pytest.raises(ValueError, match="no voxel to compare"):
        G.mattes_metric(MC.statement_hist("nothing", 32, 32), 32, 32, 1.0)


# ---- 5. the metric -----------------------------------------------------------------------------------------------------------
def _entropy(p):
    p = p[p > 0]
    return float(-np.sum(p * np.log(p)))


def test_metric_formula_on_a_hand_built_histogram():
    h = (np.array([[2, 1, 1, 0, 0], [0, 1, 1, 2, 0]]) * MC.ONE).astype(np.uint64)
    cost, table = G.mattes_metric(h, 2, 5, 3.0)
    # p = h / 8, p_f = (1/2, 1/2), p_m = (1/4, 1/4, 1/4, 1/4, 0): the two entries of 1/4 carry log 2 each, the four of 1/8 log 1
    assert abs(cost + 0.5 * math.log(2.0)) < 1e-15
    want = -(3.0 / 8.0) * np.log(np.array([[1.0, 0.5, 0.5, 1.0, 1.0], [1.0, 0.5, 0.5, 1.0, 1.0]]))
    assert np.allclose(table, want, rtol=0, atol=1e-15) and table[0, 3] == 0.0 and table[1, 0] == 0.0 and table[0, 4] == 0.0
    disjoint = (np.array([[3, 1, 0, 0, 0], [0, 0, 2, 1, 1]]) * MC.ONE).astype(np.uint64)  # the moving bin tells the fixed one
    assert abs(G.mattes_metric(disjoint, 2, 5, 1.0)[0] + _entropy(np.array([0.5, 0.5]))) < 1e-15
    for bad in (h.astype(np.int64), h[:, :4]):
        with pytest.raises(ValueError, match="uint64"):
            G.mattes_metric(bad, 2, 5, 1.0)


def test_identical_volumes_give_the_fixed_entropy_within_the_window_and_a_remap_beats_a_shift():
    fixed = K.recovery_pair()[0]
    mask = np.ones(fixed.shape, np.uint8)
    eye = np.eye(3, 4)
    lo, scale = G.bin_range(fixed, mask, 32)
    bins = G.bin_volume(fixed, lo, scale, 32)
    p_f = np.bincount(bins.ravel(), minlength=32) / bins.size
    # the volume against itself: a moving bin k holds samples with |t - k| < 2, 4 moving bins or 4 * 32 / 28 fixed bins wide,
    # so it meets at most 6 fixed bins: H(F | M) <= log 6 and H(F) - log 6 <= MI <= H(F)
    lo_m, scale_m = G.moving_bin_range(fixed, mask, 32)
    mi = -G.mattes_cost_and_gradient(bins, fixed, eye, 32, 32, lo_m, scale_m)[0]
    print(f"MI of the volume with itself {mi:.4f}, fixed entropy {_entropy(p_f):.4f}")
    assert _entropy(p_f) - math.log(6.0) <= mi <= _entropy(p_f) + 1e-12
    # a per-bin remap whose values lie 8 moving bins apart (8 fixed bins, 64 moving): the windows of two fixed bins never
    # share a moving bin, H(F | M) = 0 and MI is the fixed entropy -- of the histogram's marginal, whose weights are rounded
    # to units of 2^-30: a row is within 2 N_b units of N_b 2^30 (check 2), p_f within 4 * 2^-30 of the counts' in all, and
    # the entropy within sum |dp| (|log p| + 1) < 4e-9 * 8 of theirs
    bins8 = G.bin_volume(fixed, *G.bin_range(fixed, mask, 8), 8)
    remap8 = (100.0 + 32.0 * np.array([3, 6, 0, 5, 1, 7, 2, 4], np.float32))[bins8]
    lo8, scale8 = G.moving_bin_range(remap8, mask, 64)
    assert (lo8, scale8) == (100.0, 60.0 / 224.0)
    mi8 = -G.mattes_cost_and_gradient(bins8, remap8, eye, 8, 64, lo8, scale8)[0]
    p8 = np.bincount(bins8.ravel(), minlength=8) / bins8.size
    assert p8.min() > math.exp(-7.0) and abs(mi8 - _entropy(p8)) < 4e-9 * 8
    # a remap in place costs less than the same volume 3 voxels away
    remap = np.random.default_rng(3).uniform(100, 900, 32).astype(np.float32)[bins]
    lo_r, scale_r = G.moving_bin_range(remap, mask, 32)
    shifted = eye.copy()
    shifted[0, 3] = 3.0
    here, away = (G.mattes_cost_and_gradient(bins, remap, a, 32, 32, lo_r, scale_r)[0] for a in (eye, shifted))
    print(f"cost of a per-bin remap {here:.4f}, 3 voxels away {away:.4f}")
    assert here < away < 0.0


# ---- 6. the gradient against central differences -----------------------------------------------------------------------------
def _mattes_at(p, n_f=32, n_m=32):
    fixed, moving, g, box, ones = AC.gradient_case()
    centre, _ = G.affine_centre_and_scales(box, g)
    bins = G.bin_volume(fixed, *G.bin_range(fixed, box, n_f), n_f)
    lo_m, scale_m = G.moving_bin_range(moving, ones, n_m)
    a = R.index_affine(g, g, G.compose_affine(p, centre))
    hist = G.joint_histogram(bins, moving, a, n_f, n_m, lo_m, scale_m, box, ones)
    cost, table = G.mattes_metric(hist, n_f, n_m, scale_m)
    dc = G.mi_gradient_sums(bins, table, moving, a, n_m, lo_m, scale_m, box, ones).reshape(3, 4)
    n = round(sum(int(v) for v in hist.ravel().tolist()) / MC.ONE)  # (the rows are within 2 N 2^-30 of the count)
    return cost, G.affine_parameter_gradient(dc, p, centre, g, g), n


# Measured with the statement: the largest |analytic - central difference| over the 12 components, relative to the
# largest component, is 4.49e-4 at h = 1e-4 (the numpy prototype of the design gave 4.5e-4).  The bar is 4 times the
# measured figure; above 1e-2 the gradient would be wrong, not noisy.
MI_GRADIENT_RATIO = 4.49e-4
MI_GRADIENT_BOUND = 4 * MI_GRADIENT_RATIO


def test_mattes_gradient_against_central_differences():
    p0, h = AC.GRADIENT_P0, 1e-4
    cost, grad, n = _mattes_at(p0)
    fd = np.zeros(12)
    for i in range(12):
        d = np.zeros(12)
        d[i] = h
        (up, _, n_up), (down, _, n_down) = _mattes_at(p0 + d), _mattes_at(p0 - d)
        assert n_up == n_down == n == 20 * 28 * 36  # the box mask keeps the counted set fixed
        fd[i] = (up - down) / (2 * h)
    ratio = float(np.max(np.abs(grad - fd)) / np.max(np.abs(fd)))
    print(f"-MI {cost:.6f}; analytic {grad}; differences {fd}; largest difference / largest component {ratio:.3g}")
    assert ratio <= MI_GRADIENT_BOUND < 1e-2


# ---- 7. recovery -------------------------------------------------------------------------------------------------------------
# The statement gives TRE 0.1226 mm (mattes, 12 dof, from 7.34 mm; cr gives 0.9628) on the affine pair and 0.0310 mm (mattes,
# 6 dof, from 6.31 mm; cr 0.2592, the rigid correlation 0.2174) on the rigid pair; the pins are 1.25 times the mattes figures
# (libm differences in cos / exp / log between hosts), the margin of the cr test.
MATTES12_TRE, MATTES6_TRE = 0.1226, 0.0310


def test_recovery_of_an_affine_across_contrasts_beats_the_correlation_ratio():
    start = AC.tre(np.eye(4))
    found = MC.recovered(12)
    t_mattes, t_cr = AC.tre(found.transform), AC.tre(AC.recovered("cr", 12).transform)
    print(f"start {start:.4f} mm; TRE mattes/12 {t_mattes:.4f}, cr/12 {t_cr:.4f} mm; {found}")
    assert t_mattes < start / 4 and t_mattes < t_cr
    assert t_mattes <= 1.25 * MATTES12_TRE
    assert found.parameters.shape == (12,) and len(found.iterations) == 3 and found.metric < 0.0
    assert np.array_equal(found.transform, G.compose_affine(found.parameters, found.centre))


def test_recovery_of_a_rigid_transform_across_contrasts_beats_both_other_costs():
    fixed, moving, g, fmask, mmask = MC.rigid_pair()
    kw = dict(fixed_mask=fmask, moving_mask=mmask)
    found = G.register_rigid(fixed, moving, g, g, metric="mattes", **kw)
    t_mattes = MC.rigid_tre(found.transform)
    t_cr = MC.rigid_tre(G.register_affine(fixed, moving, g, g, metric="cr", dof=6, **kw).transform)
    t_corr = MC.rigid_tre(G.register_rigid(fixed, moving, g, g, metric="corr", **kw).transform)
    print(f"start {MC.rigid_tre(np.eye(4)):.4f} mm; TRE mattes/6 {t_mattes:.4f}, cr/6 {t_cr:.4f}, corr {t_corr:.4f} mm; {found}")
    assert t_mattes < t_cr and t_mattes < t_corr and t_mattes < 0.5 * min(g.GetSpacing())
    assert t_mattes <= 1.25 * MATTES6_TRE
    # the shape register_rigid returns: six parameters and the 4 x 4 they compose
    assert found.parameters.shape == (6,) and found.transform.shape == (4, 4) and len(found.iterations) == 3
    assert np.array_equal(found.transform, G.compose(found.parameters, found.centre))


# ---- 8. options and the ABI ----------------------------------------------------------------------------------------------------
def test_options():
    fixed, moving, g, fmask, mmask = AC.recovery_pair()
    kw = dict(fixed_mask=fmask, moving_mask=mmask, levels=(4,), max_iter=2)
    found = G.register_affine(fixed, moving, g, g, metric="mattes", dof=6, bins=16, moving_bins=5, **kw)
    assert found.iterations == (2,) and found.metric < 0.0 and np.all(found.parameters[6:] == 0)
    rigid = G.register_rigid(fixed, moving, g, g, metric="mattes", bins=16, moving_bins=5, init=np.zeros(6), **kw)
    assert rigid.parameters.tobytes() == found.parameters[:6].tobytes() and rigid.metric == found.metric
    for bad in (dict(metric="mi"), dict(metric="mattes", moving_bins=4), dict(metric="mattes", moving_bins=65), dict(moving_bins=4),
                dict(metric="mattes", bins=0), dict(metric="mattes", bins=65)):
        with pytest.raises(ValueError):
            G.register_affine(fixed, moving, g, g, **{**kw, **bad})
    for bad in (dict(metric="cr"), dict(metric="mi"), dict(metric="mattes", moving_bins=4), dict(metric="mattes", init=np.zeros(12))):
        with pytest.raises(ValueError):
            G.register_rigid(fixed, moving, g, g, **{**kw, **bad})
    far = R.Geometry(g.GetSize(), g.GetSpacing(), np.array(g.GetOrigin()) + (400.0, 0.0, 0.0), g.GetDirection())
    with pytest.raises(ValueError, match="no voxel to compare"):
        G.register_affine(fixed, moving, g, far, metric="mattes", **kw)
    from fetal_t2mapping_amd import _atlas

    subject, template, ag, mask, atlases, _ = AC.atlas_case()
    _, labels, got = _atlas.atlas_labels(subject, ag, template, ag, atlases, mask=mask, metric="mattes", levels=(4,), max_iter=2)
    assert got.metric < 0.0 and sorted(labels) == ["ho", "jhu"]


def test_abi_mirror_declares_the_new_symbols_as_looked_up():
    names = [s[0] for s in _abi.SYMBOLS]
    header = open(os.path.join(__import__("conftest").REPO, "include", "t2fit.h")).read()
    assert len(_abi.MI_SYMBOLS) == 3 and _abi.ABI_VERSION == 5 and "#define T2FIT_ABI_VERSION 5" in header
    for sym in _abi.MI_SYMBOLS:
        assert sym in names and sym + "(" in header and sym in _abi.LOOKED_UP and sym not in _abi.ADDITIVE
        assert sym not in _abi.ATLAS_SYMBOLS and sym not in _abi.REGISTER_SYMBOLS
    assert _abi.REGISTER_MI_SUMS == G.N_MI_SUMS == 12 and "#define T2FIT_REGISTER_MI_SUMS 12" in header


def test_workspace_arithmetic_and_refusals_without_a_device():
    from fetal_t2mapping_amd import build
    from fetal_t2mapping_amd._lib import load

    build.build()
    lib = load()
    assert lib.t2fit_abi_version() == 5 and all(hasattr(lib, n) for n in _abi.MI_SYMBOLS)
    need = C.c_size_t(0)
    for shape, slabs in (((19, 23, 37), 18), ((256, 256, 256), 8192), ((5, 1027, 7), 257)):
        assert lib.t2fit_register_mi_workspace_bytes(*shape, C.byref(need)) == 0
        assert int(np.prod(G.brick_counts(shape))) == slabs
        assert need.value == sum((12 * 8 * n + 255) // 256 * 256 for n in G.pass_sizes(slabs)), shape
    MC.check_refusals(lib, 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x10000, (8, 8, 8), (9, 8, 7), np.eye(3, 4), 7, 9,
                      None)


# ---- 9. recon.py over fake_sitk ------------------------------------------------------------------------------------------------
def test_register_metric_reaches_the_optimizer(monkeypatch, tmp_path):
    from fetal_t2mapping_amd import cli, recon

    base = ["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo", "--lf"]
    a = recon.parse_arguments(base)
    assert (a.register_metric, a.atlas_metric, a.register_to_lf) == ("corr", "cr", False)  # the defaults do not change
    assert recon.parse_arguments(base + ["--register", "--register_metric", "mattes"]).register_metric == "mattes"
    for bad in (["--register_metric", "mi"], ["--atlas_metric", "ncc"]):
        with pytest.raises(SystemExit):
            recon.parse_arguments(base + bad)
    cbase = ["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo", "--gaussian", "--lf", "--sim", "s"]
    a = cli.parse_arguments(cbase + ["--reconstruct", "--recon_register", "--recon_register_metric", "mattes"])
    assert a.reconstruct_args == {"fixed": "ax", "res": 1.0, "transforms_dir": None, "register": True, "register_metric": "mattes"}
    for bad in (["--recon_register_metric", "mattes"], ["--reconstruct", "--recon_register_metric", "mattes"]):
        with pytest.raises(SystemExit):
            cli.parse_arguments(cbase + bad)
    # register_stacks with the device's two calls replaced by their statements: the keyword arrives at optimize_affine
    fixed, moving, g, _, _ = MC.rigid_pair()
    seen = []
    optimize_affine = G.optimize_affine
    monkeypatch.setattr(G, "optimize_affine", lambda *args, **kw: (seen.append(kw["metric"]), optimize_affine(*args, **kw))[1])
    monkeypatch.setattr(recon.t2map, "resample_volume", lambda vol, geom, **kw: (vol, geom))
    monkeypatch.setattr(recon.t2map.register, "register_rigid",
                        lambda f, m, fg, mg, device=0, **kw: G.register_rigid(f, m, fg, mg, levels=(4,), max_iter=1, **kw))
    stacks, geoms = {"ax": fixed, "cor": moving, "sag": moving}, {"ax": g, "cor": g, "sag": g}
    found = recon.register_stacks(stacks, geoms, **recon._metric_args("mattes"))
    assert seen == ["mattes", "mattes"] and sorted(found) == ["cor", "sag"] and found["cor"].shape == (4, 4)
    assert recon._metric_args("corr") == {} and recon.register_stacks(stacks, geoms)["cor"].shape == (4, 4) and len(seen) == 2


def test_register_to_lf_rewrites_the_high_field_volumes_that_have_a_counterpart(monkeypatch, tmp_path):
    import fake_sitk
    import pandas as pd

    fake = fake_sitk.install()
    monkeypatch.setitem(sys.modules, "SimpleITK", fake)
    from fetal_t2mapping_amd import cli, recon

    base = ["--path", str(tmp_path), "--csv", "x.csv"]
    assert recon.parse_arguments(base + ["--in_vivo", "--hf", "--register_to_lf"]).register_to_lf is True
    assert recon.parse_arguments(base + ["--in_vivo", "--hf", "--register_to_lf", "--write_transforms", str(tmp_path)]).write_transforms
    for bad in (["--in_vivo", "--lf", "--register_to_lf"], ["--in_vitro", "--hf", "--register_to_lf"],
                ["--in_vitro", "--lf", "--register_to_lf"]):
        with pytest.raises(SystemExit):
            recon.parse_arguments(base + bad)

    fixed, moving, _, _, _ = MC.rigid_pair()
    fixed, moving = fixed[:, :, 4:], moving  # the low-field grid differs from the high-field one
    bids = str(tmp_path / "projects") + "/"

    def acq(sub, ses, te):
        return {"prj": "prj-901", "sub": sub, "ses": ses, "run": "run-01", "EchoTime": te / 1000.0, "CoilString": "HeadNeck",
                "ImageOrientationPatientSTR": "ax"}

    def put(row, arr):
        path = cli.get_img_path(bids, row, cli.recon_dirname).replace(" ", "")
        np.save(path + ".npy", arr)
        open(path, "w").close()
        return path

    low = put(acq("sub-001", "ses-01", 114), fixed)                      # the 0.55 T volume of sub-001; sub-002 has none
    rows = [acq("sub-001", "ses-02", 114), acq("sub-001", "ses-02", 228), acq("sub-002", "ses-02", 114), acq("sub-003", "ses-02", 299)]
    paths = [put(r, moving) for r in rows]
    put(acq("sub-003", "ses-01", 114), fixed)                            # has a counterpart, but the reference leaves te-299 of sub-003
    assert recon.low_field_path(paths[1]) == low and "te-228" in paths[1] and "ses-02" in paths[1]
    calls = []

    def rigid(f, m, fg, mg, *, metric, device=0):
        calls.append(metric)
        return G.register_rigid(f, m, R.as_geometry(fg, f.shape), R.as_geometry(mg, m.shape), metric=metric, levels=(4,), max_iter=2)

    def resample(vol, geom, *, like, transform, device=0):
        return R.resample(vol, R.index_affine(like, R.as_geometry(geom, vol.shape), transform), like.shape), like

    monkeypatch.setattr(recon.t2map.register, "register_rigid", rigid)
    monkeypatch.setattr(recon.t2map, "resample_volume", resample)
    out = str(tmp_path / "found")
    written = recon.process_register_to_lf(pd.DataFrame(rows), bids, write_transforms=out)
    assert calls == ["mattes", "mattes"]
    assert sorted(fake.written) == sorted(paths[:2]) and [w for w in written if w.endswith(".nii.gz")] == paths[:2]
    for path in paths[:2]:
        img = fake.written[path]
        assert img.arr.shape == fixed.shape and img.arr.dtype == np.float32 and img.GetSpacing() == (1.0, 1.0, 1.5)  # the fixed grid
        assert np.count_nonzero(img.arr) > 1000
    texts = sorted(w for w in written if w.endswith(".txt"))
    assert [os.path.basename(t) for t in texts] == ["sub-001_ses-02_te-114_ax_to_lf.txt", "sub-001_ses-02_te-228_ax_to_lf.txt"]
    assert np.loadtxt(texts[0]).shape == (4, 4)
