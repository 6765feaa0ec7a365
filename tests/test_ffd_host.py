"""The non-rigid alignment's numpy statement (fetal_t2mapping_amd/_ffd.py) and everything about the stage that needs no
device: the zero lattice against the affine path, the statement against independent per-voxel loops in Python floats, the
lattice gradient against central differences of -MI, subdivision and level change, recovery of a known lattice on top of an
affine, folding, the refusals and the ABI, and the drivers.  tests/test_ffd_gpu.py holds the device half."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import atlas_cases as AC
import ffd_cases as FC
import register_cases as K
from fetal_t2mapping_amd import _abi, _atlas, _bias
from fetal_t2mapping_amd import _ffd as F
from fetal_t2mapping_amd import _register as G
from fetal_t2mapping_amd import _resample as R


# ---- 1. a lattice of zeros is the affine path, bit for bit -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["outside", "prime"])
def test_zero_lattice_has_the_bits_of_the_affine_path(name):
    bins, moving, a, fmask, mmask, lo_m, scale_m = FC.named(name, 32, 32)
    shape = bins.shape
    want = R._coords(np.asarray(a, np.float64).reshape(3, 4), shape)
    for phi in (None, np.zeros((3, 4, 4, 4)), np.zeros((3, 11, 11, 11))):
        got = F.coords(a, phi, shape)
        for k in range(3):
            assert np.array_equal(K.bits(np.broadcast_to(got[k], shape)), K.bits(np.broadcast_to(want[k], shape)))
        h = F.joint_histogram(bins, moving, a, phi, 32, 32, lo_m, scale_m, fmask, mmask)
        assert np.array_equal(h, G.joint_histogram(bins, moving, a, 32, 32, lo_m, scale_m, fmask, mmask))
        w = F.warp(moving, a, phi, shape)
        assert w.dtype == np.float32 and np.array_equal(w.view(np.uint32), R.resample(moving, a, shape).view(np.uint32))
        lab = (moving > 400).astype(np.int32) * 7
        assert np.array_equal(F.warp(lab, a, phi, shape, interp="nearest", default=-3), R.resample(lab, a, shape, interp="nearest", default=-3))
    if name == "outside":  # part of the volume falls outside: the default is there, and not everywhere
        outside = R.resample(np.ones_like(moving), a, shape, default=-1.0) == -1.0
        assert 0 < np.count_nonzero(outside) < outside.size
    assert F.min_jacobian(np.zeros((3, 7, 7, 7)), fmask) == (1.0, 0)


# ---- 2. the statement against independent per-voxel loops -------------------------------------------------------------------
TINY_F, TINY_M, TINY_SIDE = (4, 5, 6), (6, 7, 8), 4


def _tiny():
    _, moving, a, fmask, mmask = K._centred_case(77, TINY_F, TINY_M, angles=(2.0, -1.5, 1.0), shift=(0.2, -0.1, 0.3), fdensity=0.9, mdensity=0.95)
    bins = np.random.default_rng(78).integers(0, 7, TINY_F).astype(np.uint8)
    return bins, moving, np.asarray(a, np.float64).reshape(3, 4), fmask, mmask, FC.lattice(TINY_SIDE, 3, 0.7)


def _basis(tau):
    """The uniform cubic B-spline basis and its derivative from the textbook polynomials, in Python floats."""
    b = [(1 - tau) ** 3 / 6, (3 * tau ** 3 - 6 * tau ** 2 + 4) / 6, (-3 * tau ** 3 + 3 * tau ** 2 + 3 * tau + 1) / 6, tau ** 3 / 6]
    d = [-(1 - tau) ** 2 / 2, (9 * tau ** 2 - 12 * tau) / 6, (-9 * tau ** 2 + 6 * tau + 3) / 6, tau ** 2 / 2]
    return b, d


def _node(i, n, c, offset=0.0):
    """First node and tau of voxel ``i`` (+ ``offset`` voxels along the same polynomial piece)."""
    s = c - 3
    if n == 1:
        return 0, 0.0
    k, tau = (s - 1, 1.0) if i == n - 1 else (int(math.floor(i * s / (n - 1))), i * s / (n - 1) - math.floor(i * s / (n - 1)))
    return k, tau + offset * s / (n - 1)


def _loop_d(phi, shape, x, y, z, off=(0.0, 0.0, 0.0)):
    """d(x) by the 64-tap triple sum, exactly summed (math.fsum): no order to share with the statement."""
    c = phi.shape[1]
    (kz, tz), (ky, ty), (kx, tx) = _node(z, shape[0], c, off[2]), _node(y, shape[1], c, off[1]), _node(x, shape[2], c, off[0])
    bz, by, bx = _basis(tz)[0], _basis(ty)[0], _basis(tx)[0]
    return [math.fsum(bz[i] * by[j] * bx[l] * float(phi[k, kz + i, ky + j, kx + l]) for i in range(4) for j in range(4) for l in range(4))
            for k in range(3)]


FIELD_BOUND = 8 * 2.0 ** -52  # three nested four-term sums of products, each rounding once: a few ulp of the amplitude


def test_field_evaluation_against_the_triple_sum():
    _, _, _, _, _, phi = _tiny()
    for shape in (TINY_F, (1, 1, 1), (2, 1, 9)):
        d = F.displacement(phi, shape)
        worst = max(abs(float(d[k][z, y, x]) - _loop_d(phi, shape, x, y, z)[k])
                    for z in range(shape[0]) for y in range(shape[1]) for x in range(shape[2]) for k in range(3))
        print(f"{shape}: largest |statement - exact triple sum| {worst:.3g} (amplitude {np.abs(phi).max():.3g})")
        assert worst <= FIELD_BOUND * np.abs(phi).max()
    # the per-axis nodes and weights are N4's
    for n, c in ((1, 4), (9, 5), (48, 7), (64, 19)):
        k, b, db = F.axis_tables(n, c)
        k0, b0, _, _ = _bias.axis_weights(n, c)
        assert np.array_equal(k, k0) and np.array_equal(b, b0) and db.shape == (n, 4) and k.max() + 3 <= c - 1
        assert np.all(np.abs(db.sum(axis=1)) < 1e-15)  # the basis sums to one


def _loop_sample(moving, mmask, c):
    """The counting rule, the interpolant and its gradient of include/t2fit.h, scalar by scalar: None when not counted."""
    n = moving.shape[::-1]
    if not all(-0.5 <= c[k] < n[k] - 0.5 for k in range(3)):
        return None
    near = [int(min(max(math.floor(c[k] + 0.5), 0), n[k] - 1)) for k in range(3)]
    if mmask[near[2], near[1], near[0]] == 0:
        return None
    lo = [int(min(max(math.floor(c[k]), 0), n[k] - 1)) for k in range(3)]
    d = [max(c[k] - lo[k], 0.0) for k in range(3)]
    hi = [min(lo[k] + 1, n[k] - 1) for k in range(3)]

    def lerp(p, q, w):
        return p if w == 0.0 else p + w * (q - p)

    v = {(i, j, l): float(moving[(lo, hi)[i][2], (lo, hi)[j][1], (lo, hi)[l][0]]) for i in (0, 1) for j in (0, 1) for l in (0, 1)}
    row = {(i, j): lerp(v[i, j, 0], v[i, j, 1], d[0]) for i in (0, 1) for j in (0, 1)}
    plane = [lerp(row[i, 0], row[i, 1], d[1]) for i in (0, 1)]
    m = lerp(plane[0], plane[1], d[2])
    g = [lerp(lerp(v[0, 0, 1] - v[0, 0, 0], v[0, 1, 1] - v[0, 1, 0], d[1]), lerp(v[1, 0, 1] - v[1, 0, 0], v[1, 1, 1] - v[1, 1, 0], d[1]), d[2]),
         lerp(row[0, 1] - row[0, 0], row[1, 1] - row[1, 0], d[2]), plane[1] - plane[0]]
    return m, [0.0 if hi[k] == lo[k] or c[k] < 0.0 else g[k] for k in range(3)]


def _loop_parzen(m, lo_m, scale_m, n_m):
    t = min(max((m - lo_m) * scale_m + 2.0, 2.0), float(n_m - 2))
    i0 = int(min(math.floor(t), n_m - 3))
    u = t - i0
    v = 1.0 - u
    w = [v * v * v / 6.0, ((3.0 * (u * u * u) - 6.0 * (u * u)) + 4.0) / 6.0, (((-3.0 * (u * u * u) + 3.0 * (u * u)) + 3.0 * u) + 1.0) / 6.0,
         u * u * u / 6.0]
    dw = [-((v * v) * 0.5), 1.5 * (u * u) - 2.0 * u, (-1.5 * (u * u) + u) + 0.5, (u * u) * 0.5]
    return i0, w, dw


def _loop_counted(moving, a, fmask, mmask, phi):
    """``(z, y, x, m, g)`` of every fixed voxel that counts, one at a time.  The coordinates are the statement's (checked
    above); everything after them is redone."""
    shape = fmask.shape
    cs = [np.broadcast_to(c, shape).tolist() for c in F.coords(a, phi, shape)]
    for z, y, x in zip(*(v.tolist() for v in np.nonzero(fmask))):
        got = _loop_sample(moving, mmask, [cs[k][z][y][x] for k in range(3)])
        if got is not None:
            yield (z, y, x) + got


CONTRACT_RATIO = 2.17e-16  # measured with the statement on the tiny case: largest |statement - math.fsum| / largest component
CONTRACT_BOUND = 4 * CONTRACT_RATIO


def test_histogram_force_and_contraction_against_a_per_voxel_loop():
    bins, moving, a, fmask, mmask, phi = _tiny()
    n_f, n_m = 7, 9
    lo_m, scale_m = G.moving_bin_range(moving, mmask, n_m)
    table = FC.normal_table(n_f, n_m)
    hist = np.zeros((n_f, n_m), np.uint64)
    force = np.zeros((3,) + TINY_F)
    counted = 0
    for z, y, x, m, g in _loop_counted(moving, a, fmask, mmask, phi):
        counted += 1
        i0, w, dw = _loop_parzen(m, lo_m, scale_m, n_m)
        b = min(int(bins[z, y, x]), n_f - 1)
        s = 0.0
        for j in range(4):
            hist[b, i0 - 1 + j] += np.uint64(math.floor(w[j] * 2.0 ** 30 + 0.5))
            s = s + float(table[b, i0 - 1 + j]) * dw[j]
        for j in range(3):
            force[j, z, y, x] = ((s * g[0]) * a[0, j] + (s * g[1]) * a[1, j]) + (s * g[2]) * a[2, j]
    assert 40 < counted < fmask.size
    assert np.array_equal(F.joint_histogram(bins, moving, a, phi, n_f, n_m, lo_m, scale_m, fmask, mmask), hist)
    f = F.force(bins, table, moving, a, phi, n_m, lo_m, scale_m, fmask, mmask)
    assert np.array_equal(K.bits(f), K.bits(force))
    grad = F.gradient(bins, table, moving, a, phi, n_m, lo_m, scale_m, fmask, mmask)
    c = TINY_SIDE
    dense = [_bias.dense(k, b, c) for k, b, _ in (F.axis_tables(n, c) for n in TINY_F)]
    exact = np.array([[[[math.fsum(float(dense[0][z, cz] * dense[1][y, cy] * dense[2][x, cx]) * float(f[j, z, y, x])
                                   for z in range(TINY_F[0]) for y in range(TINY_F[1]) for x in range(TINY_F[2]))
                         for cx in range(c)] for cy in range(c)] for cz in range(c)] for j in range(3)])
    ratio = float(np.max(np.abs(grad - exact)) / np.max(np.abs(exact)))
    print(f"contraction: largest |statement - fsum| / largest component {ratio:.3g}")
    assert ratio <= CONTRACT_BOUND


def test_histogram_of_a_shape_with_more_tiles_than_workgroups_against_the_per_voxel_loop():
    """(130, 65, 5): the smallest of ffd_cases.CAPPED_SHAPES, which tests/test_ffd_gpu.py holds the device to.  The loop also
    counts what the tiles past the histogram kernel's 2048 workgroups add."""
    shape = FC.CAPPED_SHAPES[0]
    bins, moving, a, fmask, mmask = FC.shaped(shape, cover=True)
    a = np.asarray(a, np.float64).reshape(3, 4)
    tile = np.broadcast_to(FC.tile_index(shape), shape)
    (n_f, n_m), side = FC.BIN_PAIRS[1], 19
    lo_m, scale_m = G.moving_bin_range(moving, mmask, n_m)
    phi = FC.lattice(side, 0, 1.2)
    hist, late = [[0] * n_m for _ in range(n_f)], 0
    for z, y, x, m, _ in _loop_counted(moving, a, fmask, mmask, phi):
        i0, w, _ = _loop_parzen(m, lo_m, scale_m, n_m)
        row = hist[min(int(bins[z, y, x]), n_f - 1)]
        for j in range(4):
            row[i0 - 1 + j] += math.floor(w[j] * 2.0 ** 30 + 0.5)
        late += int(tile[z, y, x] >= 2048)
    assert F.joint_histogram(bins, moving, a, phi, n_f, n_m, lo_m, scale_m, fmask, mmask).tolist() == hist
    assert late > 1000
    for s in (4, 19):
        for cap_shape in FC.CAPPED_SHAPES:
            assert FC.check_capped(cap_shape, s) == cap_shape[0] * -(-cap_shape[1] // 4)


def test_a_non_finite_force_stays_inside_its_support():
    values = np.zeros((3, 4, 24))
    values[1, 2, 0] = np.nan  # x = 0 of 24 under side 7: nodes 0..3 along x
    out = F.contract(values, 7)
    assert np.all(np.isnan(out[:, :, :4][np.isnan(out[:, :, :4])])) and np.isnan(out[..., :4]).any()
    assert np.all(out[..., 4:] == 0.0) and not np.signbit(out[..., 4:]).any()


def test_jacobian_against_central_differences_of_the_displacement():
    _, _, _, _, _, phi = _tiny()
    shape, h = TINY_F, 1e-5
    det = F.jacobian(phi, shape)
    worst = 0.0
    for z in range(shape[0]):
        for y in range(shape[1]):
            for x in range(shape[2]):
                j = np.eye(3)
                for axis in range(3):
                    off = [0.0, 0.0, 0.0]
                    off[axis] = h
                    up = _loop_d(phi, shape, x, y, z, off)
                    off[axis] = -h
                    down = _loop_d(phi, shape, x, y, z, off)
                    for k in range(3):
                        j[k, axis] += (up[k] - down[k]) / (2 * h)
                worst = max(worst, abs(float(np.linalg.det(j)) - float(det[z, y, x])))
    print(f"Jacobian: largest |analytic - central differences| {worst:.3g}")
    # truncation h^2 |d'''| / 6 ~ 1e-10 and rounding 2^-52 |d| / h ~ 2e-11 per entry, nine entries of size <= 2 in a determinant
    assert worst <= 1e-8
    assert det.min() < 0.99  # (not the identity)


# ---- 3. the lattice gradient against central differences of -MI ---------------------------------------------------------------
def _gradient_setup(side):
    fixed, moving, g, box, ones = AC.gradient_case()
    a = R.index_affine(g, g, G.compose_affine(AC.GRADIENT_P0, np.zeros(3)))
    lo_f, scale_f = G.bin_range(fixed, box, 32)
    bins = G.bin_volume(fixed, lo_f, scale_f, 32)
    lo_m, scale_m = G.moving_bin_range(moving, ones, 32)
    phi = FC.lattice(side, 1, 0.8)

    def cost(p):
        h = F.joint_histogram(bins, moving, a, p, 32, 32, lo_m, scale_m, box, ones)
        return G.mattes_metric(h, 32, 32, scale_m) + (round(sum(int(v) for v in h.ravel().tolist()) / G.HIST_ONE),)

    c, table, n = cost(phi)
    return phi, cost, n, F.gradient(bins, table, moving, a, phi, 32, lo_m, scale_m, box, ones)


def _nodes(side):
    """Two dozen nodes: the eight corners, face and edge nodes, and interior ones, over the three components."""
    rng = np.random.default_rng(side)
    last = side - 1
    corners = [(k % 3, z, y, x) for k, (z, y, x) in enumerate((z, y, x) for z in (0, last) for y in (0, last) for x in (0, last))]
    inner = [(int(rng.integers(3)),) + tuple(int(v) for v in rng.integers(1, last, 3)) for _ in range(10)]
    faces = [(0, 0, 1, 2), (1, 2, last, 1), (2, 1, 2, 0), (0, last, last, 1), (1, 1, 0, 0), (2, 2, 1, last)]
    return corners + inner + faces


# Measured with the statement at h = 1e-4 over the 24 nodes of _nodes(): the largest |analytic - central difference| relative
# to the largest component of the gradient is 1.23e-6 at side 4 and 3.73e-6 at side 7.  The bar is 4 times the measured
# figure (the project's rule, tests/test_mi_host.py); above 1e-2 the gradient would be wrong, not noisy.
FFD_GRADIENT_RATIO = {4: 1.23e-6, 7: 3.73e-6}


@pytest.mark.parametrize("side", [4, 7])
def test_lattice_gradient_against_central_differences(side):
    phi, cost, n, grad = _gradient_setup(side)
    h, worst = 1e-4, 0.0
    assert n == 20 * 28 * 36
    for idx in _nodes(side):
        up, down = phi.copy(), phi.copy()
        up[idx] += h
        down[idx] -= h
        (c_up, _, n_up), (c_down, _, n_down) = cost(up), cost(down)
        assert n_up == n_down == n  # the box mask keeps the counted set fixed
        worst = max(worst, abs((c_up - c_down) / (2 * h) - grad[idx]))
    ratio = worst / float(np.abs(grad).max())
    print(f"side {side}: largest difference / largest component {ratio:.3g} (largest component {np.abs(grad).max():.3g})")
    assert ratio <= 4 * FFD_GRADIENT_RATIO[side] < 1e-2


def test_regulariser_gradient_is_that_of_a_quadratic():
    for side in (4, 7):
        phi = FC.lattice(side, 2)
        r, g = F.regulariser(phi)
        assert r > 0.0 and g.shape == phi.shape
        worst, h = 0.0, 1e-3
        for idx in _nodes(side):
            up, down = phi.copy(), phi.copy()
            up[idx] += h
            down[idx] -= h
            worst = max(worst, abs((F.regulariser(up)[0] - F.regulariser(down)[0]) / (2 * h) - g[idx]))
        # a central difference of a quadratic is exact; what is left is rounding: 2^-52 R / h
        assert worst / np.abs(g).max() <= 1e-9
    flat = np.zeros((3, 5, 5, 5))
    flat[0] = np.arange(5.0)[None, None, :] * 0.3 + 1.0  # a linear lattice bends nowhere
    assert F.regulariser(flat)[0] < 1e-30 and np.abs(F.regulariser(flat)[1]).max() < 1e-16


# ---- 4. subdivision and the change of level ---------------------------------------------------------------------------------
# Measured with the statement: one subdivision changes the field by at most 4.44e-16 at an amplitude of 1.5 voxels, 2.96e-16 of
# the amplitude (two more roundings per axis and tap); the bar is 4 times that.
SUBDIVIDE_BOUND = 4 * 2.96e-16


def test_subdivision_leaves_the_field_and_a_level_change_scales_it():
    shape = (9, 12, 17)
    for side in (4, 5, 7, 11):
        phi = FC.lattice(side, 4)
        fine = F.subdivide(phi)
        assert fine.shape == (3,) + (2 * side - 3,) * 3
        before, after = F.displacement(phi, shape), F.displacement(fine, shape)
        worst = max(float(np.abs(b - a).max()) for b, a in zip(before, after))
        print(f"side {side} -> {2 * side - 3}: largest change of the field {worst:.3g}")
        assert worst <= SUBDIVIDE_BOUND * np.abs(phi).max()
    with pytest.raises(ValueError, match="above 19"):
        F.subdivide(FC.lattice(19))
    assert F.to_side(FC.lattice(4), 19).shape == (3, 19, 19, 19)  # 4 -> 5 -> 7 -> 11 -> 19: no cap at 11
    with pytest.raises(ValueError, match="does not subdivide"):
        F.to_side(FC.lattice(7), 5)
    phi = FC.lattice(4, 5)
    nxt = F.next_level(phi, 5, 4, 2)
    for b, a in zip(F.displacement(phi, shape), F.displacement(nxt, shape)):
        assert np.abs(2.0 * b - a).max() <= 2 * SUBDIVIDE_BOUND * np.abs(phi).max()
    assert np.array_equal(F.next_level(phi, 4, 2, 1), 2.0 * phi)


# ---- 5. recovery ------------------------------------------------------------------------------------------------------------
# The statement on the phantom of ffd_cases (a side-5 lattice that moves voxels by up to 2.3, on top of atlas_cases' affine):
# the mean distance inside the mask between the found and the true map is 0.5817 mm after the affine stage of the existing
# code (Mattes, 12 dof) and 0.3297 mm after the default register_ffd from it; the Dice of the five labels goes from 0.916 /
# 0.923 / 0.929 to 0.944 / 0.971 / 0.955.  The pin is 1.25 times the error (libm differences between hosts).
AFFINE_ONLY_ERROR, FFD_ERROR = 0.5817, 0.3297


def test_recovery_of_a_known_lattice_on_top_of_an_affine():
    affine, found = FC.phantom_affine(), FC.phantom_ffd()
    e_affine, e_ffd = FC.map_error(affine.transform, None), FC.map_error(affine.transform, found.lattice)
    d_affine, d_ffd = FC.dices(affine.transform, None), FC.dices(affine.transform, found.lattice)
    print(f"map error: affine only {e_affine:.4f} mm, with the deformation {e_ffd:.4f} mm; {found}")
    print("Dice affine only:", {k: round(v, 4) for k, v in d_affine.items()})
    print("Dice deformed:   ", {k: round(v, 4) for k, v in d_ffd.items()})
    assert abs(e_affine - AFFINE_ONLY_ERROR) <= 0.25 * AFFINE_ONLY_ERROR  # the yardstick: the existing code
    assert e_ffd < e_affine and e_ffd <= 1.25 * FFD_ERROR
    for key in d_affine:
        assert d_ffd[key] > d_affine[key], key
    assert found.n_folded == 0 and 0.0 < found.min_jacobian < 1.0
    assert found.lattice.shape == (3, 7, 7, 7) and len(found.iterations) == 3 and found.schedule == F.DEFAULT_SCHEDULE
    assert found.affine is affine and found.transform is affine.transform and found.parameters is affine.parameters
    assert found.cost < affine.metric < 0.0  # -MI + weight R went below the affine's -MI


def test_folding_is_reported_with_the_exact_count():
    phi, mask = FC.folding_lattice(), np.ones((6, 6, 6), np.uint8)
    mask[0, :2, :3] = 0
    lo, count = F.min_jacobian(phi, mask)
    assert lo < 0.0 and abs(lo + 3.0) < 1e-12 and count == 216 - 6
    assert F.min_jacobian(phi, np.zeros((6, 6, 6), np.uint8)) == (float("inf"), 0)
    assert F.min_jacobian(0.1 * phi, mask)[1] == 0  # slope -0.4: det 0.6


# ---- 6. arguments and the ABI -------------------------------------------------------------------------------------------------
def test_python_refusals():
    fixed, moving, g, fmask, mmask, _, _ = FC.phantom()
    for bad in (np.zeros((3, 6, 6, 6)), np.zeros((2, 4, 4, 4)), np.zeros((3, 4, 4, 5)), np.full((3, 4, 4, 4), np.nan)):
        with pytest.raises(ValueError, match="lattice"):
            F.check_lattice(bad)
    for bad in ((), ((4, 6),), ((4, 7), (2, 5)), ((64, 4),), "ab", ((4, 4, 4),)):
        with pytest.raises(ValueError):
            F.check_schedule(bad, fixed.shape, moving.shape)
    for kw in ({"weight": -1.0}, {"weight": np.nan}, {"max_iter": -1}, {"max_step": 0.0}, {"bins": 65}, {"moving_bins": 4}):
        with pytest.raises(ValueError):
            F.register_ffd(fixed, moving, g, g, affine=np.eye(4), fixed_mask=fmask, moving_mask=mmask, **kw)
    with pytest.raises(ValueError, match="empty"):
        F.register_ffd(fixed, moving, g, g, affine=np.eye(4), fixed_mask=np.zeros_like(fmask), moving_mask=mmask)
    for bad in (False, 3, {"levels": 2}):
        with pytest.raises(ValueError, match="nonrigid"):
            F.nonrigid_options(bad)
    assert F.nonrigid_options(True) == {} and F.nonrigid_options({"weight": 0.1}) == {"weight": 0.1}


def test_abi_mirror_declares_the_new_symbols_as_looked_up():
    names = [s[0] for s in _abi.SYMBOLS]
    header = open(os.path.join(__import__("conftest").REPO, "include", "t2fit.h")).read()
    assert len(_abi.FFD_SYMBOLS) == 5 and _abi.ABI_VERSION == 5 and "#define T2FIT_ABI_VERSION 5" in header
    for sym in _abi.FFD_SYMBOLS:
        assert sym in names and sym + "(" in header and sym in _abi.LOOKED_UP and sym not in _abi.ADDITIVE and sym not in _abi.MI_SYMBOLS
    from fetal_t2mapping_amd import build

    assert any(s.endswith("t2fit_ffd.hip") for s in build.SOURCES)


def test_workspace_arithmetic_and_refusals_without_a_device():
    from fetal_t2mapping_amd import _gpu_ffd, build
    from fetal_t2mapping_amd._lib import load

    build.build()
    lib = load()
    assert lib.t2fit_abi_version() == 5 and all(hasattr(lib, n) for n in _abi.FFD_SYMBOLS)
    need = C.c_size_t(0)
    for shape in ((19, 23, 37), (256, 256, 256), (1, 1, 1), (5, 1027, 7)):
        for side in F.SIDES:
            assert lib.t2fit_ffd_workspace_bytes(*shape, side, C.byref(need)) == 0
            assert need.value == _gpu_ffd.workspace_bytes(shape, side), (shape, side)
    FC.check_refusals(lib, 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000, 0x9000, 0xA000, 0xB000, 0x10000, (8, 8, 8),
                      (9, 8, 7), np.eye(3, 4), 5, 7, 9, None)


# ---- 7. the drivers -----------------------------------------------------------------------------------------------------------
def test_atlas_labels_without_the_keyword_return_the_bytes_of_today():
    subject, template, g, mask, atlases, _ = AC.atlas_case()
    kw = dict(mask=mask, levels=(4,), max_iter=5)
    warped, labels, found = _atlas.atlas_labels(subject, g, template, g, atlases, **kw)
    again = _atlas.atlas_labels(subject, g, template, g, atlases, nonrigid=None, **kw)
    assert type(found) is G.Registration and type(again[2]) is G.Registration and found.parameters.tobytes() == again[2].parameters.tobytes()
    a = R.index_affine(g, g, found.transform)
    assert warped.tobytes() == again[0].tobytes() == R.resample(template, a, g.shape).tobytes()
    for n, lab in atlases.items():
        assert labels[n].tobytes() == again[1][n].tobytes() == R.resample(lab, a, g.shape, interp="nearest", default=0).tobytes()


def test_nonrigid_keywords_reach_the_loop(monkeypatch, tmp_path):
    from fetal_t2mapping_amd import recon

    base = ["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo", "--lf"]
    template, ho = str(tmp_path / "t.nii.gz"), str(tmp_path / "ho.nii.gz")
    for path in (template, ho):
        open(path, "w").close()
    good = base + ["--atlas_labels", "--atlas_template", template, "--atlas", "ho=" + ho]
    a = recon.parse_arguments(good)
    assert a.nonrigid_args is None and not a.atlas_nonrigid and not a.write_atlas_warp  # off by default
    assert recon.parse_arguments(good + ["--atlas_nonrigid"]).nonrigid_args is True
    a = recon.parse_arguments(good + ["--atlas_nonrigid", "--atlas_nonrigid_sides", "5,7", "--atlas_nonrigid_weight", "0.2",
                                      "--atlas_nonrigid_iter", "7", "--write_atlas_warp"])
    assert a.nonrigid_args == {"schedule": ((2, 5), (1, 7)), "weight": 0.2, "max_iter": 7} and a.write_atlas_warp
    for bad in (base + ["--atlas_nonrigid"], good + ["--atlas_nonrigid_sides", "4,5"], good + ["--atlas_nonrigid_weight", "0.1"],
                good + ["--atlas_nonrigid_iter", "3"], good + ["--write_atlas_warp"], good + ["--atlas_nonrigid", "--atlas_nonrigid_sides", "4,6"],
                good + ["--atlas_nonrigid", "--atlas_nonrigid_sides", "7,5"], good + ["--atlas_nonrigid", "--atlas_nonrigid_sides", "4,5,7,11"],
                good + ["--atlas_nonrigid", "--atlas_nonrigid_sides", "a"], good + ["--atlas_nonrigid", "--atlas_nonrigid_weight", "-1"],
                good + ["--atlas_nonrigid", "--atlas_nonrigid_iter", "-2"]):
        with pytest.raises(SystemExit):
            recon.parse_arguments(bad)
    # atlas_labels hands the keywords to optimize_ffd, which starts from the affine it found
    subject, template_vol, g, mask, atlases, _ = AC.atlas_case()
    seen = {}
    optimize_ffd = F.optimize_ffd

    def spy(pyramid, fg, mg, affine, **kw):
        seen.update(kw, affine=affine)
        return optimize_ffd(pyramid, fg, mg, affine, **kw)

    monkeypatch.setattr(F, "optimize_ffd", spy)
    opts = {"schedule": ((4, 4),), "weight": 0.3, "max_iter": 2, "max_step": 0.5}
    warped, labels, found = _atlas.atlas_labels(subject, g, template_vol, g, atlases, mask=mask, levels=(4,), max_iter=3, nonrigid=opts)
    assert {k: seen[k] for k in opts} == opts and (seen["bins"], seen["moving_bins"]) == (32, 32)
    assert type(found) is F.FFDRegistration and found.affine is seen["affine"] and type(found.affine) is G.Registration
    assert found.iterations == (2,) and found.lattice.shape == (3, 4, 4, 4) and np.abs(found.lattice).max() > 0.0
    a = R.index_affine(g, g, found.transform)
    assert warped.tobytes() == F.warp(template_vol, a, found.lattice, g.shape).tobytes() != R.resample(template_vol, a, g.shape).tobytes()
    assert labels["ho"].tobytes() == F.warp(atlases["ho"], a, found.lattice, g.shape, interp="nearest", default=0).tobytes()


def test_recon_atlas_nonrigid_writes_the_warp_beside_the_transform(tmp_path, monkeypatch):
    """The driver over fake_sitk, the device stage replaced by its numpy statement with a short schedule."""
    import fake_sitk

    fake = fake_sitk.install()
    monkeypatch.setitem(sys.modules, "SimpleITK", fake)
    from fetal_t2mapping_amd import cli, recon

    bids, md, template_path, specs = AC.write_atlas_subject(tmp_path)
    seen = {}

    def statement(subject, sg, template, tg, atlases, *, mask, dof, bins, device, nonrigid):
        seen["nonrigid"] = nonrigid
        return _atlas.atlas_labels(subject, sg, template, tg, atlases, mask=mask, dof=dof, bins=bins, levels=(4,), max_iter=3,
                                   nonrigid={"schedule": ((4, 4),), "max_iter": 2})

    monkeypatch.setattr(recon.t2map.atlas, "atlas_labels", statement)
    monkeypatch.setattr(recon.t2map.atlas, "extract_brain", lambda v, m: _atlas.extract_brain(v, m))
    written = recon.process_atlas_labels(md, bids, template_path, specs, nonrigid=True, write_warp=True)
    assert seen == {"nonrigid": True} and len(written) == 6
    t = AC.check_atlas_files(fake, bids, md, cli)
    npz = [p for p in written if p.endswith(".npz")]
    assert len(npz) == 1 and npz[0].replace(".npz", ".txt") in written
    warp = np.load(npz[0])
    assert np.array_equal(warp["transform"], t) and warp["lattice"].shape == (3, 4, 4, 4) and warp["lattice"].dtype == np.float64
    assert int(warp["n_folded"]) == 0 and 0.0 < float(warp["min_jacobian"]) <= 1.0
    assert len(recon.process_atlas_labels(md, bids, template_path, specs, nonrigid=True)) == 5  # no --write_atlas_warp: no .npz
