"""The rigid registration's numpy statement (fetal_t2mapping_amd/_register.py) and what needs no device: the gradient of
the metric against differences of the metric, the identity, two recoveries of a known transform, counting / masks / rim
by hand, the 43 sums against their restatement in extended precision (register_cases.reference_sums), pyramid shapes and
block means, the summation tree, the ABI's refusals, the driver's flags and the transform files.
tests/test_register_gpu.py holds the device path against this statement."""
import ctypes as C
import math

import numpy as np
import pytest

import register_cases as K
from fetal_t2mapping_amd import _register as G
from fetal_t2mapping_amd import _resample as R

# measured for the case below: 5.9e-10 relative to the gradient's norm; the bar is ten times that
GRADIENT_BAR = 5.9e-9


def test_parameter_gradient_equals_central_differences_of_the_metric():
    fixed, fg, moving, mg = K.smooth_pair()
    # a fixed mask whose image stays inside the moving volume: N is then constant under the differences
    zz, yy, xx = np.meshgrid(*[np.arange(n) - (n - 1) / 2.0 for n in fixed.shape], indexing="ij")
    fmask = ((zz / 7.0) ** 2 + (yy / 8.5) ** 2 + (xx / 10.0) ** 2 <= 1.0).astype(np.uint8)
    centre, _ = G.mask_centre_and_scales(fmask, fg)
    p0 = np.array([0.031, -0.022, 0.041, 0.37, -0.61, 0.23])  # off-node

    def evaluate(p):
        s = G.registration_sums(fixed, moving, R.index_affine(fg, mg, G.compose(p, centre)), fmask, None)
        return s[0], G.metric(s)

    n0, (c0, dc) = evaluate(p0)
    assert n0 == fmask.sum() and -1.0 < c0 < -0.5
    grad = G.parameter_gradient(dc, p0, centre, fg, mg)
    h = 1e-5
    fd = np.zeros(6)
    for i in range(6):
        e = np.zeros(6)
        e[i] = h
        (na, (ca, _)), (nb, (cb, _)) = evaluate(p0 + e), evaluate(p0 - e)
        assert na == nb == n0
        fd[i] = (ca - cb) / (2 * h)
    err = float(np.linalg.norm(grad - fd) / np.linalg.norm(fd))
    print(f"relative gradient error {err:.3e}")
    assert GRADIENT_BAR <= 1e-3 and err < GRADIENT_BAR


def test_identical_volumes_stay_at_the_identity_bit_for_bit():
    fixed, _, g, fmask, _ = K.recovery_pair()
    r = G.register_rigid(fixed, fixed, g, g, fixed_mask=fmask, moving_mask=fmask)
    assert r.parameters.tobytes() == np.zeros(6).tobytes() and np.array_equal(r.transform, np.eye(4))
    assert r.iterations == (0, 0, 0) and r.stops == ("gradient",) * 3
    assert abs(r.metric + 1.0) < 1e-12
    centre, scales = G.mask_centre_and_scales(fmask, g)
    c, dc = G.metric(G.registration_sums(fixed, fixed, R.index_affine(g, g), fmask, fmask))
    assert np.linalg.norm(G.parameter_gradient(dc, np.zeros(6), centre, g, g) / scales) < G.GRAD_TOL


def test_noise_free_recovery_of_a_known_transform():
    fixed, moving, g, fmask, mmask = K.recovery_pair()
    r = G.register_rigid(fixed, moving, g, g)  # masks from build_mask
    tre = G.target_registration_error(r.transform, K.RECOVERY_TRUE, fmask, g)
    print(r, f"TRE {tre:.4f} mm")
    assert tre < 0.5
    assert r.metric < -0.999 and len(r.iterations) == 3 and r.stop in ("gradient", "step", "iterations")
    # what the GPU test compares with: two levels, 40 iterations, masks given
    r2 = G.register_rigid(fixed, moving, g, g, fixed_mask=fmask, moving_mask=mmask, levels=(2, 1), max_iter=40)
    assert G.target_registration_error(r2.transform, K.RECOVERY_TRUE, fmask, g) < 0.5


REAL_TRUE = K.rigid((2.0, -1.5, 2.5), (1.5, -1.0, 1.2))


def real_geometry_pair():
    """The vial phantom of tests/test_recon_gpu.py as thick-slice ax and cor stacks; the cor stack's declared geometry is
    its true one moved by REAL_TRUE, so the fixed point x lies at REAL_TRUE x of the declared cor frame.  Stage 1 applied:
    ``(H_ax, grid, H_cor, grid)``."""
    import test_recon_gpu as RG

    stacks, geoms, _, _, _, _ = RG._phantom_stacks(n_te=1, side=48, thick=4.0, seed=25)
    cor = geoms["cor"]
    moved = R.Geometry(cor.GetSize(), cor.GetSpacing(), REAL_TRUE[:3, :3] @ np.array(cor.GetOrigin()) + REAL_TRUE[:3, 3],
                       (REAL_TRUE[:3, :3] @ np.array(cor.GetDirection()).reshape(3, 3)).ravel())
    out = []
    for stack, g in ((stacks["ax"][0], geoms["ax"]), (stacks["cor"][0], moved)):
        iso = R.isotropic_geometry(g, 1.0)
        out += [R.resample(stack, R.index_affine(iso, g), iso.shape), iso]
    return out


def test_recovery_on_thick_slice_stacks_is_sub_voxel():
    h_ax, g_ax, h_cor, g_cor = real_geometry_pair()
    r = G.register_rigid(h_ax, h_cor, g_ax, g_cor)
    tre = G.target_registration_error(r.transform, REAL_TRUE, G.build_mask(h_ax), g_ax)
    print(r, f"TRE {tre:.4f} mm")
    assert tre < 1.0


def test_counting_masks_and_the_rim_by_hand():
    rng = np.random.default_rng(3)
    moving = rng.normal(100, 20, (3, 3, 4)).astype(np.float32)  # (Z, Y, X)
    fixed = rng.normal(100, 20, (3, 3, 4)).astype(np.float32)
    ident = np.eye(3, 4)
    s = G.registration_sums(fixed, moving, ident)
    f64, m64 = fixed.astype(np.float64), moving.astype(np.float64)
    assert s[0] == 36 and np.isclose(s[1], f64.sum(), rtol=1e-14) and np.isclose(s[5], (f64 * m64).sum(), rtol=1e-14)
    # at the nodes: m is the node; g_x is the forward difference, 0 on the last column (the upper neighbour is clamped)
    gx = np.zeros_like(m64)
    gx[:, :, :-1] = m64[:, :, 1:] - m64[:, :, :-1]
    assert np.isclose(s[6 + 3], gx.sum(), rtol=1e-13) and np.isclose(s[6 + 12 + 3], (f64 * gx).sum(), rtol=1e-13)
    assert np.isclose(s[6 + 0], (gx * np.arange(4)[None, None, :]).sum(), rtol=1e-13)
    # masks: a fixed voxel off, and a moving node off that is the nearest node of exactly one fixed voxel
    fm, mm = np.ones(fixed.shape, np.uint8), np.ones(moving.shape, np.uint8)
    fm[0, 1, 2] = 0
    mm[2, 2, 3] = 0
    s2 = G.registration_sums(fixed, moving, ident, fm, mm)
    assert s2[0] == 34 and np.isclose(s2[1], f64.sum() - f64[0, 1, 2] - f64[2, 2, 3], rtol=1e-14)
    # a shift of -0.25 in x: column 0 lies on the lower rim (c = -0.25: inside, m = node 0, flat), +0.75 pushes column 3
    # to c = 3.75 >= 3.5: outside
    a = ident.copy()
    a[0, 3] = -0.25
    s3 = G.registration_sums(fixed, moving, a)
    assert s3[0] == 36
    want_m = np.empty_like(m64)
    want_m[:, :, 0] = m64[:, :, 0]
    want_m[:, :, 1:] = m64[:, :, :-1] + 0.75 * (m64[:, :, 1:] - m64[:, :, :-1])
    assert np.isclose(s3[2], want_m.sum(), rtol=1e-14)
    gx3 = np.zeros_like(m64)
    gx3[:, :, 1:] = m64[:, :, 1:] - m64[:, :, :-1]
    assert np.isclose(s3[6 + 3], gx3.sum(), rtol=1e-13)
    a[0, 3] = 0.75
    assert G.registration_sums(fixed, moving, a)[0] == 27
    # nothing counts: 43 zeros, and the metric refuses instead of dividing by zero
    a[0, 3] = 40.0
    s4 = G.registration_sums(fixed, moving, a)
    assert s4.tobytes() == np.zeros(43).tobytes()
    with pytest.raises(ValueError, match="no voxel to compare"):
        G.metric(s4)


def test_pyramid_levels_on_ragged_sizes():
    rng = np.random.default_rng(4)
    v = rng.normal(300, 50, (19, 23, 37)).astype(np.float32)
    m = (rng.random(v.shape) < 0.02).astype(np.uint8)
    g = R.Geometry((37, 23, 19), (1.0, 1.1, 1.2), (-3.0, 2.0, 5.0), K.OBLIQUE.ravel())
    for s, shape in ((1, (19, 23, 37)), (2, (9, 11, 18)), (4, (4, 5, 9))):
        lv, lm, lg = G.shrink(v, s), G.shrink_mask(m, s), G.level_geometry(g, s)
        assert lv.shape == lm.shape == shape == G.level_shape(v.shape, s) == lg.shape and lv.dtype == np.float32
        z, y, x = 1, 2, 3
        block = v[z * s:(z + 1) * s, y * s:(y + 1) * s, x * s:(x + 1) * s]
        assert np.isclose(lv[z, y, x], block.astype(np.float64).mean(), rtol=1e-6)
        assert lm[z, y, x] == int(m[z * s:(z + 1) * s, y * s:(y + 1) * s, x * s:(x + 1) * s].any())
        # the level's voxel 0 sits at the centre of the first block
        mat, o = R._index_to_point(g)
        assert np.allclose(lg.GetOrigin(), o + mat @ np.full(3, (s - 1) / 2.0)) and np.allclose(lg.GetSpacing(), np.array(g.GetSpacing()) * s)
    assert np.array_equal(G.shrink(v, 1), v)
    with pytest.raises(ValueError, match="fewer than"):
        G.check_levels((8, 1), v.shape, v.shape)
    with pytest.raises(ValueError, match="shrink factors"):
        G.check_levels((0,), v.shape, v.shape)


def test_the_summation_tree_adds_every_term_once():
    """Against math.fsum of the same terms: a wrong tree (a slab dropped or added twice, a pad that is not zero) misses
    by far more than 1e-12."""
    fixed, fg, moving, mg = K.smooth_pair()
    big = np.tile(fixed, (3, 2, 3))[:41, :, :70]  # several bricks per axis and ragged last ones
    a = R.index_affine(fg, mg, G.compose([0.02, -0.01, 0.03, 0.3, -0.2, 0.4], np.zeros(3)))
    fm, mm = np.ones(big.shape, np.uint8), np.ones(moving.shape, np.uint8)
    s = G.registration_sums(big, moving, a, fm, mm)
    assert G.brick_counts(big.shape) == (6, 12, 2) and G.pass_sizes(144) == [144] and G.pass_sizes(70000) == [70000, 274, 2]
    terms = np.concatenate([G._terms(big, fm, moving, mm, a, z, 1) for z in range(big.shape[0])], axis=1)
    assert s[0] > 1000
    for q in range(G.N_SUMS):
        exact = math.fsum(terms[q].ravel().tolist())
        scale = math.fsum(np.abs(terms[q]).ravel().tolist())
        assert abs(s[q] - exact) <= 1e-12 * scale, q
    # more than one pass: 300 slabs of ones
    assert np.array_equal(G.reduce_slabs(np.ones((43, 300))), np.full(43, 300.0))
    # two passes whose first ends in a ragged group, on real slabs: against the sums restated from the definition
    for name, bricks, passes in (("tail774", (3, 258, 1), [774, 4]), ("tail257", (1, 257, 1), [257, 2])):
        shape = K.case(name)[0].shape
        assert G.brick_counts(shape) == bricks and G.pass_sizes(int(np.prod(bricks))) == passes
        assert np.all(K.counted_per_slab(name)[passes[0] // 256 * 256:] > 0)  # every slab of the ragged group is something
        K.assert_within_reference(K.statement_sums(name), name)


@pytest.mark.parametrize("name", K.REFERENCE_CASES)
def test_the_statement_equals_the_sums_restated_from_the_definition(name):
    """register_cases.reference_sums shares the float64 coordinates with the statement and nothing else: eight-tap weight
    products in extended precision on a padded volume instead of nested float64 lerps, the counted voxels gathered, every
    sum exact.  ``|s - ref| <= TOL * scale`` per sum (scale: the sum of the absolute terms) and the count exactly.

    Measured, the statement's largest ``|s - ref| / scale`` per case: prime 2.2e-16, bricks 1.9e-16, empty_bricks
    1.8e-16, outside 1.7e-16, tail774 3.7e-18, tail257 2.2e-16, moving_x1 2.2e-16, moving_y1 1.5e-16, moving_z1 1.8e-16,
    fixed_1x1x1 4.6e-16 (one voxel: a single term's roundings), fixed_3x2x5 1.7e-16, fixed_9x6x65 2.1e-16, fixed_8x4x64
    2.4e-17, integer 1.9e-16, half_rim 1.4e-16.  The largest is 4.6e-16; TOL is 16 times it, 7.4e-15.  The largest N is
    57 340, so TOL * N < 1e-9: a voxel dropped or counted twice changes sum 0 by 1 and the others by about 1 / N of their
    scale, far above the bar."""
    fixed, _, _, fmask, _ = K.case(name)
    s = K.statement_sums(name)
    assert K.TOL == 16 * 4.6e-16
    K.assert_within_reference(s, name)
    if name in ("prime", "bricks", "empty_bricks", "outside") + K.TWO_PASS:  # the non-trivial cases of the device tests
        assert 1000 < s[0] < 0.6 * fmask.sum() and np.all(s[1:42] != 0) and s[42] == 0


def test_the_rim_and_degenerate_cases_are_what_they_claim():
    # a moving axis of one voxel: thousands count, the interpolant is flat along it (its 12 gradient sums are exactly 0)
    for axis, name in enumerate(("moving_x1", "moving_y1", "moving_z1")):
        s = K.statement_sums(name)
        assert K.case(name)[1].shape[2 - axis] == 1 and s[0] > 5000
        flat = [6 + 4 * (3 * w + axis) + j for w in range(3) for j in range(4)]
        assert np.all(s[flat] == 0) and np.all(np.delete(s[1:42], np.array(flat) - 1) != 0)
    assert K.statement_sums("fixed_1x1x1")[0] == 1 and K.statement_sums("fixed_3x2x5")[0] == 30
    # half_rim: c = i - 0.5; the voxels on c = -0.5 count, those on c = n - 0.5 do not
    fixed, moving, a, fmask, mmask = K.case("half_rim")
    iz, iy, ix, c = K.counted_voxels(fixed.shape, moving.shape, a, fmask, mmask)
    assert (ix == 0).any() and (iy == 0).any() and (iz == 0).any()
    assert ix.max() == moving.shape[2] - 1 and iy.max() == moving.shape[1] - 1 and iz.max() == moving.shape[0] - 1
    assert fmask[-1].any() and fmask[:, -1].any() and fmask[:, :, -1].any()  # they were there to be refused
    # integer: the non-finite nodes are masked, their lower edge and corner neighbours and upper neighbours count, and
    # nothing non-finite reaches a sum; off the nodes by 2^-40 it does, in the statement as in the reference
    fixed, moving, a, fmask, mmask = K.case("integer")
    iz, iy, ix, c = K.counted_voxels(fixed.shape, moving.shape, a, fmask, mmask)
    at = set(zip((iz + int(a[2, 3])).tolist(), (iy + int(a[1, 3])).tolist(), (ix + int(a[0, 3])).tolist()))  # moving nodes hit
    touched = 0
    for z, y, x, v in K.NON_FINITE_NODES:
        assert not np.isfinite(moving[z, y, x]) and mmask[z, y, x] == 0 and (z, y, x) not in at
        lower = [(z - dz, y - dy, x - dx) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1) if dz + dy + dx >= 2]
        touched += sum(p in at for p in lower)
    assert touched >= 8  # voxels that count and have a non-finite node among their eight taps, at weight 0
    assert np.all(np.isfinite(K.statement_sums("integer"))) and K.statement_sums("integer")[0] == len(iz)
    off, (ref, _) = K.statement_sums("integer_eps"), K.reference("integer_eps")
    assert off[0] == ref[0] == len(iz) and np.array_equal(np.isfinite(off), np.isfinite(ref)) and not np.all(np.isfinite(off))


@pytest.mark.parametrize("s", K.PYRAMID_FACTORS)
def test_block_means_are_the_correctly_rounded_ones(s):
    """The statement adds a block's float32 values in float64 in a fixed order and divides: at most s^3 + 1 roundings of
    2^-53 each, 4e-12 relative at s = 32, against half a float32 ulp of 6e-8.  The float32 result is therefore one of the
    two float32 neighbours of the exact mean: the correctly rounded one, or -- when the exact mean lies within 4e-12
    relative of a tie -- the one next to it.  The bar is 1 ulp; measured: 0 of 16169, 504, 84 and 2 values differ."""
    v, m = K.pyramid_case(s)
    got, want = G.shrink(v, s), K.block_means(s)
    assert got.shape == want.shape == G.level_shape(v.shape, s) and all(n % s for n in v.shape) == (s > 1)
    ulps = np.abs(K.ordered(got) - K.ordered(want))
    print(f"s = {s}: {np.count_nonzero(ulps)} of {ulps.size} block means are not the correctly rounded one")
    assert ulps.max() <= 1
    lm = G.shrink_mask(m, s)
    assert 0 < lm.sum() < lm.size


# ---- the ABI, without a device ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from fetal_t2mapping_amd import build
    from fetal_t2mapping_amd._lib import load

    build.build()
    return load()


def _err(lib):
    return lib.t2fit_last_error().decode()


def test_symbols_workspace_arithmetic_and_refusals_without_a_device(lib):
    from fetal_t2mapping_amd import _abi

    assert lib.t2fit_abi_version() == 5 and all(hasattr(lib, n) for n in _abi.REGISTER_SYMBOLS)
    need = C.c_size_t(0)
    up = lambda v: (v + 255) // 256 * 256
    for shape, slabs in (((19, 23, 37), 3 * 6 * 1), ((40, 48, 70), 5 * 12 * 2), ((256, 256, 256), 32 * 64 * 4),
                         ((19, 1030, 5), 774), ((5, 1027, 7), 257), ((2035, 1034, 3), 66045)):
        assert lib.t2fit_register_workspace_bytes(*shape, C.byref(need)) == 0
        passes = G.pass_sizes(slabs)
        assert need.value == sum(up(43 * 8 * n) for n in passes) == G.workspace_bytes(shape), shape
    assert G.pass_sizes(32 * 64 * 4) == [8192, 32]
    assert G.pass_sizes(774) == [774, 4] and G.pass_sizes(257) == [257, 2] and G.pass_sizes(66045) == [66045, 258, 2]
    assert lib.t2fit_register_workspace_bytes(4, 4, 4, None) == _abi.E_INVALID
    assert lib.t2fit_register_workspace_bytes(4, 0, 4, C.byref(need)) == _abi.E_INVALID and ">= 1" in _err(lib)

    A = (C.c_double * 12)(*np.eye(3, 4).ravel())
    nan = (C.c_double * 12)(*np.eye(3, 4).ravel())
    nan[5] = np.nan
    assert lib.t2fit_register_workspace_bytes(8, 8, 8, C.byref(need)) == 0

    def call(f=0x1000, fm=0x2000, fs=(8, 8, 8), m=0x3000, mm=0x4000, ms=(8, 8, 8), A=A, sums=0x5000, ws=0x10000, nb=need.value):
        return lib.t2fit_register_sums_dev(f, fm, *fs, m, mm, *ms, A, sums, ws, nb, None)

    for kwargs, text in (({"f": None}, "NULL"), ({"fm": None}, "NULL"), ({"m": None}, "NULL"), ({"mm": None}, "NULL"),
                         ({"A": None}, "NULL"), ({"sums": None}, "NULL"), ({"ws": None}, "NULL"),
                         ({"fs": (8, 0, 8)}, "fixed sizes"), ({"ms": (8, 8, -1)}, "moving sizes"), ({"A": nan}, "non-finite"),
                         ({"f": 0x1002}, "aligned to 4"), ({"m": 0x3001}, "aligned to 4"), ({"sums": 0x5004}, "aligned to 8"),
                         ({"ws": 0x10080}, "aligned to 256"), ({"nb": need.value - 1}, "workspace too small")):
        assert call(**kwargs) == _abi.E_INVALID, kwargs
        assert text in _err(lib), (kwargs, _err(lib))
    for fn in (lib.t2fit_shrink_dev, lib.t2fit_shrink_mask_dev):
        for args, text in (((None, 8, 8, 8, 2, 0x2000), "NULL"), ((0x1000, 8, 8, 8, 2, None), "NULL"),
                           ((0x1000, 8, 8, 8, 2, 0x1000), "must not be src_dev"), ((0x1000, 8, 0, 8, 2, 0x2000), ">= 1"),
                           ((0x1000, 8, 8, 8, 0, 0x2000), "outside 1..32"), ((0x1000, 8, 8, 8, 33, 0x2000), "outside 1..32"),
                           ((0x1000, 8, 3, 8, 4, 0x2000), "empty")):
            assert fn(*args, None) == _abi.E_INVALID, args
            assert text in _err(lib), (args, _err(lib))
    assert lib.t2fit_shrink_dev(0x1002, 8, 8, 8, 2, 0x2000, None) == _abi.E_INVALID and "aligned to 4" in _err(lib)


# ---- drivers ---------------------------------------------------------------------------------------------------------
def test_driver_flags_refusals_and_the_transform_files(tmp_path):
    from fetal_t2mapping_amd import cli, recon

    base = ["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo", "--lf"]
    a = recon.parse_arguments(base)
    assert (a.register, a.register_echoes, a.write_transforms) == (False, False, None)  # off by default
    a = recon.parse_arguments(base + ["--register", "--register_echoes", "--write_transforms", str(tmp_path / "t")])
    assert (a.register, a.register_echoes, a.write_transforms) == (True, True, str(tmp_path / "t"))
    for bad in (["--register", "--transforms", str(tmp_path)], ["--register_echoes", "--transforms", str(tmp_path)],
                ["--write_transforms", str(tmp_path)]):
        with pytest.raises(SystemExit):
            recon.parse_arguments(base + bad)
    cbase = ["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo", "--gaussian", "--lf", "--sim", "s"]
    a = cli.parse_arguments(cbase + ["--reconstruct", "--recon_register", "--recon_register_echoes"])
    assert a.reconstruct_args == {"fixed": "ax", "res": 1.0, "transforms_dir": None, "register": True, "register_echoes": True}
    for bad in (["--recon_register"], ["--reconstruct", "--recon_register", "--recon_transforms", str(tmp_path)]):
        with pytest.raises(SystemExit):
            cli.parse_arguments(cbase + bad)
    # what --write_transforms writes, --transforms reads back bit for bit; an echo's own file goes before the subject's
    acq = {"sub": "sub-001", "ses": "ses-01", "EchoTime": 0.114}
    other = {"sub": "sub-001", "ses": "ses-01", "EchoTime": 0.202}
    t = {"cor": K.rigid((1.234567, -2.5, 0.3), (1 / 3, -2 / 7, 1e-3)), "sag": K.RECOVERY_TRUE}
    out = str(tmp_path / "found")
    paths = recon.save_transforms(out, acq, t)
    assert [p.split("/")[-1] for p in paths] == ["sub-001_ses-01_te-114_cor.txt", "sub-001_ses-01_te-114_sag.txt"]
    got = recon.load_transforms(out, acq, "ax")
    assert sorted(got) == ["cor", "sag"] and all(got[o].tobytes() == t[o].tobytes() for o in t)
    assert recon.load_transforms(out, other, "ax") == {}
    np.savetxt(recon.transform_path(out, acq, "cor"), np.eye(4))
    assert np.array_equal(recon.load_transforms(out, other, "ax")["cor"], np.eye(4))
    assert recon.load_transforms(out, acq, "ax")["cor"].tobytes() == t["cor"].tobytes()
