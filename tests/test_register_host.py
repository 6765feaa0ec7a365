"""The rigid registration's numpy statement (fetal_t2mapping_amd/_register.py) and what needs no device: the gradient of
the metric against differences of the metric, the identity, two recoveries of a known transform, counting / masks / rim
by hand, pyramid shapes, the summation tree, the ABI's refusals, the driver's flags and the transform files.
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
    for shape, slabs in (((19, 23, 37), 3 * 6 * 1), ((40, 48, 70), 5 * 12 * 2), ((256, 256, 256), 32 * 64 * 4)):
        assert lib.t2fit_register_workspace_bytes(*shape, C.byref(need)) == 0
        passes = G.pass_sizes(slabs)
        assert need.value == sum(up(43 * 8 * n) for n in passes) == G.workspace_bytes(shape), shape
    assert G.pass_sizes(32 * 64 * 4) == [8192, 32]
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
