"""The correlation-ratio affine registration and the atlas-label stage, host side: the numpy statement
(fetal_t2mapping_amd/_register.py) against the sums restated from their definition, against the 43 sums it extends, the
metric against its formula, the gradient against differences, recovery of a known affine across contrasts, and the
stage on a painted atlas.  tests/test_atlas_gpu.py holds the device to the statement bit for bit."""
import os
import sys

import numpy as np
import pytest

import atlas_cases as AC
import register_cases as K
from fetal_t2mapping_amd import _abi
from fetal_t2mapping_amd import _register as G
from fetal_t2mapping_amd import _resample as R


# ---- the definition ----------------------------------------------------------------------------------------------------
def _reference_binned(name, n_bins):
    """``(N_b, S_b, sum |terms of S_b|)`` from the definition in extended precision: the voxel set of
    register_cases.counted_voxels, the eight-tap interpolant of register_cases.reference_sums, exact sums."""
    ld = np.longdouble
    fixed, moving, a, fmask, mmask = K.case(name)
    bins = AC.bins_of(name, n_bins)
    n = moving.shape[::-1]
    iz, iy, ix, c = K.counted_voxels(fixed.shape, moving.shape, a, fmask, mmask)
    padded = np.pad(moving, 1, mode="edge").astype(ld)
    lo, w = [], []
    for k in range(3):
        cc = np.clip(c[k], 0.0, float(n[k] - 1))
        base = np.floor(cc)
        t = cc.astype(ld) - base.astype(ld)
        lo.append(base.astype(np.int64) + 1)
        w.append((ld(1) - t, t))
    m = np.zeros(iz.shape, ld)
    with np.errstate(all="ignore"):
        for tz in (0, 1):
            for ty in (0, 1):
                for tx in (0, 1):
                    weight = w[0][tx] * w[1][ty] * w[2][tz]
                    m += np.where(weight == 0, ld(0), weight * padded[lo[2] + tz, lo[1] + ty, lo[0] + tx])
    b = bins[iz, iy, ix]
    counts = np.bincount(b, minlength=n_bins).astype(np.float64)
    sums = np.array([K._exact_sum(m[b == q]) for q in range(n_bins)])
    scale = np.array([K._exact_sum(np.abs(m[b == q])) for q in range(n_bins)])
    return counts, sums, scale


# The statement's largest |S_b - ref| / sum |terms| over the cases and bin counts below is 2.2e-16, inside
# register_cases.TOL = 7.4e-15 (the same tree, the same bound), which is the bar.
@pytest.mark.parametrize("name", [n for n in AC.SUMS_CASES if n != "nothing"])
@pytest.mark.parametrize("n_bins", AC.N_BINS)
def test_binned_sums_against_the_definition(name, n_bins):
    binned, lut, sums = AC.statement(name, n_bins)
    counts, ref, scale = _reference_binned(name, n_bins)
    assert binned.shape == (2 * n_bins,) and np.array_equal(binned[:n_bins], counts)
    s = binned[n_bins:]
    assert np.array_equal(s[scale == 0], ref[scale == 0])
    ratio = float(np.max(np.abs(s - ref)[scale > 0] / scale[scale > 0], initial=0.0))
    print(f"{name} B = {n_bins}: N {counts.sum():.0f}, largest |S_b - ref| / scale {ratio:.3g}")
    assert np.all(np.abs(s - ref) <= K.TOL * scale)
    # the counts add up to the N of the 43 sums bit for bit, and N and sum m do not depend on f
    assert K.bits(np.sum(binned[:n_bins])) == K.bits(sums[0]) == K.bits(K.statement_sums(name)[0])
    assert K.bits(sums[2]) == K.bits(K.statement_sums(name)[2]) and K.bits(sums[4]) == K.bits(K.statement_sums(name)[4])
    assert np.array_equal(lut[counts > 0], (s / np.where(counts > 0, counts, 1))[counts > 0]) and np.all(lut[counts == 0] == 0)
    if n_bins == 64 and counts.sum() > 1000:
        assert counts[0] > 0 and counts[63] > 0


def test_no_voxel_leaves_zeros_and_non_finite_nodes_stay_out():
    binned, lut, sums = AC.statement("nothing", 7)
    assert binned.tobytes() == np.zeros(14).tobytes() and lut.tobytes() == np.zeros(7).tobytes() and sums.tobytes() == np.zeros(43).tobytes()
    binned, _, sums = AC.statement("integer", 7)  # whole-voxel shifts next to Inf and NaN: a zero weight returns lo
    assert np.all(np.isfinite(binned)) and np.all(np.isfinite(sums)) and binned[:7].sum() == K.statement_sums("integer")[0]


def test_bin_volume_rule():
    v = np.array([[[0.0, 1.0, 9.999, 10.0, 5.0, np.nan, -3.0, np.inf, -np.inf, 20.0]]], np.float32)
    lo, scale = G.bin_range(v[..., :5], np.ones((1, 1, 5)), 4)
    assert (lo, scale) == (0.0, 0.4)
    assert G.bin_volume(v, lo, scale, 4).ravel().tolist() == [0, 0, 3, 3, 2, 0, 0, 3, 0, 3]  # hi clamps to B - 1, NaN gives 0
    assert G.bin_range(np.full((2, 2, 2), 7.0), np.ones((2, 2, 2)), 8) == (7.0, 0.0)  # lo == hi
    assert not G.bin_volume(v, 7.0, 0.0, 8).any()  # scale 0: all zeros, the infinities too (0 * inf is NaN)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="n_bins"):
            G.bin_volume(v, 0.0, 1.0, bad)
    with pytest.raises(ValueError, match="empty"):
        G.bin_range(v, np.zeros(v.shape), 4)


def test_a_table_of_the_fixed_values_gives_the_43_sums_bit_for_bit():
    """At most 64 distinct float32 values, bins = the value's rank, lut = the values: f is the fixed sample itself."""
    fixed, moving, a, fmask, mmask = K.case("prime")
    rng = np.random.default_rng(7)
    values = np.sort(rng.normal(400, 120, 64).astype(np.float32))
    rank = rng.integers(0, 64, fixed.shape).astype(np.uint8)
    want = G.registration_sums(values[rank], moving, a, fmask, mmask)
    got = G.registration_sums_lut(rank, values.astype(np.float64), moving, a, fmask, mmask)
    assert np.array_equal(K.bits(got), K.bits(want)) and np.all(got[:42] != 0)


# ---- the metric --------------------------------------------------------------------------------------------------------
def _cr_formula(binned, sums):
    n_b, s_b = binned[:binned.size // 2], binned[binned.size // 2:]
    n, sm, smm = sums[0], sums[2], sums[4]
    between = np.sum(s_b[n_b > 0] ** 2 / n_b[n_b > 0]) - sm * sm / n
    return 1.0 - between / (smm - sm * sm / n)


@pytest.mark.parametrize("name,n_bins", [("prime", 7), ("bricks", 64), ("tail257", 7)])
def test_cr_metric_is_the_definition_formula(name, n_bins):
    binned, _, sums = AC.statement(name, n_bins)
    cr, dc = G.cr_metric(binned, sums)
    print(f"{name}: CR {cr:.15f}, formula {_cr_formula(binned, sums):.15f}")
    assert abs(cr - _cr_formula(binned, sums)) <= 1e-12 and 0.0 < cr <= 1.0 and dc.shape == (3, 4)
    with pytest.raises(ValueError, match="counts add up"):
        G.cr_metric(binned[:-2], sums)


def test_cr_of_a_per_bin_remap_under_the_identity_is_zero():
    fixed = K.recovery_pair()[0]
    mask = np.ones(fixed.shape, np.uint8)
    lo, scale = G.bin_range(fixed, mask, 32)
    bins = G.bin_volume(fixed, lo, scale, 32)
    table = np.random.default_rng(3).uniform(100, 900, 32).astype(np.float32)
    binned = G.binned_sums(bins, table[bins], np.eye(3, 4), 32)
    cr, _ = G.cr_metric(binned, G.registration_sums_lut(bins, G.lut_from_binned(binned), table[bins], np.eye(3, 4)))
    print(f"CR of a per-bin remap: {cr:.3g}")
    assert abs(cr) <= 1e-12


# ---- the transform and the gradient ----------------------------------------------------------------------------------------
def test_compose_affine_and_its_parameter_gradient():
    centre = np.array([3.0, -2.0, 5.0])
    p = AC.GRADIENT_P0
    t = G.compose_affine(p, centre)
    rigid = G.compose(p[:6], centre)
    k = np.array([[np.exp(p[6]), p[9], p[10]], [0, np.exp(p[7]), p[11]], [0, 0, np.exp(p[8])]])
    assert np.allclose(t[:3, :3], rigid[:3, :3] @ k, atol=1e-15) and np.allclose(t[:3, :3] @ centre + t[:3, 3], centre + p[3:6])
    assert np.array_equal(G.compose_affine(np.r_[p[:6], np.zeros(6)], centre), rigid)
    fg = R.Geometry((28, 24, 20), (1.0, 1.1, 1.2), (-13.0, -12.0, -11.0), K.OBLIQUE.ravel())
    mg = R.Geometry((30, 21, 22), (0.9, 1.2, 1.0), (-12.5, -11.5, -10.0), (K.rot(1, 4.0) @ K.OBLIQUE).ravel())
    w = np.random.default_rng(11).normal(size=(3, 4))  # C = sum w A: dC/dA = w
    got = G.affine_parameter_gradient(w, p, centre, fg, mg)
    h = 1e-6
    for i in range(12):
        d = np.zeros(12)
        d[i] = h
        fd = np.sum(w * (R.index_affine(fg, mg, G.compose_affine(p + d, centre)) - R.index_affine(fg, mg, G.compose_affine(p - d, centre)))) / (2 * h)
        assert abs(got[i] - fd) <= 1e-7 * max(1.0, abs(fd)), (i, got[i], fd)
    assert np.array_equal(G.affine_parameter_gradient(w, p, centre, fg, mg)[3:6], (np.linalg.inv(R._index_to_point(mg)[0]).T @ w)[:, 3])


def test_dof_basis_and_scales():
    assert [G.dof_basis(d).shape for d in G.DOFS] == [(12, 6), (12, 7), (12, 9), (12, 12)]
    assert np.array_equal(G.dof_basis(7)[6:, 6], [1, 1, 1, 0, 0, 0]) and np.array_equal(G.dof_basis(9)[9:], np.zeros((3, 9)))
    with pytest.raises(ValueError, match="dof"):
        G.dof_basis(8)
    mask = np.zeros((9, 7, 5), np.uint8)
    mask[2:8, 1:6, 1:4] = 1
    g = R.Geometry((5, 7, 9), (1.0, 2.0, 3.0))
    centre, scales = G.affine_centre_and_scales(mask, g)
    pts = np.argwhere(mask)[:, ::-1] * np.array([1.0, 2.0, 3.0]) - centre
    ms = np.mean(pts ** 2, axis=0)
    assert np.allclose(scales, np.r_[[ms.sum()] * 3, 1, 1, 1, ms, ms[1], ms[2], ms[2]])


def _cr_at(p, n_bins=32):
    fixed, moving, g, box, ones = AC.gradient_case()
    centre, _ = G.affine_centre_and_scales(box, g)
    lo, scale = G.bin_range(fixed, box, n_bins)
    bins = G.bin_volume(fixed, lo, scale, n_bins)
    a = R.index_affine(g, g, G.compose_affine(p, centre))
    binned = G.binned_sums(bins, moving, a, n_bins, box, ones)
    cr, dc = G.cr_metric(binned, G.registration_sums_lut(bins, G.lut_from_binned(binned), moving, a, box, ones))
    return cr, G.affine_parameter_gradient(dc, p, centre, g, g), binned[:n_bins].sum()


# Measured with the statement: the largest |analytic - central difference| over the 12 components, relative to the
# largest component, is 1.94e-4 at h = 1e-4 (the numpy prototype of the design gave 2e-4: the differences carry the
# voxels whose bin table changes, the analytic gradient holds it fixed).  The bar is 4 times the measured figure; above
# 1e-2 the gradient would be wrong, not noisy.
GRADIENT_RATIO = 1.94e-4
GRADIENT_BOUND = 4 * GRADIENT_RATIO


def test_cr_gradient_against_central_differences():
    p0, h = AC.GRADIENT_P0, 1e-4
    cr, grad, n = _cr_at(p0)
    fd = np.zeros(12)
    for i in range(12):
        d = np.zeros(12)
        d[i] = h
        (up, _, n_up), (down, _, n_down) = _cr_at(p0 + d), _cr_at(p0 - d)
        assert n_up == n_down == n  # the box mask keeps the counted set fixed
        fd[i] = (up - down) / (2 * h)
    ratio = float(np.max(np.abs(grad - fd)) / np.max(np.abs(fd)))
    print(f"CR {cr:.6f}; analytic {grad}; differences {fd}; largest difference / largest component {ratio:.3g}")
    assert ratio <= GRADIENT_BOUND < 1e-2


# ---- recovery --------------------------------------------------------------------------------------------------------------
# The statement gives TRE 0.9628 mm (cr, 12), 2.1826 mm (cr, 6), 1.6152 mm (ncc, 12) from a start of 7.3405 mm; the pin is
# 1.25 times the first (libm differences in cos / exp between hosts).
CR12_TRE = 0.9628


def test_recovery_of_an_affine_across_contrasts():
    start = AC.tre(np.eye(4))
    cr12, cr6, ncc12 = (AC.recovered(m, d) for m, d in (("cr", 12), ("cr", 6), ("ncc", 12)))
    t12, t6, tn = AC.tre(cr12.transform), AC.tre(cr6.transform), AC.tre(ncc12.transform)
    print(f"start {start:.4f} mm; TRE cr/12 {t12:.4f}, cr/6 {t6:.4f}, ncc/12 {tn:.4f} mm; {cr12}")
    assert abs(start - AC.START_TRE) < 0.005
    assert t12 < start / 4 and t12 < t6 and t12 < tn
    assert t12 <= 1.25 * CR12_TRE
    assert cr12.parameters.shape == (12,) and len(cr12.iterations) == 3 and np.all(cr6.parameters[6:] == 0)
    assert np.array_equal(cr12.transform, G.compose_affine(cr12.parameters, cr12.centre)) and 0.0 < cr12.metric < 0.5


def test_register_affine_options():
    fixed, moving, g, fmask, mmask = AC.recovery_pair()
    kw = dict(fixed_mask=fmask, moving_mask=mmask, levels=(4,), max_iter=3)
    seven = G.register_affine(fixed, moving, g, g, dof=7, **kw)
    assert seven.parameters[6] == seven.parameters[7] == seven.parameters[8] != 0 and np.all(seven.parameters[9:] == 0)
    nine = G.register_affine(fixed, moving, g, g, dof=9, bins=8, **kw)
    assert np.all(nine.parameters[6:9] != 0) and np.all(nine.parameters[9:] == 0)
    # 'centroids': the moving grid put elsewhere in space is found again through the masks' centroids
    far = R.Geometry(g.GetSize(), g.GetSpacing(), np.array(g.GetOrigin()) + (40.0, -25.0, 30.0), g.GetDirection())
    p = G.affine_init("centroids", fmask, g, mmask, far)
    assert np.allclose(p[3:6], G.mask_centroid(mmask, far) - G.mask_centroid(fmask, g)) and np.all(p[6:] == 0) and np.all(p[:3] == 0)
    moved = G.register_affine(fixed, moving, g, far, init="centroids", **kw)
    assert np.linalg.norm(moved.parameters[3:6] - (40.0, -25.0, 30.0)) < 8.0
    with pytest.raises(ValueError, match="no voxel to compare"):
        G.register_affine(fixed, moving, g, far, **kw)
    for bad in (dict(metric="mi"), dict(bins=0), dict(bins=65), dict(dof=8), dict(init="center"), dict(init=np.zeros(6))):
        with pytest.raises(ValueError):
            G.register_affine(fixed, moving, g, g, **{**kw, **bad})


def test_abi_mirror_declares_the_new_symbols_as_looked_up():
    names = [s[0] for s in _abi.SYMBOLS]
    header = open(__import__("os").path.join(__import__("conftest").REPO, "include", "t2fit.h")).read()
    assert len(_abi.ATLAS_SYMBOLS) == 4
    for sym in _abi.ATLAS_SYMBOLS:
        assert sym in names and sym + "(" in header and sym in _abi.LOOKED_UP and sym not in _abi.ADDITIVE


def test_workspace_arithmetic_and_refusals_without_a_device():
    import ctypes as C

    from fetal_t2mapping_amd import build
    from fetal_t2mapping_amd._lib import load

    build.build()
    lib = load()
    assert lib.t2fit_abi_version() == 5 and all(hasattr(lib, n) for n in _abi.ATLAS_SYMBOLS)
    need = C.c_size_t(0)
    for shape, slabs in (((19, 23, 37), 18), ((256, 256, 256), 8192), ((5, 1027, 7), 257), ((2035, 1034, 3), 66045)):
        for n_bins in (1, 7, 32, 64):
            assert lib.t2fit_register_binned_workspace_bytes(*shape, n_bins, C.byref(need)) == 0
            assert need.value == sum((2 * n_bins * 8 * n + 255) // 256 * 256 for n in G.pass_sizes(slabs)), (shape, n_bins)
    AC.check_refusals(lib, 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000, 0x10000, 0x20000, (8, 8, 8), (9, 8, 7),
                      np.eye(3, 4), 7, None)


# ---- the stage -------------------------------------------------------------------------------------------------------------
# The statement's Dice per label against the balls carried through the true transform: 0.910 (535 voxels), 0.949 (875),
# 0.927 (1385); the bar is the 0.9 the design asks for.
def test_atlas_labels_overlap_the_labels_painted_through_the_true_transform():
    from fetal_t2mapping_amd import _atlas

    subject, template, g, mask, atlases, truth = AC.atlas_case()
    warped, labels, found = AC.atlas_statement()
    assert sorted(labels) == ["ho", "jhu"] and warped.dtype == np.float32 and warped.shape == subject.shape
    for name, lab in labels.items():
        assert lab.dtype == np.int32 and lab.shape == subject.shape and set(np.unique(lab)) == set(np.unique(atlases[name]))
        for value in np.unique(truth[name])[1:]:
            d = AC.dice(lab, truth[name], value)
            print(f"{name} label {value}: Dice {d:.4f} over {np.count_nonzero(truth[name] == value)} voxels")
            assert d >= 0.9
    assert AC.tre(found.transform) < AC.START_TRE / 4 and found.parameters.shape == (12,)
    # the warped template follows the subject's anatomy better than the template where it lay
    inside = mask != 0
    target = AC.remap(subject)[inside]
    assert np.corrcoef(warped[inside], target)[0, 1] > np.corrcoef(template[inside], target)[0, 1]
    brain = _atlas.extract_brain(subject, mask)
    assert np.array_equal(brain[inside], subject[inside]) and not brain[~inside].any() and brain.dtype == np.float32
    with pytest.raises(ValueError, match="share a grid"):
        _atlas.atlas_labels(subject, g, template, g, {"ho": atlases["ho"][1:]}, mask=mask)
    with pytest.raises(ValueError, match="integer"):
        _atlas.atlas_labels(subject, g, template, g, {"ho": atlases["ho"].astype(np.float32)}, mask=mask)


def test_recon_atlas_labels_writes_what_the_roi_reader_opens(tmp_path, monkeypatch):
    """The driver over fake_sitk, the device stage replaced by its numpy statement (tests/test_atlas_gpu.py runs the
    device's): names, grids, the transform file, and cli.py's reader on the result."""
    import fake_sitk

    from fetal_t2mapping_amd import _atlas

    fake = fake_sitk.install()
    monkeypatch.setitem(sys.modules, "SimpleITK", fake)
    from fetal_t2mapping_amd import cli, recon

    bids, md, template_path, specs = AC.write_atlas_subject(tmp_path)
    seen = {}

    def statement(subject, sg, template, tg, atlases, *, mask, dof, bins, device):
        seen.update(dof=dof, bins=bins, spacing=sg.GetSpacing())
        return _atlas.atlas_labels(subject, sg, template, tg, atlases, mask=mask, dof=dof, bins=bins, levels=(4,), max_iter=3)

    monkeypatch.setattr(recon.t2map.atlas, "atlas_labels", statement)
    monkeypatch.setattr(recon.t2map.atlas, "extract_brain", lambda v, m: _atlas.extract_brain(v, m))
    written = recon.process_atlas_labels(md, bids, template_path, specs, dof=9, bins=16)
    assert len(written) == 5 and seen == {"dof": 9, "bins": 16, "spacing": (1.0, 1.0, 1.5)}
    AC.check_atlas_files(fake, bids, md, cli)
    shifted = str(tmp_path / "shifted.nii.gz")
    np.save(shifted + ".npy", AC.atlas_case()[4]["ho"][:, :, 1:])
    with pytest.raises(ValueError, match="template's grid"):
        recon.process_atlas_labels(md, bids, template_path, [("ho", shifted)])


def test_recon_atlas_flags(tmp_path):
    from fetal_t2mapping_amd import recon

    base = ["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo", "--lf"]
    template, ho = str(tmp_path / "t.nii.gz"), str(tmp_path / "ho.nii.gz")
    for path in (template, ho):
        open(path, "w").close()
    a = recon.parse_arguments(base)
    assert (a.atlas_labels, a.atlas_template, a.atlas, a.atlas_dof, a.atlas_bins) == (False, None, [], 12, 32)  # off by default
    a = recon.parse_arguments(base + ["--atlas_labels", "--atlas_template", template, "--atlas", "ho=" + ho, "--atlas", "jhu=" + ho,
                                      "--atlas_dof", "9", "--atlas_bins", "64"])
    assert a.atlas_specs == [("ho", ho), ("jhu", ho)] and (a.atlas_dof, a.atlas_bins) == (9, 64)
    good = ["--atlas_labels", "--atlas_template", template, "--atlas", "ho=" + ho]
    for bad in (["--atlas_labels", "--atlas_template", template, "--atlas", ho],            # an --atlas without '='
                ["--atlas_labels", "--atlas", "ho=" + ho],                                    # no template
                ["--atlas_labels", "--atlas_template", str(tmp_path / "none.nii.gz"), "--atlas", "ho=" + ho],  # a missing one
                ["--atlas_labels", "--atlas_template", template],                             # no atlas
                ["--atlas_labels", "--atlas_template", template, "--atlas", "ho=" + str(tmp_path / "none.nii.gz")],
                ["--atlas_labels", "--atlas_template", template, "--atlas", "h_o=" + ho],    # a name --roi_stats refuses
                ["--atlas_labels", "--atlas_template", template, "--atlas", "mask=" + ho],   # another image's name
                good + ["--atlas", "ho=" + ho], good + ["--atlas_bins", "65"], good + ["--atlas_dof", "8"],
                ["--atlas_template", template], ["--atlas", "ho=" + ho]):                    # no effect without --atlas_labels
        with pytest.raises(SystemExit):
            recon.parse_arguments(base + bad)
    with pytest.raises(ValueError, match="NAME=FILE"):
        recon.parse_atlas_spec("ho")
