"""The numpy statement of the tissue segmentation (fetal_t2mapping_amd._seg) against a per-voxel reference written from the
definition (tests/seg_cases.py), the behaviour of the EM loop, its benefit on a phantom, and the plumbing that needs no
device: the library's workspace arithmetic and refusals, recon.py's flags, atlas_labels(tissue=...)."""
import ctypes as C
import math
import sys

import numpy as np
import pytest
import seg_cases as SC

from fetal_t2mapping_amd import _abi, _seg


# ---- taps and blur ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.3, 0.7, 1.0, 2.0, 2.5, 8.0])
def test_taps_are_symmetric_normalised_and_use_scipys_radius(sigma):
    w = _seg.gauss_taps(sigma)
    r = int(4.0 * sigma + 0.5)
    assert w.dtype == np.float64 and len(w) == 2 * r + 1
    assert np.array_equal(w, w[::-1])
    assert abs(math.fsum(w) - 1.0) <= 2.0 ** -52
    from scipy.ndimage import gaussian_filter1d

    impulse = np.zeros(4 * r + 3)
    impulse[2 * r + 1] = 1.0
    got = gaussian_filter1d(impulse, sigma, mode="constant", truncate=4)
    assert np.count_nonzero(got) == 2 * r + 1 and np.allclose(got[got != 0], w, rtol=0, atol=1e-15)


def test_taps_edges():
    assert np.array_equal(_seg.gauss_taps(0.0), [1.0]) and np.array_equal(_seg.gauss_taps(0.1), [1.0])
    assert len(_seg.gauss_taps(8.1)) == 65
    for bad in (8.2, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            _seg.gauss_taps(bad)
    with pytest.raises(ValueError):
        _seg.priors_from_labels(np.zeros((3, 3, 3), np.int32), [1, 2], (1.0, 2.0))


@pytest.mark.parametrize("sigma", [0.7, (0.0, 1.0, 0.5)])
def test_priors_equal_the_triple_loop_reference(sigma):
    classes, labels, _, _, _ = SC.random_case((5, 6, 7), 3, 1, seed=1)
    got = _seg.priors_from_labels(labels, classes, sigma)
    taps = [_seg.gauss_taps(s) for s in np.broadcast_to(sigma, (3,))]
    want = SC.ref_priors(labels, classes, taps)
    assert got.dtype == np.float32 and got.shape == (3, 5, 6, 7)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("sigma", [0.7, 1.0, 2.5])
def test_priors_are_scipys_gaussian_filter_within_one_ulp_at_one(sigma):
    from scipy.ndimage import gaussian_filter

    classes, labels, _, _, _ = SC.random_case((11, 13, 17), 3, 1, seed=2)
    got = _seg.priors_from_labels(labels, classes, sigma)
    want = np.stack([gaussian_filter((labels == c).astype(np.float32), sigma, mode="constant", truncate=4) for c in classes])
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"sigma {sigma}: max |difference| = 2^{np.log2(err) if err else -np.inf:.1f}")
    assert err <= 2.0 ** -24


def test_normalise_priors():
    classes, labels, _, mask, _ = SC.random_case((4, 5, 6), 3, 1, seed=3)
    prior = _seg.priors_from_labels(labels, classes, 1.0)
    pi = _seg.normalise_priors(prior, mask, 1e-3)
    inside = mask != 0
    assert pi.dtype == np.float32 and not pi[:, ~inside].any()
    for idx in np.argwhere(inside)[::7]:
        v = [float(prior[(k,) + tuple(idx)]) for k in range(3)]
        den = ((0.0 + v[0]) + v[1]) + v[2] + 3 * 1e-3
        for k in range(3):
            assert pi[(k,) + tuple(idx)] == np.float32((v[k] + 1e-3) / den)
    assert np.abs(pi[:, inside].astype(np.float64).sum(axis=0) - 1.0).max() <= 3 * 2.0 ** -24


# ---- sums ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,K,C", [((3, 5, 7), 2, 1), ((1, 25, 41), 3, 2), ((2, 16, 37), 8, 4)])
def test_moment_sums_against_fsum_and_the_literal_tree(shape, K, C):
    _, _, y, mask, p = SC.random_case(shape, K, C, seed=4, nan=True)
    got = _seg.moment_sums(p, y, mask)
    assert got.shape == (K, 1 + C + C * (C + 1) // 2) and got.dtype == np.float64
    n_vox = int(np.prod(shape))
    for k in range(K):
        terms, where = SC.ref_terms(p, y, mask, k)
        for m, t in enumerate(terms):
            exact = math.fsum(t)
            assert abs(got[k, m] - exact) <= 8 * 2.2e-16 * math.fsum(abs(v) for v in t), (k, m)
            if k in (0, K - 1):
                assert got[k, m] == SC.ref_tree(t, where, n_vox), (k, m)  # bit for bit


def test_moment_sums_tree_with_a_second_reduce_pass():
    shape = SC.TWO_PASS_SHAPE
    rng = np.random.default_rng(5)
    y = (100.0 + 20.0 * rng.standard_normal((1,) + shape)).astype(np.float32)
    p = rng.random((2,) + shape).astype(np.float32)
    mask = (rng.random(shape) < 0.7).astype(np.uint8)
    got = _seg.moment_sums(p, y, mask)
    terms, where = SC.ref_terms(p, y, mask, 1)
    assert int(np.prod(shape)) > 1024 * 256
    assert got[1, 1] == SC.ref_tree(terms[1], where, int(np.prod(shape)))
    assert abs(got[1, 1] - math.fsum(terms[1])) <= 8 * 2.2e-16 * math.fsum(abs(v) for v in terms[1])


# ---- E-step ----------------------------------------------------------------------------------------------------------------
def _model_of(p, y, mask, C, dead_last=False):
    sums = _seg.moment_sums(p, y, mask)
    if dead_last:
        sums[-1] = 0.0
    return _seg.class_model(sums, C, 1e-6)


@pytest.mark.parametrize("shape,K,C,dead", [((3, 5, 7), 2, 1, False), ((4, 6, 5), 3, 2, True), ((3, 4, 6), 8, 4, False)])
def test_e_step_against_the_per_voxel_reference(shape, K, C, dead):
    _, _, y, mask, p = SC.random_case(shape, K, C, seed=6, nan=True)
    model = _model_of(p, y, mask, C, dead)
    rows, live = _seg.pack_model(model)
    assert bool(model.dead[-1]) == dead
    pi = _seg.normalise_priors(p, _seg.effective_mask(y, mask), 1e-3)
    got = _seg.e_step(p, pi, y, mask, model, 0.5)
    want = SC.ref_e_step(p, pi, y, mask, rows, live, 0.5)
    M = SC.ref_in_m(y, mask)
    assert got.dtype == np.float32 and np.all(np.isfinite(got))
    assert SC.ulp_distance_f32(got, want).max() <= 1
    assert not got[:, ~M].view(np.uint32).any() and not got[~live.astype(bool)].view(np.uint32).any()  # exactly +0.0
    assert np.count_nonzero(~M) > 0 and not M[tuple(v // 2 for v in shape)]  # the NaN voxel is outside M
    assert np.abs(got[:, M].astype(np.float64).sum(axis=0) - 1.0).max() <= K * 2.0 ** -24
    # beta = 0: no neighbour enters
    other = np.roll(p, 1, axis=0)
    assert np.array_equal(_seg.e_step(p, pi, y, mask, model, 0.0), _seg.e_step(other, pi, y, mask, model, 0.0))
    assert not np.array_equal(got, _seg.e_step(other, pi, y, mask, model, 0.5))


def test_hard_labels_take_the_first_maximum():
    p = np.zeros((3, 1, 1, 4), np.float32)
    p[:, 0, 0, 0] = (0.2, 0.5, 0.3)
    p[:, 0, 0, 1] = (0.4, 0.4, 0.2)  # a tie: the first
    p[:, 0, 0, 2] = (0.1, 0.1, 0.8)
    p[:, 0, 0, 3] = (0.1, 0.1, 0.8)  # outside the mask
    got = _seg.hard_labels(p, [5, 2, 9], np.array([[[1, 1, 1, 0]]], np.uint8))
    assert got.dtype == np.int32 and got.ravel().tolist() == [2, 5, 9, 0]


# ---- EM behaviour ----------------------------------------------------------------------------------------------------------
def test_em_finds_the_means_of_a_separated_mixture_from_flat_priors():
    rng = np.random.default_rng(7)
    shape, means, sigma = (8, 16, 16), (100.0, 200.0, 300.0), 10.0
    truth = rng.integers(0, 3, shape)
    y = (np.choose(truth, means) + sigma * rng.standard_normal(shape)).astype(np.float32)[None]
    # exactly flat priors are a fixed point (every class gets the same model): a faint hint (0.34 / 0.33 / 0.33) breaks the
    # symmetry, and EM leaves the neighbourhood of that point slowly, hence 60 iterations
    prior = np.full((3,) + shape, 0.33, np.float32)
    for k in range(3):
        prior[k][truth == k] = 0.34
    res = _seg.segment_em(y, None, prior, [1, 2, 3], beta=0.0, n_iter=60)
    assert res.n_iter == 60 and res.s0_trace.shape == (60, 3) and not res.model.dead.any()
    for k in range(3):
        n_k = np.count_nonzero(truth == k)
        assert abs(res.model.mean[k, 0] - means[k]) <= 5 * sigma / np.sqrt(n_k), (k, res.model.mean[k, 0])
    assert np.mean(res.labels == truth + 1) > 0.99
    # tol: stops early, on the same path
    early = _seg.segment_em(y, None, prior, [1, 2, 3], beta=0.0, n_iter=60, tol=1e-6)
    assert 1 < early.n_iter < 60 and np.array_equal(early.s0_trace, res.s0_trace[:early.n_iter])


def test_the_potts_term_flips_one_wrong_voxel_inside_a_homogeneous_region():
    rng = np.random.default_rng(8)
    shape = (9, 9, 18)
    truth = np.zeros(shape, int)
    truth[:, :, 9:] = 1
    y = (np.choose(truth, (100.0, 140.0)) + 10.0 * rng.standard_normal(shape)).astype(np.float32)
    # deep in class 0, an intensity that class 1 explains better: 2.5 sigma from 100, 1.5 sigma from 140, so the log-likelihoods
    # differ by 2 and the priors by log(0.55 / 0.45) = 0.2 the other way.  Six neighbours that are surely class 0 cost class 1
    # 6 beta = 3 at beta = 0.5: more than 1.8
    y[4, 4, 4] = 125.0
    prior = np.full((2,) + shape, 0.5, np.float32)
    prior[0][truth == 0] = 0.55
    prior[1][truth == 1] = 0.55
    kw = dict(n_iter=15, var_floor=1e-6)
    plain = _seg.segment_em(y[None], None, prior, [1, 2], beta=0.0, **kw)
    potts = _seg.segment_em(y[None], None, prior, [1, 2], beta=0.5, **kw)
    assert plain.labels[4, 4, 4] == 2 and potts.labels[4, 4, 4] == 1


def test_a_class_without_prior_mass_ends_dead_and_all_dead_raises():
    rng = np.random.default_rng(9)
    shape = (4, 8, 8)
    truth = rng.integers(0, 2, shape)
    y = (np.choose(truth, (100.0, 200.0)) + 5.0 * rng.standard_normal(shape)).astype(np.float32)[None]
    prior = np.zeros((3,) + shape, np.float32)
    prior[0][truth == 0] = 1.0
    prior[1][truth == 1] = 1.0
    res = _seg.segment_em(y, None, prior, [1, 2, 3], prior_floor=0.0)
    assert res.model.dead.tolist() == [False, False, True] and 3 not in res.labels
    assert np.array_equal(res.labels, truth + 1)
    with pytest.raises(ValueError, match="every class is dead"):
        _seg.segment_em(y, np.zeros(shape, np.uint8), prior, [1, 2, 3])
    with pytest.raises(ValueError, match="every class is dead"):
        _seg.class_model(np.zeros((2, 3)), 1)
    for bad in (dict(beta=-1.0), dict(n_iter=0), dict(prior_floor=np.nan), dict(tol=-1e-3)):
        with pytest.raises(ValueError):
            _seg.segment_em(y, None, prior, [1, 2, 3], **bad)
    with pytest.raises(ValueError):
        _seg.segment_em(y, None, prior, [1, 2])  # K planes, K classes
    with pytest.raises(ValueError):
        _seg.segment_em(np.concatenate([y] * 5), None, prior, [1, 2, 3])  # 5 channels


# ---- benefit ---------------------------------------------------------------------------------------------------------------
# Measured with the defaults (seed 20): propagated 0.475 / 0.500 / 0.669 / 0.573 (mean 0.555), after EM 0.999 / 0.987 / 0.977 /
# 1.000 (mean 0.991).  The condition is the issue's: every class gains, the mean by more than 0.2.
def test_em_improves_on_the_propagated_labels_of_the_phantom():
    y, mask, truth, atlas = SC.phantom()
    cl = SC.PHANTOM_CLASSES
    before = SC.dice(SC.propagated_labels(atlas, mask, cl), truth, cl)
    res = _seg.segment_em(y, mask, _seg.priors_from_labels(atlas, cl, 2.0), cl)
    after = SC.dice(res.labels, truth, cl)
    print("Dice propagated", before.round(3), "after EM", after.round(3))
    assert np.all(after > before) and after.mean() - before.mean() > 0.2
    assert not res.labels[mask == 0].any() and res.n_iter == 15


# ---- plumbing --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from fetal_t2mapping_amd import build
    from fetal_t2mapping_amd._lib import load

    build.build()
    return load()


def test_abi_mirror_declares_the_seg_symbols_as_looked_up():
    names = [s[0] for s in _abi.SYMBOLS]
    assert len(_abi.SEG_SYMBOLS) == 7
    for sym in _abi.SEG_SYMBOLS:
        assert sym in names and sym in _abi.LOOKED_UP
    assert (_abi.SEG_MAX_CLASSES, _abi.SEG_MAX_CHANNELS, _abi.SEG_MAX_RADIUS) == (_seg.MAX_CLASSES, _seg.MAX_CHANNELS, _seg.MAX_RADIUS)


def test_workspace_arithmetic(lib):
    need = C.c_size_t(0)
    up = lambda v: (v + 255) // 256 * 256
    for shape in ((3, 5, 7), (1, 32, 32), (65, 64, 64), (256, 256, 256)):
        n = int(np.prod(shape))
        b = -(-n // 1024)
        for K, Cn in SC.CLASS_CHANNELS:
            Q = K * (1 + Cn + Cn * (Cn + 1) // 2)
            assert lib.t2fit_seg_workspace_bytes(K, Cn, *shape, C.byref(need)) == 0
            assert need.value == max(up(4 * K * n), up(8 * Q * b) + up(8 * Q * (-(-b // 256)))), (shape, K, Cn)


def test_every_refusal_comes_before_any_launch(lib):
    """Made-up pointers: a refusal touches none of them."""
    SC_check_refusals(lib)


def SC_check_refusals(lib, p=0x1000, q=0x2000, y=0x3000, m=0x4000, lab=0x5000, ws=0x10000, sums=0x20000, stream=None):
    def refused(rc, word):
        err = lib.t2fit_last_error().decode()
        assert rc == _abi.E_INVALID and word in err, (rc, word, err)

    need = C.c_size_t(0)
    cls = (C.c_int32 * 8)(*range(1, 9))
    live = (C.c_int32 * 8)(*([1] * 8))
    dead = (C.c_int32 * 8)()
    taps = (C.c_double * 65)(*([1.0 / 65] * 65))
    model = (C.c_double * 120)()
    V = C.c_void_p
    refused(lib.t2fit_seg_workspace_bytes(1, 1, 4, 4, 4, C.byref(need)), "n_class")
    refused(lib.t2fit_seg_workspace_bytes(9, 1, 4, 4, 4, C.byref(need)), "n_class")
    refused(lib.t2fit_seg_workspace_bytes(2, 0, 4, 4, 4, C.byref(need)), "n_chan")
    refused(lib.t2fit_seg_workspace_bytes(2, 5, 4, 4, 4, C.byref(need)), "n_chan")
    refused(lib.t2fit_seg_workspace_bytes(2, 1, 0, 4, 4, C.byref(need)), "nz")
    refused(lib.t2fit_seg_workspace_bytes(2, 1, 4, 4, 4, None), "bytes")
    refused(lib.t2fit_seg_mask_dev(None, V(m), 1, 64, V(m), stream), "y_dev")
    refused(lib.t2fit_seg_mask_dev(V(y), V(m), 5, 64, V(m), stream), "n_chan")
    refused(lib.t2fit_seg_mask_dev(V(y), V(m), 1, 0, V(m), stream), "n_vox")
    refused(lib.t2fit_seg_mask_dev(V(y + 2), V(m), 1, 64, V(m), stream), "aligned")
    pri = lambda **kw: lib.t2fit_seg_priors_dev(*[kw.get(k, d) for k, d in (
        ("labels", V(lab)), ("classes", cls), ("K", 3), ("nz", 4), ("ny", 4), ("nx", 4), ("tz", taps), ("rz", 2), ("ty", taps), ("ry", 2),
        ("tx", taps), ("rx", 2), ("out", V(p)), ("ws", V(ws)), ("stream", stream))])
    refused(pri(labels=None), "labels_dev")
    refused(pri(classes=None), "classes")
    refused(pri(tx=None), "taps_x")
    refused(pri(out=None), "prior_out_dev")
    refused(pri(ws=None), "workspace_dev")
    refused(pri(K=1), "n_class")
    refused(pri(ny=-1), "ny")
    refused(pri(rz=33), "rz")
    refused(pri(rx=-1), "rx")
    refused(pri(out=V(p + 1)), "aligned")
    refused(lib.t2fit_seg_normalise_dev(None, V(m), 3, 64, 1e-3, V(q), stream), "prior_dev")
    refused(lib.t2fit_seg_normalise_dev(V(p), None, 3, 64, 1e-3, V(q), stream), "mask_dev")
    refused(lib.t2fit_seg_normalise_dev(V(p), V(m), 3, 64, 1e-3, None, stream), "pi_out_dev")
    refused(lib.t2fit_seg_normalise_dev(V(p), V(m), 9, 64, 1e-3, V(q), stream), "n_class")
    refused(lib.t2fit_seg_normalise_dev(V(p), V(m), 3, 0, 1e-3, V(q), stream), "n_vox")
    refused(lib.t2fit_seg_normalise_dev(V(p), V(m), 3, 64, -1.0, V(q), stream), "floor")
    refused(lib.t2fit_seg_normalise_dev(V(p), V(m), 3, 64, float("nan"), V(q), stream), "floor")
    su = lambda **kw: lib.t2fit_seg_sums_dev(*[kw.get(k, d) for k, d in (
        ("p", V(p)), ("y", V(y)), ("m", V(m)), ("K", 3), ("C", 2), ("nz", 4), ("ny", 4), ("nx", 4), ("out", V(sums)), ("ws", V(ws)),
        ("stream", stream))])
    for name in ("p", "y", "m", "out", "ws"):
        refused(su(**{name: None}), "NULL")
    refused(su(K=0), "n_class")
    refused(su(C=5), "n_chan")
    refused(su(nx=0), "nx")
    refused(su(p=V(p + 2)), "4 bytes")
    refused(su(out=V(sums + 4)), "8 bytes")
    es = lambda **kw: lib.t2fit_seg_estep_dev(*[kw.get(k, d) for k, d in (
        ("po", V(p)), ("pi", V(q)), ("y", V(y)), ("m", V(m)), ("model", model), ("live", live), ("beta", 0.5), ("K", 3), ("C", 2),
        ("nz", 4), ("ny", 4), ("nx", 4), ("pn", V(p + 0x800)), ("stream", stream))])
    for name in ("po", "pi", "y", "m", "model", "live", "pn"):
        refused(es(**{name: None}), "NULL")
    refused(es(pn=V(p)), "p_new_dev must not be p_old_dev")
    refused(es(K=9), "n_class")
    refused(es(C=0), "n_chan")
    refused(es(nz=0), "nz")
    refused(es(beta=-0.5), "beta")
    refused(es(beta=float("inf")), "beta")
    refused(es(live=dead), "live")
    refused(es(pi=V(q + 1)), "aligned")
    refused(lib.t2fit_seg_labels_dev(None, V(m), cls, 3, 64, V(lab), stream), "p_dev")
    refused(lib.t2fit_seg_labels_dev(V(p), None, cls, 3, 64, V(lab), stream), "mask_dev")
    refused(lib.t2fit_seg_labels_dev(V(p), V(m), None, 3, 64, V(lab), stream), "classes")
    refused(lib.t2fit_seg_labels_dev(V(p), V(m), cls, 3, 64, None, stream), "labels_out_dev")
    refused(lib.t2fit_seg_labels_dev(V(p), V(m), cls, 1, 64, V(lab), stream), "n_class")
    refused(lib.t2fit_seg_labels_dev(V(p), V(m), cls, 3, -5, V(lab), stream), "n_vox")


def test_t2map_seg_names():
    from fetal_t2mapping_amd import t2map

    for name in ("segment_em", "priors_from_labels", "moment_sums", "e_step", "hard_labels", "seg_params"):
        assert callable(getattr(t2map.seg, name)), name
    import fetal_t2mapping_amd as pkg

    assert pkg.seg is t2map.seg and "seg" not in pkg.__all__
    assert t2map.seg.seg_params() == dict(sigma=2.0, beta=0.5, prior_floor=1e-3, var_floor=1e-6, n_iter=15, tol=0.0)


def test_recon_tissue_flags(tmp_path):
    from fetal_t2mapping_amd import cli, recon

    base = ["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo", "--lf"]
    template, ho, tis = (str(tmp_path / n) for n in ("t.nii.gz", "ho.nii.gz", "tissue.nii.gz"))
    for path in (template, ho, tis):
        open(path, "w").close()
    atlas = ["--atlas_labels", "--atlas_template", template, "--atlas", "ho=" + ho]
    a = recon.parse_arguments(base + atlas)
    assert a.tissue_atlas is None and a.tissue_args is None  # off by default
    a = recon.parse_arguments(base + atlas + ["--tissue_atlas", tis])
    assert a.tissue_args == {"path": tis, "classes": (1, 2, 3, 4, 5, 6, 7), "echoes": None, "sigma": None, "beta": None,
                             "n_iter": None, "write_prior": False}
    a = recon.parse_arguments(base + atlas + ["--tissue_atlas", tis, "--tissue_classes", "2,3", "--tissue_echoes", "114", "228",
                                              "--tissue_sigma", "1.5", "--tissue_beta", "0.25", "--tissue_iter", "5",
                                              "--write_tissue_prior"])
    assert a.tissue_args == {"path": tis, "classes": (2, 3), "echoes": [114, 228], "sigma": 1.5, "beta": 0.25, "n_iter": 5,
                             "write_prior": True}
    good = atlas + ["--tissue_atlas", tis]
    for bad in (["--tissue_atlas", tis],                                    # without --atlas_labels
                atlas + ["--tissue_atlas", str(tmp_path / "none.nii.gz")],  # a missing file
                good + ["--tissue_echoes", "1", "2", "3", "4", "5"],        # more than 4 echoes
                good + ["--tissue_echoes", "114", "114"],
                good + ["--tissue_classes", "2"],                           # fewer than 2 classes
                good + ["--tissue_classes", "1,x"], good + ["--tissue_classes", "1,1"], good + ["--tissue_classes", "0,1"],
                good + ["--tissue_sigma", "9"], good + ["--tissue_beta", "-1"], good + ["--tissue_iter", "0"],
                atlas + ["--tissue_beta", "0.5"], atlas + ["--write_tissue_prior"], atlas + ["--tissue_echoes", "114"]):
        with pytest.raises(SystemExit):
            recon.parse_arguments(base + bad)
    # an echo that was not reconstructed: known once the metadata is read, reported through the same p.error
    echoes = [(0.114, {"ax": "a"}), (0.228, {"ax": "b"})]
    assert recon.tissue_echo_rows(echoes, None) == [{"ax": "a"}] and recon.tissue_echo_rows(echoes, [228, 114]) == [{"ax": "b"}, {"ax": "a"}]
    with pytest.raises(ValueError, match="no echo of 300 ms"):
        recon.tissue_echo_rows(echoes, [114, 300])
    with pytest.raises(SystemExit):
        a.error("--tissue_echoes: no echo of 300 ms is reconstructed")
    # the reserved-name check stays, and the name is the one cli.py reads
    with pytest.raises(ValueError, match="another image's name"):
        recon.parse_atlas_spec("feta=" + tis)
    assert recon.feta_dirname is cli.feta_dirname and recon.tissue_prior_dirname == cli.feta_dirname + "_prior"


def _quick_atlas(**more):
    import atlas_cases as AC

    from fetal_t2mapping_amd import _atlas

    subject, template, g, mask, atlases, _ = AC.atlas_case()
    return _atlas.atlas_labels(subject, g, template, g, atlases, mask=mask, levels=(4,), max_iter=3, **more)


def test_atlas_labels_without_tissue_returns_what_it_returned_and_with_it_a_fourth_value():
    import atlas_cases as AC

    plain, none = _quick_atlas(), _quick_atlas(tissue=None)
    assert len(plain) == 3 and len(none) == 3
    assert np.array_equal(plain[0].view(np.uint32), none[0].view(np.uint32)) and np.array_equal(plain[2].transform, none[2].transform)
    assert all(np.array_equal(plain[1][n], none[1][n]) for n in plain[1]) and sorted(plain[1]) == sorted(none[1])
    subject, template, g, mask, atlases, _ = AC.atlas_case()
    classes = [int(v) for v in np.unique(atlases["ho"])[1:]]
    assert len(classes) >= 2
    out = _quick_atlas(tissue={"labels": atlases["ho"], "classes": classes, "channels": [subject, 0.7 * subject], "n_iter": 2, "sigma": 1.0})
    assert len(out) == 4 and np.array_equal(out[0].view(np.uint32), plain[0].view(np.uint32))
    t = out[3]
    assert np.array_equal(t["propagated"], plain[1]["ho"])  # the tissue atlas follows the transform like any other atlas
    assert t["labels"].dtype == np.int32 and t["labels"].shape == subject.shape and not t["labels"][mask == 0].any()
    assert set(np.unique(t["labels"])) <= {0, *classes} and t["n_iter"] == 2 and t["prior"].shape == (len(classes),) + subject.shape
    for bad in ({"labels": atlases["ho"]}, {"labels": atlases["ho"][1:], "classes": classes, "channels": subject},
                {"labels": atlases["ho"], "classes": classes, "channels": subject[1:]},
                {"labels": atlases["ho"], "classes": classes, "channels": subject, "betta": 1.0}):
        with pytest.raises(ValueError):
            _quick_atlas(tissue=bad)


def test_recon_writes_the_tissue_labels_where_the_roi_reader_opens_them(tmp_path, monkeypatch):
    import atlas_cases as AC
    import fake_sitk

    from fetal_t2mapping_amd import _atlas

    fake = fake_sitk.install()
    monkeypatch.setitem(sys.modules, "SimpleITK", fake)
    from fetal_t2mapping_amd import cli, recon

    bids, md, template_path, specs = AC.write_atlas_subject(tmp_path)
    seen = {}

    def statement(subject, sg, template, tg, atlases, *, mask, dof, bins, device, tissue=None):
        seen["channels"] = None if tissue is None else np.asarray(tissue["channels"]).shape
        return _atlas.atlas_labels(subject, sg, template, tg, atlases, mask=mask, dof=dof, bins=bins, levels=(4,), max_iter=3, tissue=tissue)

    monkeypatch.setattr(recon.t2map.atlas, "atlas_labels", statement)
    monkeypatch.setattr(recon.t2map.atlas, "extract_brain", lambda v, m: _atlas.extract_brain(v, m))
    ho_path = dict(specs)["ho"]
    classes = tuple(int(v) for v in np.unique(AC.atlas_case()[4]["ho"])[1:])
    tissue = {"path": ho_path, "classes": classes, "echoes": [114, 228], "sigma": 1.0, "beta": None, "n_iter": 2, "write_prior": True}
    written = recon.process_atlas_labels(md, bids, template_path, specs, dof=9, bins=16, tissue=tissue)
    assert len(written) == 7 and seen["channels"] == (2,) + AC.atlas_case()[0].shape
    anat = bids + "prj-901/derivatives/{0}/sub-001/ses-01/anat/sub-001_ses-01_te-114_{0}.nii.gz"
    feta, prior = fake.written[anat.format("recon_1mm_feta")], fake.written[anat.format("recon_1mm_feta_prior")]
    assert feta.arr.dtype == np.int32 and np.array_equal(prior.arr, fake.written[anat.format("recon_1mm_ho")].arr)
    path = anat.format("recon_1mm_feta")
    np.save(path + ".npy", feta.arr)
    open(path, "w").close()
    got = cli._read_label_image(fake, bids, [acq for _, acq in md.iterrows()], cli.feta_dirname)
    assert got is not None and np.array_equal(got, feta.arr)
    with pytest.raises(ValueError, match="no echo of 300 ms"):
        recon.process_atlas_labels(md, bids, template_path, specs, tissue=dict(tissue, echoes=[300]))
    shifted = str(tmp_path / "shifted.nii.gz")
    np.save(shifted + ".npy", AC.atlas_case()[4]["ho"][:, :, 1:])
    with pytest.raises(ValueError, match="template's grid"):
        recon.process_atlas_labels(md, bids, template_path, specs, tissue=dict(tissue, path=shifted))
