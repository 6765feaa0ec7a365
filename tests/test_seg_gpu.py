"""The tissue segmentation on the device (csrc/t2fit_seg.hip) against its numpy statement (fetal_t2mapping_amd/_seg.py):
priors, normalise, sums and labels bit for bit (the sums and labels on the device's own posteriors), the E-step within one
float32 ulp with exact zeros where the statement has them; the whole call against the shared loop driven with the device
steps; repeats, raw calls on a caller's stream with a poisoned workspace and offset pointers; the benefit phantom.
tests/test_seg_host.py holds the statement to an independent reference."""
import ctypes as C

import numpy as np
import pytest
import seg_cases as SC

from fetal_t2mapping_amd import _seg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def seg():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X")
    from fetal_t2mapping_amd import t2map

    return t2map.seg


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = int(np.sum(_bits(got) != _bits(want)))
    assert bad == 0, (what, bad)


def _model(p, y, mask, C_, dead_last):
    sums = _seg.moment_sums(p, y, mask)
    if dead_last:
        sums[-1] = 0.0
    return _seg.class_model(sums, C_, 1e-6)


def _check_steps(seg, shape, K, Cn, seed, *, mask=None, nan=True, dead=False, beta=0.5, sigma=1.0):
    classes, labels, y, m, p = SC.random_case(shape, K, Cn, seed, nan=nan, dead=dead)
    if mask is not None:
        m = mask
    what = (shape, K, Cn)
    _same(seg.priors_from_labels(labels, classes, sigma), _seg.priors_from_labels(labels, classes, sigma), what + ("priors",))
    M = seg.effective_mask(y, m)
    _same(M, _seg.effective_mask(y, m), what + ("mask",))
    prior = _seg.priors_from_labels(labels, classes, sigma)
    pi = seg.normalise_priors(prior, M, 1e-3)
    _same(pi, _seg.normalise_priors(prior, M, 1e-3), what + ("normalise",))
    if not M.any():
        return
    model = _model(p, y, m, Cn, dead)
    got = seg.e_step(p, pi, y, m, model, beta)
    want = _seg.e_step(p, pi, y, m, model, beta)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert SC.ulp_distance_f32(got, want).max() <= 1, what
    zero = _bits(want) == 0
    assert np.array_equal(_bits(got) == 0, zero), what  # +0.0 exactly where the statement has it, and nowhere else
    assert zero[:, M == 0].all() and (not dead or zero[-1].all())
    # the sums and the labels of the device's own posteriors
    _same(seg.moment_sums(got, y, m), _seg.moment_sums(got, y, m), what + ("sums",))
    _same(seg.hard_labels(got, classes, M), _seg.hard_labels(got, classes, M), what + ("labels",))


SHAPES = sorted(set(SC.ESTEP_SHAPES + SC.SUMS_SHAPES))


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
@pytest.mark.parametrize("kc", SC.CLASS_CHANNELS, ids=[f"K{k}C{c}" for k, c in SC.CLASS_CHANNELS])
def test_every_step_on_the_edge_shapes(seg, shape, kc):
    _check_steps(seg, shape, kc[0], kc[1], seed=11)


def test_masks_faces_an_isolated_voxel_a_dead_class_and_beta_zero(seg):
    shape = (5, 6, 66)
    _check_steps(seg, shape, 3, 2, 12, mask=np.ones(shape, np.uint8), nan=False)  # touches all six faces
    lone = np.zeros(shape, np.uint8)
    lone[2, 3, 40] = 1      # no neighbour in M
    lone[0:2, 0:2, 0:3] = 1  # and a corner block, so that the classes have mass
    _check_steps(seg, shape, 3, 2, 13, mask=lone, nan=False)
    _check_steps(seg, shape, 3, 2, 14, dead=True)
    _check_steps(seg, shape, 8, 4, 15, beta=0.0)
    _check_steps(seg, (4, 7, 9), 2, 1, 16, sigma=(0.0, 2.0, 0.6))
    _check_steps(seg, shape, 2, 1, 17, mask=np.zeros(shape, np.uint8), nan=False)  # an empty M: all zeros


def test_sums_with_a_second_reduce_pass(seg):
    shape = SC.TWO_PASS_SHAPE
    rng = np.random.default_rng(18)
    y = (100.0 + 20.0 * rng.standard_normal((1,) + shape)).astype(np.float32)
    p = rng.random((2,) + shape).astype(np.float32)
    mask = (rng.random(shape) < 0.7).astype(np.uint8)
    _same(seg.moment_sums(p, y, mask), _seg.moment_sums(p, y, mask), "two passes")


def _equal_results(a, b, what):
    _same(np.asarray(a.labels), np.asarray(b.labels), (what, "labels"))
    assert a.n_iter == b.n_iter, what
    _same(a.s0_trace, b.s0_trace, (what, "trace"))
    for name in ("mean", "cov", "precision", "logc"):
        _same(getattr(a.model, name), getattr(b.model, name), (what, name))
    assert np.array_equal(a.model.dead, b.model.dead)


@pytest.mark.parametrize("shape,K,Cn,kw", [((3, 5, 7), 2, 1, dict()), ((5, 5, 65), 3, 2, dict(beta=0.0, n_iter=4)),
                                           ((4, 9, 66), 8, 4, dict(n_iter=1)), ((6, 8, 33), 3, 2, dict(n_iter=40, tol=1e-3))],
                         ids=["3x5x7", "beta0", "one-iteration", "tol"])
def test_whole_call_equals_the_shared_loop_with_device_steps_and_repeats(seg, shape, K, Cn, kw):
    classes, labels, y, mask, _ = SC.random_case(shape, K, Cn, 19, nan=True, dead=(K == 3))
    prior = _seg.priors_from_labels(labels, classes, 1.0)
    got = seg.segment_em(y, mask, prior, classes, return_posteriors=True, **kw)
    want = _seg.segment_em(y, mask, prior, classes, steps=seg.DEVICE_STEPS, return_posteriors=True, **kw)
    _equal_results(got, want, shape)
    _same(got.posteriors, want.posteriors, (shape, "posteriors"))
    _equal_results(seg.segment_em(y, mask, prior, classes, **kw), got, (shape, "repeat"))
    if K == 3 and Cn == 2 and "tol" not in kw:
        assert got.model.dead.tolist() == [False, False, True]
    if "tol" in kw:
        assert got.n_iter < kw["n_iter"]
    # and it is the statement's segmentation up to the last bits of exp
    ref = _seg.segment_em(y, mask, prior, classes, **kw)
    assert np.mean(got.labels == ref.labels) >= 0.999 and got.n_iter == ref.n_iter


def test_tensors_in_tensors_out(seg):
    import torch

    classes, labels, y, mask, _ = SC.random_case((4, 6, 70), 3, 2, 20)
    dev = torch.device("cuda", 0)
    prior = seg.priors_from_labels(torch.from_numpy(labels).to(dev), classes, 1.0)
    assert torch.is_tensor(prior) and prior.is_cuda
    res = seg.segment_em(torch.from_numpy(y).to(dev), torch.from_numpy(mask).to(dev), prior, classes, n_iter=3)
    assert torch.is_tensor(res.labels) and res.labels.dtype == torch.int32
    host = seg.segment_em(y, mask, prior.cpu().numpy(), classes, n_iter=3)
    assert np.array_equal(res.labels.cpu().numpy(), host.labels)
    with pytest.raises(ValueError, match="p_new_dev must not be p_old_dev"):
        p = prior.clone()
        seg.e_step(p, prior, torch.from_numpy(y).to(dev), None, host.model, 0.5, out=p)


def test_raw_calls_on_a_callers_stream_with_a_poisoned_workspace_and_offset_pointers(seg):
    """ctypes calls on a caller's stream; the workspace is all NaN before each call; every float buffer starts 4 bytes past
    a 256-byte boundary and nx is no multiple of 4.  The bits are those of the binding's calls."""
    import torch

    from fetal_t2mapping_amd._lib import load

    lib = load()
    shape, K, Cn = (5, 6, 67), 3, 2
    n = int(np.prod(shape))
    classes, labels, y, mask, p = SC.random_case(shape, K, Cn, 21, nan=True)
    M = seg.effective_mask(y, mask)
    prior = seg.priors_from_labels(labels, classes, 1.0)
    pi = seg.normalise_priors(prior, M, 1e-3)
    model = _model(p, y, mask, Cn, False)
    rows, live = _seg.pack_model(model)
    want_p = seg.e_step(p, pi, y, mask, model, 0.5)
    want_sums = seg.moment_sums(want_p, y, mask)
    want_lab = seg.hard_labels(want_p, classes, M)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)

    def off(arr, dtype=torch.float32):  # a device copy that starts one element past an aligned address
        buf = torch.empty(arr.size + 1, dtype=dtype, device=dev)
        buf[1:] = torch.from_numpy(np.ascontiguousarray(arr).reshape(-1)).to(dev)
        return buf, buf[1:]

    need = C.c_size_t(0)
    assert lib.t2fit_seg_workspace_bytes(K, Cn, *shape, C.byref(need)) == 0
    ws = torch.empty(need.value // 8 + 32, dtype=torch.float64, device=dev)
    ws_ptr = (ws.data_ptr() + 255) // 256 * 256
    cls = (C.c_int32 * K)(*classes.tolist())
    taps = _seg.gauss_taps(1.0)
    tp = taps.ctypes.data_as(C.POINTER(C.c_double))
    keep = [off(labels, torch.int32), off(y), off(p), off(pi)]
    (_, lab_d), (_, y_d), (_, p_d), (_, pi_d) = keep
    m_d = torch.from_numpy(M).to(dev).reshape(-1)
    raw_mask_d = torch.from_numpy(mask).to(dev)
    out_prior = torch.empty(K * n + 1, dtype=torch.float32, device=dev)
    out_p = torch.empty(K * n + 1, dtype=torch.float32, device=dev)
    out_pi = torch.empty(K * n + 1, dtype=torch.float32, device=dev)
    out_m = torch.empty(n, dtype=torch.uint8, device=dev)
    out_sums = torch.empty(K * 6, dtype=torch.float64, device=dev)
    out_lab = torch.empty(n + 1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for _ in range(2):
            ws.fill_(float("nan"))
            assert lib.t2fit_seg_mask_dev(y_d.data_ptr(), raw_mask_d.data_ptr(), Cn, n, out_m.data_ptr(), st) == 0
            assert lib.t2fit_seg_priors_dev(lab_d.data_ptr(), cls, K, *shape, tp, 4, tp, 4, tp, 4, out_prior[1:].data_ptr(), ws_ptr, st) == 0
            assert lib.t2fit_seg_normalise_dev(out_prior[1:].data_ptr(), m_d.data_ptr(), K, n, 1e-3, out_pi[1:].data_ptr(), st) == 0
            assert lib.t2fit_seg_estep_dev(p_d.data_ptr(), pi_d.data_ptr(), y_d.data_ptr(), m_d.data_ptr(),
                                           rows.ctypes.data_as(C.POINTER(C.c_double)), live.ctypes.data_as(C.POINTER(C.c_int32)), 0.5, K, Cn,
                                           *shape, out_p[1:].data_ptr(), st) == 0
            ws.fill_(float("nan"))
            assert lib.t2fit_seg_sums_dev(out_p[1:].data_ptr(), y_d.data_ptr(), m_d.data_ptr(), K, Cn, *shape, out_sums.data_ptr(), ws_ptr,
                                          st) == 0
            assert lib.t2fit_seg_labels_dev(out_p[1:].data_ptr(), m_d.data_ptr(), cls, K, n, out_lab[1:].data_ptr(), st) == 0
            stream.synchronize()
            _same(out_m.cpu().numpy().reshape(shape), M, "raw mask")
            _same(out_prior[1:].cpu().numpy().reshape((K,) + shape), prior, "raw priors")
            _same(out_pi[1:].cpu().numpy().reshape((K,) + shape), pi, "raw normalise")
            _same(out_p[1:].cpu().numpy().reshape((K,) + shape), want_p, "raw estep")
            _same(out_sums.cpu().numpy().reshape(K, 6), want_sums, "raw sums")
            _same(out_lab[1:].cpu().numpy().reshape(shape), want_lab, "raw labels")


def test_the_benefit_phantom_through_the_device(seg):
    y, mask, truth, atlas = SC.phantom()
    cl = SC.PHANTOM_CLASSES
    before = SC.dice(SC.propagated_labels(atlas, mask, cl), truth, cl)
    res = seg.segment_em(y, mask, seg.priors_from_labels(atlas, cl), cl)
    after = SC.dice(res.labels, truth, cl)
    print("Dice propagated", before.round(3), "after EM on the device", after.round(3))
    assert np.all(after > before) and after.mean() - before.mean() > 0.2
    assert res.n_iter == 15 and not res.labels[mask == 0].any()


def test_atlas_labels_with_a_tissue_atlas_on_the_device():
    import atlas_cases as AC

    from fetal_t2mapping_amd import _atlas, t2map

    subject, template, g, mask, atlases, _ = AC.atlas_case()
    classes = [int(v) for v in np.unique(atlases["ho"])[1:]]
    kw = dict(mask=mask, levels=(4,), max_iter=3)
    tissue = {"labels": atlases["ho"], "classes": classes, "channels": [subject, 0.7 * subject], "n_iter": 3}
    plain = t2map.atlas.atlas_labels(subject, g, template, g, atlases, **kw)
    none = t2map.atlas.atlas_labels(subject, g, template, g, atlases, tissue=None, **kw)
    out = t2map.atlas.atlas_labels(subject, g, template, g, atlases, tissue=tissue, **kw)
    assert len(plain) == 3 and len(none) == 3 and len(out) == 4
    for a, b in ((plain, none), (plain, out)):
        assert a[0].tobytes() == b[0].tobytes() and all(a[1][k].tobytes() == b[1][k].tobytes() for k in a[1])
    t = out[3]
    assert np.array_equal(t["propagated"], plain[1]["ho"]) and t["labels"].dtype == np.int32 and not t["labels"][mask == 0].any()
    want = _atlas.atlas_labels(subject, g, template, g, atlases, tissue=tissue, **kw)[3]
    if np.array_equal(want["propagated"], t["propagated"]):
        assert np.mean(want["labels"] == t["labels"]) >= 0.999
