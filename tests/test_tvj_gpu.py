"""The vector-valued (joint) TV denoiser on the device (csrc/t2fit_denoise.hip: tvj_pass_kernel, tvj_finish_kernel) against
its numpy statement (fetal_t2mapping_amd/_tv.py: tv_joint_problem): bit for bit at fixed iteration counts over the shapes of
tests/tvj_cases.py, C = 1 against the scalar kernel, iteration counts under the stop rule, a NaN that stays in its problem,
raw calls (in place, offset buffers, a caller's stream, a poisoned workspace, NULL outputs, repeats), slice groups, the
unchanged default path, the CLI and the joint prox of the super-resolution loop.  tests/test_tvj_host.py holds the
statement to an independent reference."""
import ctypes as C
import os

import numpy as np
import pytest

import denoise_cases as D
import tvj_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def t2():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X")
    import fetal_t2mapping_amd as t2

    return t2


TABLE = [(shape, dims, precision) for precision in ("f32", "f64") for dims in (2, 3) for shape in K.GPU_SHAPES]


@pytest.mark.parametrize("shape,dims,precision", TABLE, ids=[f"{p}-{d}d-" + "x".join(map(str, s)) for s, d, p in TABLE])
def test_fixed_iteration_count_is_bit_equal_to_the_numpy_statement(t2, shape, dims, precision):
    """1, 2 and 7 iterations: the first pass, and a result in either half of the ping-pong pair."""
    a = np.array(K.gpu_stack(shape))
    n_problems = shape[1] if dims == 2 else 1
    for max_iter in K.GPU_ITERS:
        want, want_n, want_e = K.gpu_want(shape, dims, precision, max_iter)
        got, info = t2.denoise_tv(a, K.WEIGHT, eps=0.0, max_iter=max_iter, dims=dims, precision=precision, return_info=True,
                                  joint=True)
        assert got.dtype == np.float32 and got.shape == a.shape and info["n_iter"].shape == (n_problems,)
        assert np.array_equal(info["n_iter"], want_n) and np.all(want_n == max_iter - 1)
        bad = int(np.sum(got.view(np.uint32) != want.view(np.uint32)))
        assert bad == 0, (shape, dims, precision, max_iter, bad, float(np.abs(got - want).max()))
        assert np.allclose(info["energy"], want_e, rtol=1e-12, atol=0.0)
        if shape[0] == 1:  # one channel: the scalar kernel's bytes, n_iter and energy
            one, oinfo = t2.denoise_tv(a, K.WEIGHT, eps=0.0, max_iter=max_iter, dims=dims, precision=precision, return_info=True)
            assert one.tobytes() == got.tobytes() and np.array_equal(oinfo["n_iter"], info["n_iter"])
            assert np.allclose(oinfo["energy"], info["energy"], rtol=1e-12, atol=0.0)


STOP_SHAPE, STOP_WEIGHTS = (3, 6, 40, 72), (10.0, 20.0, 40.0)


def _stop_stack():
    """Three echoes of the picture of denoise_cases (another disc in every slice), decaying, under its Rician noise."""
    a = D.picture((3,) + STOP_SHAPE[1:], seed=5)[0]
    return (a * np.exp(-0.3 * np.arange(3))[:, None, None, None]).astype(np.float32)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_stop_rule_gives_the_iteration_counts_of_the_numpy_statement(t2, precision):
    """dims = 2: the slices stop at different iterations.  Every iteration of every problem is at least 1e-9 E_init away
    from the threshold by the statement (the kernel's sums differ from np.sum by ~1e-12), asserted before the device runs."""
    from fetal_t2mapping_amd import _tv

    a = _stop_stack()
    for weight in STOP_WEIGHTS:
        margin = np.inf
        for z in range(a.shape[1]):
            hist = []
            _tv.tv_joint_problem(a[:, z], weight, 2e-4, 200, K.DTYPE[precision], history=hist)
            e_prev = hist[0]
            for e in hist[1:]:
                margin = min(margin, abs(abs(e_prev - e) - 2e-4 * hist[0]) / hist[0])
                e_prev = e
        assert margin >= D.STOP_MARGIN, (weight, margin)
        want, want_n, want_e = _tv.denoise_tv_joint(a, weight, 2e-4, 200, 2, precision)
        got, info = t2.denoise_tv(a, weight, dims=2, precision=precision, return_info=True, joint=True)
        print(f"{precision} weight {weight}: n_iter {want_n.tolist()}, margin {margin:.3g}")
        assert np.array_equal(info["n_iter"], want_n), (weight, info["n_iter"], want_n)
        assert got.tobytes() == want.tobytes() and np.allclose(info["energy"], want_e, rtol=1e-12, atol=0.0)
        assert np.all(want_n > 1) and np.all(want_n < 199)
    assert len(set(want_n.tolist())) > 1  # (at the last weight the slices stop at different iterations)
    # the whole stack as one problem stops as the statement's one problem does
    want, want_n, want_e = _tv.denoise_tv_joint(a, 20.0, 2e-4, 200, 3, precision)
    got, info = t2.denoise_tv(a, 20.0, dims=3, precision=precision, return_info=True, joint=True)
    assert info["n_iter"].tolist() == want_n.tolist() and 1 < want_n[0] < 199 and got.tobytes() == want.tobytes()


def test_a_nan_in_one_channel_reaches_every_channel_of_its_slice_and_no_other(t2):
    a = _stop_stack()
    clean, cinfo = t2.denoise_tv(a, 20.0, dims=2, return_info=True, joint=True)
    b = a.copy()
    b[1, 3, 17, 40] = np.nan
    got, info = t2.denoise_tv(b, 20.0, dims=2, return_info=True, joint=True)
    assert np.isnan(got[:, 3]).all(axis=(1, 2)).all()  # 199 iterations carry it across the 40 x 72 slice of all channels
    assert info["n_iter"][3] == 199 and np.isnan(info["energy"][3])
    keep = [z for z in range(a.shape[1]) if z != 3]
    assert got[:, keep].tobytes() == clean[:, keep].tobytes() and np.isfinite(got[:, keep]).all()
    assert np.array_equal(info["n_iter"][keep], cinfo["n_iter"][keep])
    # a few iterations: the NaN has reached the other channels at the same voxels, and only those
    few = t2.denoise_tv(b, 20.0, eps=0.0, max_iter=4, dims=2, joint=True)
    assert np.isnan(few[0, 3, 17, 40]) and np.isnan(few[2, 3, 17, 40]) and not np.isnan(few[:, 3]).all()
    assert np.array_equal(np.isnan(few[0]), np.isnan(few[2]))


@pytest.mark.parametrize("dims", [2, 3])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_raw_calls_on_another_stream_poisoned_workspace_and_offset_buffers(t2, dims, precision):
    """ctypes calls on a caller's stream, the workspace all 0xFF before each call, nx % 4 == 0: (a) in and out 4 bytes past
    a 256-byte boundary, (b) only out, (c) only in, (d) in place 4 bytes past, (e) aligned and in place, (f) aligned with
    n_iter_dev and energy_dev NULL, three times over.  Every result bit-equal to the statement, at an even and an odd
    n_iter; the words around every buffer keep their bytes."""
    import torch

    from fetal_t2mapping_amd import _abi, _tv
    from fetal_t2mapping_amd._lib import load

    lib = load()
    shape = (3, 3, 9, 68)
    a = K.field(shape, seed=68)
    n, pad, guard = a.size, 64, 0x5A5A5A5A
    n_problems = shape[1] if dims == 2 else 1
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)

    def buffer(shift):
        buf = torch.full((n + 3 * pad,), guard, dtype=torch.int32, device="cuda")
        assert buf.data_ptr() % 256 == 0
        view = buf[pad + shift:pad + shift + n].view(torch.float32)
        assert view.data_ptr() % 256 == 4 * shift
        return buf, view

    def guards_kept(buf, shift):
        host = buf.cpu().numpy()
        return bool(np.all(host[:pad + shift] == guard) and np.all(host[pad + shift + n:] == guard))

    for max_iter in (7, 8):
        par = _abi.T2FitTvParams()
        assert lib.t2fit_tv_params_default(C.byref(par)) == _abi.OK
        par.weight, par.eps, par.max_iter, par.dims, par.precision = 12.0, 0.0, max_iter, dims, _abi.PRECISIONS[precision]
        want, want_n, want_e = _tv.denoise_tv_joint(a, 12.0, 0.0, max_iter, dims, precision)
        need = C.c_size_t()
        assert lib.t2fit_tv_joint_workspace_bytes(C.byref(par), *shape, C.byref(need)) == _abi.OK
        for name, in_shift, out_shift, in_place, with_info in (("a", 1, 1, False, True), ("b", 0, 1, False, True),
                                                               ("c", 1, 0, False, True), ("d", 1, 1, True, True),
                                                               ("e", 0, 0, True, True), ("f", 0, 0, False, False),
                                                               ("f", 0, 0, False, False), ("f", 0, 0, False, False)):
            with torch.cuda.stream(stream):
                ws = torch.empty(need.value + 256, dtype=torch.uint8, device="cuda")
                ws.fill_(0xFF)
                ws_ptr = (ws.data_ptr() + 255) // 256 * 256
                src_buf, src = buffer(in_shift)
                src.copy_(torch.from_numpy(a.reshape(-1)))
                dst_buf, dst = (src_buf, src) if in_place else buffer(out_shift)
                n_iter = torch.full((n_problems,), -1, dtype=torch.int32, device="cuda")
                energy = torch.full((n_problems,), -1.0, dtype=torch.float64, device="cuda")
                rc = lib.t2fit_tv_joint_denoise_dev(C.byref(par), src.data_ptr(), dst.data_ptr(), *shape, ws_ptr, need.value,
                                                    n_iter.data_ptr() if with_info else None,
                                                    energy.data_ptr() if with_info else None, st)
                assert rc == _abi.OK, (name, lib.t2fit_last_error())
                stream.synchronize()
            what = (name, dims, precision, max_iter)
            assert dst.cpu().numpy().tobytes() == want.tobytes(), what
            assert guards_kept(dst_buf, out_shift), what
            if not in_place:
                assert src.cpu().numpy().tobytes() == a.tobytes() and guards_kept(src_buf, in_shift), what
            if with_info:
                assert np.array_equal(n_iter.cpu().numpy(), want_n) and np.all(want_n == max_iter - 1), what
                assert np.allclose(energy.cpu().numpy(), want_e, rtol=1e-12, atol=0.0), what
            else:
                assert np.all(n_iter.cpu().numpy() == -1) and np.all(energy.cpu().numpy() == -1.0), what


def test_wrapper_entries_slice_groups_and_the_refusals(t2, monkeypatch):
    import torch

    from fetal_t2mapping_amd import _abi, _tv
    from fetal_t2mapping_amd._gpu_tv import tv_params
    from fetal_t2mapping_amd._lib import load

    lib = load()
    shape = (3, 5, 9, 12)
    a = K.field(shape, seed=5)
    want, want_n, want_e = _tv.denoise_tv_joint(a, 15.0, 2e-4, 200, 2, "f32")
    got, info = t2.denoise_tv(a, 15.0, return_info=True, joint=True)
    assert got.tobytes() == want.tobytes() and np.array_equal(info["n_iter"], want_n)
    # tensor entry, out of place and in place
    t = torch.from_numpy(a).cuda()
    res, tinfo = t2.denoise_tv(t, 15.0, return_info=True, joint=True)
    assert res.is_cuda and res.data_ptr() != t.data_ptr() and torch.equal(t.cpu(), torch.from_numpy(a))
    assert res.cpu().numpy().tobytes() == want.tobytes() and np.array_equal(tinfo["n_iter"].cpu().numpy(), want_n)
    same = t2.denoise_tv(t, 15.0, out=t, joint=True)
    assert same.data_ptr() == t.data_ptr() and t.cpu().numpy().tobytes() == want.tobytes()
    # slices in groups of 3 and 2 under a budget that fits exactly three; a joint problem is never split across channels
    par = tv_params(15.0)

    def need(nz):
        v = C.c_size_t()
        assert lib.t2fit_tv_joint_workspace_bytes(C.byref(par), shape[0], nz, *shape[2:], C.byref(v)) == _abi.OK
        return v.value

    budget = need(3)
    assert need(5) > budget and need(4) > budget
    real, calls = lib.t2fit_tv_joint_denoise_dev, []

    def spy(*args):
        calls.append((int(args[3]), int(args[4]), int(args[8])))
        return real(*args)

    monkeypatch.setattr(lib, "t2fit_tv_joint_denoise_dev", spy)
    grouped, ginfo = t2.denoise_tv(a, 15.0, return_info=True, joint=True, max_workspace_bytes=budget)
    assert calls == [(3, 3, budget), (3, 2, budget)]
    assert grouped.tobytes() == want.tobytes() and np.array_equal(ginfo["n_iter"], want_n)
    assert np.allclose(ginfo["energy"], want_e, rtol=1e-12, atol=0.0)
    with pytest.raises(ValueError, match="cannot be split"):
        t2.denoise_tv(a, 15.0, dims=3, joint=True, max_workspace_bytes=budget)
    with pytest.raises(ValueError, match=r"\(C, Z, Y, X\)"):
        t2.denoise_tv(a[0], 15.0, joint=True)
    with pytest.raises(ValueError, match="T2FIT_TV_JOINT_MAX_CHAN"):
        t2.denoise_tv(np.zeros((K.MAX_CHAN + 1, 1, 2, 2), np.float32), 15.0, joint=True)


def test_the_default_path_is_unchanged(t2, monkeypatch):
    """joint=False (given or not) is the scalar statement's bytes and calls the scalar entry point only."""
    from fetal_t2mapping_amd import _tv
    from fetal_t2mapping_amd._lib import load

    lib = load()
    a = np.array(K.gpu_stack((3, 5, 33, 65)))
    real, joint_calls = lib.t2fit_tv_joint_denoise_dev, []
    monkeypatch.setattr(lib, "t2fit_tv_joint_denoise_dev", lambda *args: joint_calls.append(1) or real(*args))
    for dims in (2, 3):
        want, want_n, _ = _tv.denoise_tv(a, 20.0, 2e-4, 200, dims, "f32")
        for kw in ({}, {"joint": False}):
            got, info = t2.denoise_tv(a, 20.0, dims=dims, return_info=True, **kw)
            assert got.tobytes() == want.tobytes() and np.array_equal(info["n_iter"], want_n)
        joint = t2.denoise_tv(a, 20.0, dims=dims, joint=True)
        assert joint.tobytes() != want.tobytes()
    assert len(joint_calls) == 2


def test_cli_denoises_jointly_ahead_of_the_fit(t2, tmp_path, monkeypatch, capsys):
    import sys

    from test_denoise_gpu import _tree

    from fetal_t2mapping_amd import _tv
    from fetal_t2mapping_amd import cli as R
    from fetal_t2mapping_amd import nifti

    monkeypatch.setitem(sys.modules, "SimpleITK", None)
    root0, out0, echoes, mask, te = _tree(tmp_path / "tv")
    base = ["--csv", "log.csv", "--in_vivo", "--gaussian", "--lf", "--sim", "d1", "--TEs"] + [str(int(t)) for t in te]
    R.main(["--path", root0] + base + ["--denoise", "tv", "--denoise_weight", "1sigma"])
    capsys.readouterr()
    root1, out1, _, _, _ = _tree(tmp_path / "joint")
    R.main(["--path", root1] + base + ["--denoise", "tv_joint", "--denoise_weight", "1sigma"])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Denoising:")]
    assert len(line) == 1 and "joint across the echoes" in line[0] and "10 problems" in line[0]
    name = [f for f in os.listdir(out0) if "t2map" in f][0]
    tv = nifti.ReadImage(os.path.join(out0, name)).arr
    joint = nifti.ReadImage(os.path.join(out1, name)).arr
    assert sorted(os.listdir(out0)) == sorted(os.listdir(out1)) and not np.array_equal(tv, joint)
    sigma, _ = t2.estimate_background_sigma(echoes, mask)
    den = _tv.denoise_tv_joint(echoes, sigma, 2e-4, 200, 2, "f32")[0]
    assert t2.denoise_tv(echoes, sigma, joint=True).tobytes() == den.tobytes()
    fit = t2.fit_volume(den, mask, te, "gaussian", t2.fit_table("gaussian", True))
    assert np.array_equal(joint, fit.t2)


def test_one_super_resolution_iteration_with_the_joint_prox_is_bit_equal_to_the_statement(t2):
    from test_recon_gpu import _phantom_stacks

    from fetal_t2mapping_amd import _sr

    stacks, geoms = _phantom_stacks(n_te=3, side=16, thick=4.0)[:2]
    kw = dict(weight=20.0, n_iter=1, prox_iter=5)
    want, _ = _sr.reconstruct_sr(stacks, geoms, tv="joint", **kw)
    got, _ = t2.sr.reconstruct_sr(stacks, geoms, tv="joint", **kw)
    chan, _ = t2.sr.reconstruct_sr(stacks, geoms, **kw)
    got, chan = got.cpu().numpy(), chan.cpu().numpy()
    assert got.shape == want.shape == (3, 16, 16, 16)
    assert got.tobytes() == want.tobytes() and got.tobytes() != chan.tobytes()
    assert chan.tobytes() == _sr.reconstruct_sr(stacks, geoms, **kw)[0].tobytes()
    with pytest.raises(ValueError, match="tv must be"):
        t2.sr.reconstruct_sr(stacks, geoms, tv="both", **kw)
