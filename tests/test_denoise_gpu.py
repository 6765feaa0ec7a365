"""The TV-Chambolle denoiser on the device (csrc/t2fit_denoise.hip) against its numpy statement (fetal_t2mapping_amd/_tv.py):
bit for bit at a fixed iteration count over the table of edge shapes of tests/denoise_cases.py, the exact 1-D minimiser,
iteration counts under the stop rule, independence of the problems of one call, in-place / repeat / entry-point
identities, raw calls with unaligned buffers on a caller's stream, groups of volumes, a whole-size stack, and the step
inside the fit pipeline and the CLI.  tests/test_denoise_host.py holds the statement to the independent references and
covers the argument checks and the flags without a device."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import denoise_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def t2():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X")
    import fetal_t2mapping_amd as t2

    return t2


_stack = K.picture
SIZES = [(2, 1, 64, 64), (2, 5, 37, 53), (1, 3, 256, 256), (2, 16, 17, 1)]
assert [shape for shape, _, _ in K.SHAPES[:4]] == SIZES  # the table keeps the first four as they were, with _stack(seed=11)
TABLE = [(shape, dims, precision) for precision in ("f32", "f64") for dims in (2, 3) for shape, dim_list, _ in K.SHAPES
         if dims in dim_list]


@pytest.mark.parametrize("shape,dims,precision", TABLE, ids=[f"{p}-{d}-" + "x".join(map(str, s)) for s, d, p in TABLE])
def test_fixed_iteration_count_is_bit_equal_to_the_numpy_statement(t2, shape, dims, precision):
    """Every entry of denoise_cases.SHAPES (each names the branch of the kernels it reaches)."""
    from fetal_t2mapping_amd import _tv

    a = np.array(K.stack(shape))  # (the shared case is read-only)
    if shape in SIZES:
        assert np.array_equal(a, _stack(shape, seed=11)[0])
    if shape == (1, 1, 1025, 65):
        assert K.tiles(shape, dims) == 66
    if shape == (2, 33, 57, 5):
        assert 65 <= K.tiles(shape, dims) <= 127 and K.tiles(shape, dims) % 64 != 0
    for max_iter in (1, 2, 7, 40):
        want, want_n, want_e = _tv.denoise_tv(a, 25.0, 0.0, max_iter, dims, precision)
        got, info = t2.denoise_tv(a, 25.0, eps=0.0, max_iter=max_iter, dims=dims, precision=precision, return_info=True)
        assert got.dtype == np.float32 and got.shape == a.shape
        assert np.array_equal(info["n_iter"], want_n) and np.all(want_n == max_iter - 1)
        bad = int(np.sum(got.view(np.uint32) != want.view(np.uint32)))
        assert bad == 0, (shape, dims, precision, max_iter, bad, float(np.abs(got - want).max()))
        assert np.allclose(info["energy"], want_e, rtol=1e-12, atol=0.0)
        if a.size == 1:  # one voxel: E = 0 at every iteration, the loop runs out, out == f
            assert np.array_equal(got, a) and info["energy"][0] == 0.0
    if a.size == 1:  # .. under the default eps as well: 0 < eps * 0 never holds
        got, info = t2.denoise_tv(a, 25.0, dims=dims, precision=precision, return_info=True)
        assert np.array_equal(got, a) and info["n_iter"].tolist() == [199] and info["energy"][0] == 0.0


@pytest.mark.parametrize("n,weight", K.ONE_D, ids=[f"n{n}-w{w:g}" for n, w in K.ONE_D])
def test_one_dimensional_problems_reach_the_exact_minimiser(t2, n, weight):
    """A column, a row and a 3-D line after K iterations with eps = 0 against the exact minimiser of 1-D total variation
    (denoise_cases.exact_1d: bounded least squares on the dual, no Chambolle).  float64: within the float64 statement's
    own distance plus half a float32 ulp of the output for the final rounding; float32: within twice the float32
    statement's distance.  The bars come from the statement on the CPU, never from the device."""
    f, u = K.exact_1d(n, weight)
    for form, (dims, shape) in K.ONE_D_FORMS.items():
        _, dist64 = K.statement_1d(n, weight, form, K.K, "f64")
        assert dist64 <= 1e-6, (form, dist64)  # the reference is converged before the device is looked at
        _, dist32 = K.statement_1d(n, weight, form, K.K, "f32")
        assert 0.0 < dist32 <= K.STATEMENT_DISTANCE["f32"]
        a = np.array(f).reshape(shape(n))
        for precision in ("f64", "f32"):
            t0 = time.perf_counter()
            got, info = t2.denoise_tv(a, weight, eps=0.0, max_iter=K.K, dims=dims, precision=precision, return_info=True)
            dt = time.perf_counter() - t0
            assert info["n_iter"].tolist() == [K.K - 1]
            err = np.abs(got.reshape(-1).astype(np.float64) - u)
            bar = dist64 + 0.5 * np.spacing(np.abs(got.reshape(-1))).astype(np.float64) if precision == "f64" else 2.0 * dist32
            print(f"n {n} weight {weight} {form} {precision}: max |device - exact| {err.max():.3g}, statement f64 {dist64:.3g} "
                  f"f32 {dist32:.3g}, {K.K} iterations in {dt:.3f} s")
            assert np.all(err <= bar), (form, precision, float(err.max()), float(np.max(bar)))


@pytest.mark.parametrize("dims,precision", [(2, "f32"), (2, "f64"), (3, "f32"), (3, "f64")])
def test_stop_rule_gives_the_iteration_counts_of_the_numpy_statement(t2, dims, precision):
    from fetal_t2mapping_amd import _tv

    a, _ = _stack((2, 6, 96, 80), seed=5)
    # the picture, and an entry of the table with several x tiles and a ragged quad; test_denoise_host.py keeps every
    # iteration of every problem of both at least 1e-9 E_init away from the threshold
    b = np.array(K.stop_stacks()[1])
    assert np.array_equal(K.stop_stacks()[0], a) and b.shape[-1] > 64 and b.shape[-1] % 4 != 0
    assert K.STOP_WEIGHTS == (0.1, 10.0, 20.0, 40.0)
    for stack in (a, b):
        for weight in (0.1, 10.0, 20.0, 40.0):
            want, want_n, want_e = _tv.denoise_tv(stack, weight, 2e-4, 200, dims, precision)
            got, info = t2.denoise_tv(stack, weight, dims=dims, precision=precision, return_info=True)
            diff = np.flatnonzero(info["n_iter"] != want_n)
            for k in diff:  # the bar is none; a marginal stop (|E_prev - E| within float64 rounding of the threshold) would show here
                print(f"problem {k}: n_iter {info['n_iter'][k]} vs {want_n[k]}, E {info['energy'][k]!r} vs {want_e[k]!r}")
            assert diff.size == 0, (weight, diff, info["n_iter"][diff], want_n[diff])
            assert got.tobytes() == want.tobytes(), weight
            assert np.allclose(info["energy"], want_e, rtol=1e-12, atol=0.0)
            print(f"{stack.shape} dims {dims} {precision} weight {weight}: n_iter min {want_n.min()} mean {want_n.mean():.1f} "
                  f"max {want_n.max()}")
    assert np.all(_tv.denoise_tv(a, 0.1, 2e-4, 200, 2, "f32")[1] == 1)  # the reference's setting: one update


def test_problems_of_one_call_are_independent(t2):
    import torch

    a, _ = _stack((1, 4, 64, 96), seed=3)
    a[0, 1] = 700.0  # a flat slice: E = 0 throughout, |E_prev - E| < eps * 0 never holds, it runs to the limit unchanged
    a[0, 3, 10, 20] = np.nan  # never stops, stays in its slice
    a[0, 3, 40, 50] = np.inf
    got, info = t2.denoise_tv(a, 20.0, return_info=True)
    assert info["n_iter"][1] == 199 and info["n_iter"][3] == 199 and 1 < info["n_iter"][0] < 199
    assert np.all(got[0, 1] == 700.0) and np.isfinite(got[0, :3]).all() and not np.isfinite(got[0, 3]).all()
    for k in range(4):
        alone, one = t2.denoise_tv(a[:, k:k + 1], 20.0, return_info=True)
        assert alone.tobytes() == got[:, k:k + 1].tobytes() and one["n_iter"][0] == info["n_iter"][k], k
    # in place, twice, tensor entry, grouped volumes: the same bytes
    b, _ = _stack((3, 4, 40, 52), seed=9)
    want, winfo = t2.denoise_tv(b, 15.0, return_info=True)
    again = t2.denoise_tv(b, 15.0)
    assert again.tobytes() == want.tobytes()
    t = torch.from_numpy(b).cuda()
    res, tinfo = t2.denoise_tv(t, 15.0, return_info=True)
    assert res.is_cuda and res.data_ptr() != t.data_ptr() and torch.equal(t.cpu(), torch.from_numpy(b))
    assert res.cpu().numpy().tobytes() == want.tobytes() and np.array_equal(tinfo["n_iter"].cpu().numpy(), winfo["n_iter"])
    same = t2.denoise_tv(t, 15.0, out=t)
    assert same.data_ptr() == t.data_ptr() and t.cpu().numpy().tobytes() == want.tobytes()
    grouped, ginfo = t2.denoise_tv(b, 15.0, return_info=True, max_workspace_bytes=1)
    assert grouped.tobytes() == want.tobytes() and np.array_equal(ginfo["n_iter"], winfo["n_iter"])
    with pytest.raises(ValueError, match="moveaxis"):
        t2.denoise_tv(np.zeros((4, 4, 4, 3), np.float32), layout="voxel_major")


def test_raw_ctypes_call_equals_the_wrapper(t2):
    import torch

    from fetal_t2mapping_amd import _abi
    from fetal_t2mapping_amd._lib import load

    lib = load()
    a, _ = _stack((2, 3, 33, 44), seed=21)
    want, info = t2.denoise_tv(a, 12.0, dims=3, precision="f64", return_info=True)
    par = _abi.T2FitTvParams()
    assert lib.t2fit_tv_params_default(C.byref(par)) == _abi.OK
    par.weight, par.dims, par.precision = 12.0, 3, _abi.PREC_F64
    need = C.c_size_t()
    assert lib.t2fit_tv_workspace_bytes(C.byref(par), 2, 3, 33, 44, C.byref(need)) == _abi.OK
    src = torch.from_numpy(a).cuda()
    dst = torch.empty_like(src)
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    n_iter = torch.empty(2, dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.t2fit_tv_denoise_dev(C.byref(par), src.data_ptr(), dst.data_ptr(), 2, 3, 33, 44, ws.data_ptr(), need.value,
                                    n_iter.data_ptr(), None, st) == _abi.OK
    torch.cuda.synchronize()
    assert dst.cpu().numpy().tobytes() == want.tobytes() and np.array_equal(n_iter.cpu().numpy(), info["n_iter"])
    assert lib.t2fit_tv_denoise_dev(C.byref(par), src.data_ptr(), dst.data_ptr(), 2, 3, 33, 44, ws.data_ptr() + 16, need.value,
                                    None, None, st) == _abi.E_INVALID
    assert b"aligned" in lib.t2fit_last_error()


@pytest.mark.parametrize("dims", [2, 3])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_raw_calls_on_another_stream_poisoned_workspace_and_offset_buffers(t2, dims, precision):
    """ctypes calls on a caller's stream, the workspace all 0xFF (every float and double of it a NaN) before each call,
    nx % 4 == 0: (a) in and out 4 bytes past a 256-byte boundary, (b) only out, (c) only in, (d) in place 4 bytes past,
    (e) aligned with n_iter_dev and energy_dev NULL.  Every result bit-equal to the statement, at an even and an odd
    n_iter; the words around every output buffer keep their bytes."""
    import torch

    from fetal_t2mapping_amd import _abi, _tv
    from fetal_t2mapping_amd._lib import load

    lib = load()
    shape = (2, 3, 9, 68)
    a = K.field(shape, seed=68)
    n, pad, guard = a.size, 64, 0x5A5A5A5A
    n_problems = len(K.problems(a, dims))
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)

    def buffer(shift):
        """n floats that start `shift` * 4 bytes past a 256-byte boundary, guard words on both sides."""
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
        want, want_n, want_e = _tv.denoise_tv(a, 12.0, 0.0, max_iter, dims, precision)
        need = C.c_size_t()
        assert lib.t2fit_tv_workspace_bytes(C.byref(par), *shape, C.byref(need)) == _abi.OK
        for name, in_shift, out_shift, in_place, with_info in (("a", 1, 1, False, True), ("b", 0, 1, False, True),
                                                               ("c", 1, 0, False, True), ("d", 1, 1, True, True),
                                                               ("e", 0, 0, False, False)):
            with torch.cuda.stream(stream):
                ws = torch.empty(need.value + 256, dtype=torch.uint8, device="cuda")
                ws.fill_(0xFF)
                ws_ptr = (ws.data_ptr() + 255) // 256 * 256
                src_buf, src = buffer(in_shift)
                src.copy_(torch.from_numpy(a.reshape(-1)))
                dst_buf, dst = (src_buf, src) if in_place else buffer(out_shift)
                n_iter = torch.full((n_problems,), -1, dtype=torch.int32, device="cuda")
                energy = torch.full((n_problems,), -1.0, dtype=torch.float64, device="cuda")
                rc = lib.t2fit_tv_denoise_dev(C.byref(par), src.data_ptr(), dst.data_ptr(), *shape, ws_ptr, need.value,
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


def test_groups_of_three_and_two_volumes_equal_the_whole_call(t2, monkeypatch):
    """Five volumes under a max_workspace_bytes that fits exactly three: the wrapper halves 5 to 3, runs 3 and 2, and
    returns the bytes of the whole call."""
    from fetal_t2mapping_amd import _abi
    from fetal_t2mapping_amd._gpu_tv import tv_params
    from fetal_t2mapping_amd._lib import load

    lib = load()
    shape = (5, 2, 9, 12)
    a = K.field(shape, seed=5)
    par = tv_params(15.0)

    def need(n_vol):
        v = C.c_size_t()
        assert lib.t2fit_tv_workspace_bytes(C.byref(par), n_vol, *shape[1:], C.byref(v)) == _abi.OK
        return v.value

    budget = need(3)
    assert need(5) > budget and need(4) > budget and (5 + 1) // 2 == 3  # 5 does not fit, its half rounded up does
    want, winfo = t2.denoise_tv(a, 15.0, return_info=True)
    real, calls = lib.t2fit_tv_denoise_dev, []

    def spy(*args):
        calls.append((int(args[3]), int(args[8])))
        return real(*args)

    monkeypatch.setattr(lib, "t2fit_tv_denoise_dev", spy)
    got, info = t2.denoise_tv(a, 15.0, return_info=True, max_workspace_bytes=budget)
    assert calls == [(3, budget), (2, budget)]
    assert got.tobytes() == want.tobytes() and np.array_equal(info["n_iter"], winfo["n_iter"])
    assert info["energy"].tobytes() == winfo["energy"].tobytes()
    assert len(set(info["n_iter"].tolist())) > 1  # (the problems differ: a wrong offset of a group's results would show)


def test_whole_size_stack_at_one_sigma(t2):
    import torch

    from fetal_t2mapping_amd import synth

    shape = (180, 256, 256)
    echoes, mask, te = synth.brain_volume_torch(shape, 6, seed=synth.SEED_BASE, device=torch.device("cuda", 0))
    echoes, mask = echoes.reshape((6,) + shape), mask.reshape(shape)
    sigma, count = t2.estimate_background_sigma(echoes, mask)
    assert 15.0 < sigma < 25.0
    mean_in = echoes.double().mean(dim=(2, 3))
    out, info = t2.denoise_tv(echoes, sigma, return_info=True)
    torch.cuda.synchronize()
    n_iter = info["n_iter"].cpu().numpy()
    print(f"256 x 256 x 180 x 6 at weight 1 sigma = {sigma:.2f}: n_iter min {n_iter.min()} mean {n_iter.mean():.1f} "
          f"median {np.median(n_iter):.0f} max {n_iter.max()}")
    assert n_iter.shape == (6 * 180,) and n_iter.min() >= 1 and n_iter.max() <= 199
    mean_out = out.double().mean(dim=(2, 3))
    assert torch.all((mean_out - mean_in).abs() <= 1e-4 * mean_in.abs().clamp(min=1.0))  # sum d = 0 up to float32 rounding
    assert float((out - echoes).abs().max()) > 1.0


def test_fit_of_the_denoised_phantom_is_closer_to_the_truth(t2):
    from fetal_t2mapping_amd import synth

    echoes, mask, label, te, gt = synth.phantom_volume((12, 96, 96), 6, sigma=40.0)
    truth = np.zeros(label.shape)
    for i, v in enumerate(gt):
        truth[label == i + 1] = v
    sel = (label > 0) & (truth >= 40) & (truth <= 700)
    sigma, _ = t2.estimate_background_sigma(echoes, mask)
    den = t2.denoise_tv(echoes, sigma)
    rmse = {}
    for name, stack in (("noisy", echoes), ("denoised", den)):
        maps = t2.fit_volume(stack, mask, te, "gaussian", t2.fit_table("gaussian", False), solver="lm", precision="f32")
        rmse[name] = float(np.sqrt(np.mean((maps.t2[sel] - truth[sel]) ** 2)))
    print(f"T2 RMSE over the vials, sigma {sigma:.1f}: {rmse}")
    assert rmse["denoised"] < rmse["noisy"]


def _tree(tmp_path):
    """A tiny BIDS tree: three echoes of a synthetic brain volume and their masks."""
    import pandas as pd

    from fetal_t2mapping_amd import cli as R
    from fetal_t2mapping_amd import nifti, synth

    echoes, mask, te = synth.brain_volume((10, 24, 32), 3, seed=synth.SEED_BASE, low_field=True)
    root = str(tmp_path)
    bids = os.path.join(root, "projects") + "/"
    os.makedirs(os.path.join(bids, "prj-905"))
    os.makedirs(os.path.join(root, "dicom", "logs"))
    rows = []
    for i, t in enumerate(te):
        acq = {"prj": "prj-905", "sub": "sub-006", "ses": "ses-01", "run": f"run-{i + 1:02d}", "EchoTime": t / 1000.0,
               "CoilString": "HeadNeck"}
        rows.append(acq)
        for arr, dirname in ((echoes[i], R.recon_dirname), (mask, R.mask_dirname)):
            nifti.WriteImage(nifti.GetImageFromArray(arr), R.get_img_path(bids, acq, dirname).replace(" ", ""))
    pd.DataFrame(rows).to_csv(os.path.join(root, "dicom", "logs", "log.csv"), index=False)
    out_dir = os.path.join(bids, "prj-905", "derivatives", R.t2map_dirname, "sub-006", "ses-01", "anat")
    return root, out_dir, echoes, mask, te


def test_cli_denoises_ahead_of_the_fit(t2, tmp_path, monkeypatch, capsys):
    import sys

    from fetal_t2mapping_amd import cli as R
    from fetal_t2mapping_amd import nifti

    monkeypatch.setitem(sys.modules, "SimpleITK", None)
    root0, out0, echoes, mask, te = _tree(tmp_path / "plain")
    base = ["--csv", "log.csv", "--in_vivo", "--gaussian", "--lf", "--sim", "d1", "--TEs"] + [str(int(t)) for t in te]
    R.main(["--path", root0] + base)
    assert "Denoising" not in capsys.readouterr().out
    root1, out1, _, _, _ = _tree(tmp_path / "tv")
    R.main(["--path", root1] + base + ["--denoise", "tv", "--denoise_weight", "1sigma"])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Denoising:")]
    assert len(line) == 1 and "background sigma" in line[0] and "n_iter mean" in line[0] and "30 problems" in line[0]
    assert sorted(os.listdir(out0)) == sorted(os.listdir(out1)) and len(os.listdir(out0)) == 4
    name = [f for f in os.listdir(out0) if "t2map" in f][0]
    plain = nifti.ReadImage(os.path.join(out0, name)).arr
    tv = nifti.ReadImage(os.path.join(out1, name)).arr
    assert not np.array_equal(plain, tv) and np.all(tv[mask == 0] == 0)
    # without the flag the maps are those of the fit of the stack as read; with it, those of the denoised stack
    fit = t2.fit_volume(echoes, mask, te, "gaussian", t2.fit_table("gaussian", True))
    assert np.array_equal(plain, fit.t2)
    sigma, _ = t2.estimate_background_sigma(echoes, mask)
    fit_tv = t2.fit_volume(t2.denoise_tv(echoes, sigma), mask, te, "gaussian", t2.fit_table("gaussian", True))
    assert np.array_equal(tv, fit_tv.t2)
