"""The TV-Chambolle denoiser on the device (csrc/t2fit_denoise.hip) against its numpy statement (fetal_t2mapping_amd/_tv.py):
bit for bit at a fixed iteration count, iteration counts under the stop rule, independence of the problems of one call,
in-place / repeat / entry-point identities, a whole-size stack, and the step inside the fit pipeline and the CLI.
tests/test_denoise_host.py covers the definition, the argument checks and the flags without a device."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def t2():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X")
    import fetal_t2mapping_amd as t2

    return t2


def _stack(shape, seed, sigma=20.0):
    """Piecewise-constant slices (blocks of 300 / 900 / 1500 over a zero background) under Rician noise."""
    rng = np.random.default_rng(seed)
    n, z, y, x = shape
    yy, xx = np.meshgrid(np.arange(y), np.arange(x), indexing="ij")
    clean = np.zeros(shape)
    for v in range(n):
        for k in range(z):
            img = np.where((yy > y // 5) & (xx > x // 6), 300.0, 0.0)
            img = np.where((yy > y // 2) & (xx < x // 2 + k), 900.0 + 50.0 * v, img)
            img = np.where((yy - y / 2) ** 2 + (xx - x / 2) ** 2 < (min(y, x) / 5 + k) ** 2, 1500.0, img)
            clean[v, k] = img
    noisy = np.hypot(clean + rng.normal(scale=sigma, size=shape), rng.normal(scale=sigma, size=shape))
    return noisy.astype(np.float32), clean


SIZES = [(2, 1, 64, 64), (2, 5, 37, 53), (1, 3, 256, 256), (2, 16, 17, 1)]


@pytest.mark.parametrize("shape", SIZES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dims", [2, 3])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_fixed_iteration_count_is_bit_equal_to_the_numpy_statement(t2, shape, dims, precision):
    from fetal_t2mapping_amd import _tv

    a, _ = _stack(shape, seed=11)
    for max_iter in (1, 2, 7, 40):
        want, want_n, want_e = _tv.denoise_tv(a, 25.0, 0.0, max_iter, dims, precision)
        got, info = t2.denoise_tv(a, 25.0, eps=0.0, max_iter=max_iter, dims=dims, precision=precision, return_info=True)
        assert got.dtype == np.float32 and got.shape == a.shape
        assert np.array_equal(info["n_iter"], want_n) and np.all(want_n == max_iter - 1)
        bad = int(np.sum(got.view(np.uint32) != want.view(np.uint32)))
        assert bad == 0, (shape, dims, precision, max_iter, bad, float(np.abs(got - want).max()))
        assert np.allclose(info["energy"], want_e, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("dims,precision", [(2, "f32"), (2, "f64"), (3, "f32"), (3, "f64")])
def test_stop_rule_gives_the_iteration_counts_of_the_numpy_statement(t2, dims, precision):
    from fetal_t2mapping_amd import _tv

    a, _ = _stack((2, 6, 96, 80), seed=5)
    for weight in (0.1, 10.0, 20.0, 40.0):
        want, want_n, want_e = _tv.denoise_tv(a, weight, 2e-4, 200, dims, precision)
        got, info = t2.denoise_tv(a, weight, dims=dims, precision=precision, return_info=True)
        diff = np.flatnonzero(info["n_iter"] != want_n)
        for k in diff:  # the bar is none; a marginal stop (|E_prev - E| within float64 rounding of the threshold) would show here
            print(f"problem {k}: n_iter {info['n_iter'][k]} vs {want_n[k]}, E {info['energy'][k]!r} vs {want_e[k]!r}")
        assert diff.size == 0, (weight, diff, info["n_iter"][diff], want_n[diff])
        assert got.tobytes() == want.tobytes(), weight
        print(f"dims {dims} {precision} weight {weight}: n_iter min {want_n.min()} mean {want_n.mean():.1f} max {want_n.max()}")
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
