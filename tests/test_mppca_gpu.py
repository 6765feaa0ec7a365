"""The MP-PCA denoiser on the device (csrc/t2fit_mppca.hip: mppca_eigen_kernel, mppca_aggregate_kernel) against its numpy
statement (fetal_t2mapping_amd/_mppca.py): the uint32 views of out and sigma, and rank, exactly, over the table of
tests/mppca_cases.py, every echo count from 2 to 16, both estimators, degenerate blocks, a NaN, a mask, raw calls (in
place, offset buffers, a caller's stream, a poisoned workspace, estimate-only without a workspace, repeats, refusals),
slice groups and slabs, the CLI and the unchanged default path.  tests/test_mppca_host.py holds the statement to an
independent reference."""
import ctypes as C
import os

import numpy as np
import pytest

import mppca_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def t2():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X")
    import fetal_t2mapping_amd as t2

    return t2


def _same(got, want, what):
    out, sigma, rank = got
    assert out.dtype == np.float32 and sigma.dtype == np.float32 and rank.dtype == np.uint8, what
    assert out.shape == want[0].shape and sigma.shape == want[1].shape and rank.shape == want[2].shape, what
    # NaN payloads included: the words are compared, not the values
    bad = (int(np.sum(out.view(np.uint32) != want[0].view(np.uint32))), int(np.sum(sigma.view(np.uint32) != want[1].view(np.uint32))),
           int(np.sum(rank != want[2])))
    assert bad == (0, 0, 0), (what, bad)


def _run(t2, a, r, dims, estimator=2, mask=None, **kw):
    out, maps = t2.denoise_mppca(a, radius=r, dims=dims, estimator=estimator, mask=mask, return_maps=True, **kw)
    return out, maps["sigma"], maps["rank"]


@pytest.mark.parametrize("case", K.GPU_CASES, ids=["x".join(map(str, c[:4])) + f"-{c[4]}d-r{c[5]}" for c in K.GPU_CASES])
def test_table_is_bit_equal_to_the_numpy_statement(t2, case):
    a = np.array(K.gpu_stack(case))
    want = K.gpu_want(case)
    _same(_run(t2, a, case[5], case[4]), want, case)
    sigma, rank = t2.mppca_noise_map(a, radius=case[5], dims=case[4])
    assert sigma.tobytes() == want[1].tobytes() and rank.tobytes() == want[2].tobytes()
    assert t2.denoise_mppca(a, radius=case[5], dims=case[4]).tobytes() == want[0].tobytes()
    if want[2].size >= 1000:  # the picture has windows inside one compartment and windows across a boundary
        assert (want[2] == 1).any() and (want[2] == 2).any() and want[2].min() >= 1
    assert np.isfinite(want[0]).all() and (want[1] > 0).all() and want[0].tobytes() != a.tobytes()


@pytest.mark.parametrize("case", K.BOTH_ESTIMATORS, ids=["x".join(map(str, c[:4])) for c in K.BOTH_ESTIMATORS])
def test_both_estimators(t2, case):
    a = np.array(K.gpu_stack(case))
    one, two = K.gpu_want(case, 1), K.gpu_want(case, 2)
    _same(_run(t2, a, case[5], case[4], estimator=1), one, (case, 1))
    _same(_run(t2, a, case[5], case[4], estimator=2), two, (case, 2))
    assert one[2].tobytes() != two[2].tobytes() and one[0].tobytes() != two[0].tobytes()


@pytest.mark.parametrize("case", K.EVERY_M, ids=["x".join(map(str, c[:4])) + f"-{c[4]}d-r{c[5]}" for c in K.EVERY_M])
def test_every_echo_count_with_both_estimators(t2, case):
    """M = 2 .. 8 each have kernels of their own (the matrices in registers, every index a constant), M = 9 .. 16 share
    the generic pair: each launched, the centres more than one wave and the last wave ragged."""
    a = np.array(K.gpu_stack(case))
    for estimator in (2, 1):
        want = K.gpu_want(case, estimator)
        _same(_run(t2, a, case[5], case[4], estimator=estimator), want, (case, estimator))
        assert np.isfinite(want[0]).all() and (want[1] > 0).all() and want[2].min() >= 1 and want[0].tobytes() != a.tobytes()
    centres = np.prod([n - 2 * case[5] for n in case[2:4]]) * (case[1] - 2 * case[5] if case[4] == 3 else case[1])
    assert centres > 64 and centres % 64 != 0


def _degenerate_blocks(t2, m):
    """A constant block, an all-zero block, one NaN and a mask with holes at ``m`` echoes, 2-D and 3-D.  Radius 1, but for
    2-D above 8 echoes radius 2: a window holds more voxels than there are echoes, and 9 are not more than 12."""
    from fetal_t2mapping_amd import _mppca

    shape = (m, 3, 13, 21)
    cases = [(dims, 2 if dims == 2 and m >= 9 else 1) for dims in (2, 3)]
    if m >= 9:
        with pytest.raises(ValueError, match="more voxels"):
            _mppca.check(shape, 1, 2, 2)
    a = np.array(K.picture(shape, seed=77))
    a[:, :, 3:9, 2:9] = 250.0                      # a constant block: G of rank 1 exactly, with ties in its spectrum
    a[:, :, 6:13, 12:21] = 0.0                     # an all-zero block: G = 0, no sweep, nothing cut
    for dims, r in cases:
        want = _mppca.mppca(a, r, dims)
        _same(_run(t2, a, r, dims), want, ("blocks", m, dims))
        assert want[2][1, 9, 16] == shape[0] and want[1][1, 9, 16] == 0.0 and not want[0][:, 1, 9, 16].any()
    b = np.array(K.picture(shape, seed=78))
    b[2, 1, 6, 10] = np.nan
    mask = K.holes_mask(shape[1:])
    for dims, r in cases:
        want = _mppca.mppca(b, r, dims)
        _same(_run(t2, b, r, dims), want, ("nan", m, dims))
        assert np.isnan(want[0][2, 1, 6, 10]) and np.isnan(want[0]).sum() == 1 and want[1][1, 6, 10] == 0.0
        want = _mppca.mppca(b, r, dims, mask=mask)
        _same(_run(t2, b, r, dims, mask=mask), want, ("nan + mask", m, dims))
        clean = np.array(K.picture(shape, seed=78))
        want = _mppca.mppca(clean, r, dims, mask=mask)
        _same(_run(t2, clean, r, dims, mask=mask), want, ("mask", m, dims))
        assert (want[1] == 0).any() and (want[1] > 0).any() and (want[0] == clean).all(axis=0).any()
        sigma, rank = t2.mppca_noise_map(clean, radius=r, dims=dims, mask=mask)
        assert sigma.tobytes() == want[1].tobytes() and rank.tobytes() == want[2].tobytes()
        none = _run(t2, clean, r, dims, mask=np.zeros(shape[1:], np.uint8))
        assert none[0].tobytes() == clean.tobytes() and not none[1].any() and not none[2].any()


def test_constant_and_zero_blocks_one_nan_and_a_mask_with_holes(t2):
    _degenerate_blocks(t2, 4)


@pytest.mark.parametrize("m", [5, 7, 12])
def test_degenerate_blocks_at_the_echo_counts_no_other_test_launches_and_on_the_generic_path(t2, m):
    _degenerate_blocks(t2, m)


@pytest.mark.parametrize("case", [(6, 3, 9, 68, 2, 1), (8, 5, 7, 12, 3, 1), (9, 4, 6, 8, 3, 1), (5, 3, 7, 12, 3, 1), (7, 2, 9, 12, 2, 1),
                                  (12, 3, 7, 12, 3, 1)], ids=["6-2d", "8-3d", "9-3d-generic", "5-3d", "7-2d", "12-3d-generic"])
def test_raw_calls_on_another_stream_poisoned_workspace_offset_buffers_and_estimate_only(t2, case):
    """ctypes calls on a caller's stream, the workspace all 0xFF before each call: (a) in and out 4 bytes past a 256-byte
    boundary, (b) only out, (c) only in, (d) in place 4 bytes past, (e) aligned and in place, (f) aligned with sigma and
    rank NULL, (g) estimate-only: out NULL, workspace NULL and 0 bytes; (e) three times over.  Every result bit-equal to the
    statement; the words around every buffer keep their bytes.  Under the mask a centre that is not processed must still
    write a zero projector over the poisoned words, for all M (M + 1) / 2 pairs: in the kernels of M = 5 and 7 as on the
    generic path (M = 9, 12)."""
    import torch

    from fetal_t2mapping_amd import _abi, _mppca
    from fetal_t2mapping_amd._lib import load

    lib = load()
    shape, dims, r = case[:4], case[4], case[5]
    a = K.picture(shape, seed=68)
    mask = K.holes_mask(shape[1:], seed=4)
    n, n_v, pad, guard = a.size, a[0].size, 64, 0x5A5A5A5A
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)
    par = _abi.T2FitMppcaParams()
    assert lib.t2fit_mppca_params_default(C.byref(par)) == _abi.OK
    par.radius, par.dims = r, dims
    need = C.c_size_t()
    assert lib.t2fit_mppca_workspace_bytes(C.byref(par), *shape, C.byref(need)) == _abi.OK

    def buffer(shift, count):
        buf = torch.full((count + 3 * pad,), guard, dtype=torch.int32, device="cuda")
        assert buf.data_ptr() % 256 == 0
        view = buf[pad + shift:pad + shift + count].view(torch.float32)
        assert view.data_ptr() % 256 == 4 * shift
        return buf, view

    def guards_kept(buf, shift, count):
        host = buf.cpu().numpy()
        return bool(np.all(host[:pad + shift] == guard) and np.all(host[pad + shift + count:] == guard))

    for use_mask in (False, True):
        want = _mppca.mppca(a, r, dims, mask=mask if use_mask else None)
        for name, in_shift, out_shift, in_place, maps, estimate in (
                ("a", 1, 1, False, True, False), ("b", 0, 1, False, True, False), ("c", 1, 0, False, True, False),
                ("d", 1, 1, True, True, False), ("e", 0, 0, True, True, False), ("e", 0, 0, True, True, False),
                ("e", 0, 0, True, True, False), ("f", 0, 0, False, False, False), ("g", 1, 0, False, True, True)):
            with torch.cuda.stream(stream):
                ws = torch.empty(need.value + 256, dtype=torch.uint8, device="cuda")
                ws.fill_(0xFF)
                ws_ptr = (ws.data_ptr() + 255) // 256 * 256
                src_buf, src = buffer(in_shift, n)
                src.copy_(torch.from_numpy(a.reshape(-1)))
                dst_buf, dst = (src_buf, src) if in_place else buffer(out_shift, n)
                sig_buf, sig = buffer(out_shift, n_v)
                rank = torch.full((n_v + 128,), 0xA5, dtype=torch.uint8, device="cuda")
                m_d = torch.from_numpy(mask.reshape(-1)).cuda() if use_mask else None
                rc = lib.t2fit_mppca_dev(C.byref(par), src.data_ptr(), None if m_d is None else m_d.data_ptr(),
                                         None if estimate else dst.data_ptr(), sig.data_ptr() if maps else None,
                                         rank.data_ptr() + 64 if maps else None, *shape, None if estimate else ws_ptr,
                                         0 if estimate else need.value, st)
                assert rc == _abi.OK, (name, lib.t2fit_last_error())
                stream.synchronize()
            what = (name, case, use_mask)
            if estimate:
                assert np.all(dst_buf.cpu().numpy() == guard), what
            else:
                assert dst.cpu().numpy().tobytes() == want[0].tobytes(), what
                assert guards_kept(dst_buf, out_shift, n), what
            if not in_place:
                assert src.cpu().numpy().tobytes() == a.tobytes() and guards_kept(src_buf, in_shift, n), what
            rank_h = rank.cpu().numpy()
            if maps:
                assert sig.cpu().numpy().tobytes() == want[1].tobytes() and guards_kept(sig_buf, out_shift, n_v), what
                assert rank_h[64:64 + n_v].tobytes() == want[2].tobytes(), what
                assert np.all(rank_h[:64] == 0xA5) and np.all(rank_h[64 + n_v:] == 0xA5), what
            else:
                assert np.all(sig_buf.cpu().numpy() == guard) and np.all(rank_h == 0xA5), what
    # refusals with live buffers: E_INVALID, a message, and no byte of any buffer written
    src_buf, src = buffer(0, n)
    dst_buf, dst = buffer(0, n)
    torch.cuda.synchronize()
    for kw in ({"radius": 0}, {"dims": 4}, {"estimator": 3}, {"flags": 2}, {"ws_bytes": need.value - 1}, {"n_te": 1},
               {"n_te": K.MAX_TE + 1}, {"nx": 2 * r}, {"ws": 64}):
        q = _abi.T2FitMppcaParams(kw.get("radius", r), kw.get("dims", dims), kw.get("estimator", 2), kw.get("flags", 0))
        size = (kw.get("n_te", shape[0]), shape[1], shape[2], kw.get("nx", shape[3]))
        rc = lib.t2fit_mppca_dev(C.byref(q), src.data_ptr(), None, dst.data_ptr(), None, None, *size, ws_ptr + kw.get("ws", 0),
                                 kw.get("ws_bytes", need.value), st)
        assert rc == _abi.E_INVALID and b"t2fit_mppca_dev" in lib.t2fit_last_error(), kw
    torch.cuda.synchronize()
    assert np.all(src_buf.cpu().numpy() == guard) and np.all(dst_buf.cpu().numpy() == guard)


def test_wrapper_entries_slice_groups_slabs_and_the_refusals(t2, monkeypatch):
    import torch

    from fetal_t2mapping_amd import _abi, _mppca
    from fetal_t2mapping_amd._gpu_mppca import mppca_params
    from fetal_t2mapping_amd._lib import load

    lib = load()
    real, calls = lib.t2fit_mppca_dev, []

    def spy(*args):
        calls.append((int(args[7]), int(args[11])))  # (nz of the call, workspace bytes)
        return real(*args)

    monkeypatch.setattr(lib, "t2fit_mppca_dev", spy)
    for dims, r, shape in ((2, 2, (4, 5, 9, 12)), (3, 1, (4, 9, 7, 12))):
        a = K.picture(shape, seed=5 + dims)
        mask = K.holes_mask(shape[1:], seed=6)
        want = _mppca.mppca(a, r, dims)
        par = mppca_params(r, dims)

        def need(nz):
            v = C.c_size_t()
            assert lib.t2fit_mppca_workspace_bytes(C.byref(par), shape[0], nz, *shape[2:], C.byref(v)) == _abi.OK
            return v.value

        # tensor entry, out of place and in place
        t = torch.from_numpy(a).cuda()
        res, maps = t2.denoise_mppca(t, radius=r, dims=dims, return_maps=True)
        assert res.is_cuda and res.data_ptr() != t.data_ptr() and torch.equal(t.cpu(), torch.from_numpy(a))
        _same((res.cpu().numpy(), maps["sigma"].cpu().numpy(), maps["rank"].cpu().numpy()), want, ("tensor", dims))
        same = t2.denoise_mppca(t, radius=r, dims=dims, out=t)
        assert same.data_ptr() == t.data_ptr() and t.cpu().numpy().tobytes() == want[0].tobytes()
        # dims 2: slices in groups of 3 and 2; dims 3: slabs of 3 + 3 + 3 slices with a halo of 2 r on each inner side
        del calls[:]
        if dims == 2:
            budget = need(3)
            assert need(5) > budget and need(4) > budget
            expect = [(3, budget), (2, budget)]
        else:
            budget = need(3 + 4 * r)
            assert need(9) > budget and need(5 + 4 * r) > budget
            expect = [(5, budget), (7, budget), (5, budget)]
        _same(_run(t2, a, r, dims, max_workspace_bytes=budget), want, ("groups", dims))
        assert calls == expect, calls
        want_m = _mppca.mppca(a, r, dims, mask=mask)
        _same(_run(t2, a, r, dims, mask=mask, max_workspace_bytes=budget), want_m, ("groups + mask", dims))
        # grouped and in place: a later slab must not read what an earlier one wrote
        t = torch.from_numpy(a).cuda()
        t2.denoise_mppca(t, radius=r, dims=dims, out=t, max_workspace_bytes=budget)
        assert t.cpu().numpy().tobytes() == want[0].tobytes()
        with pytest.raises(ValueError, match="does not fit"):
            t2.denoise_mppca(a, radius=r, dims=dims, max_workspace_bytes=need(1 + 4 * r if dims == 3 else 1) - 1)
    with pytest.raises(ValueError, match=r"\(nTE, Z, Y, X\)"):
        t2.denoise_mppca(a[0])
    with pytest.raises(ValueError, match=r"\(nTE, Z, Y, X\)"):
        t2.mppca_noise_map(a[0])
    with pytest.raises(ValueError, match="out= goes with a CUDA tensor"):
        t2.denoise_mppca(a, out=np.empty_like(a))
    for kw, word in (({"radius": 0}, "radius"), ({"radius": 5}, "radius"), ({"dims": 1}, "dims"), ({"estimator": 3}, "estimator")):
        with pytest.raises(ValueError, match=word):
            t2.denoise_mppca(a, **kw)
    with pytest.raises(ValueError, match="T2FIT_MPPCA_MAX_TE"):
        t2.denoise_mppca(np.zeros((K.MAX_TE + 1, 1, 9, 9), np.float32))
    with pytest.raises(ValueError, match="more voxels"):
        t2.mppca_noise_map(np.zeros((9, 1, 9, 9), np.float32), radius=1)
    with pytest.raises(ValueError, match="mask shape"):
        t2.denoise_mppca(a, radius=1, mask=np.ones((2, 2, 2), np.uint8))


def _tree(tmp_path, shape=(4, 16, 16)):
    """A tiny BIDS tree: three echoes of a synthetic brain volume and their masks."""
    import pandas as pd

    from fetal_t2mapping_amd import cli as R
    from fetal_t2mapping_amd import nifti, synth

    echoes, mask, te = synth.brain_volume(shape, 3, seed=synth.SEED_BASE, low_field=True)
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
    return root, out_dir, np.asarray(echoes, np.float32), mask, te


def _read(out_dir, tag):
    from fetal_t2mapping_amd import nifti

    name = [f for f in os.listdir(out_dir) if f"_{tag}map_" in f]
    assert len(name) == 1, (tag, os.listdir(out_dir))
    return nifti.ReadImage(os.path.join(out_dir, name[0])).arr


def test_cli_denoises_writes_the_noise_map_and_feeds_the_bootstrap_and_the_tv_weight(t2, tmp_path, monkeypatch, capsys):
    import sys

    from fetal_t2mapping_amd import _mppca, _tv
    from fetal_t2mapping_amd import cli as R
    from fetal_t2mapping_amd._lib import load

    monkeypatch.setitem(sys.modules, "SimpleITK", None)
    lib = load()
    real, calls = lib.t2fit_mppca_dev, []
    monkeypatch.setattr(lib, "t2fit_mppca_dev", lambda *args: calls.append(args[3] is not None) or real(*args))
    table = t2.fit_table("gaussian", True)

    def run(name, extra):
        root, out, echoes, mask, te = _tree(tmp_path / name)
        base = ["--csv", "log.csv", "--in_vivo", "--gaussian", "--lf", "--sim", "d1", "--TEs"] + [str(int(t)) for t in te]
        del calls[:]
        R.main(["--path", root] + base + extra)
        return out, echoes, mask, te, capsys.readouterr().out

    # --denoise tv: the bytes of the TV statement's fit, four files, and no MP-PCA launch
    out_tv, echoes, mask, te, text = run("tv", ["--denoise", "tv", "--denoise_weight", "1sigma"])
    assert calls == [] and len(os.listdir(out_tv)) == 4
    sigma_bg, _ = t2.estimate_background_sigma(echoes, mask)
    den = _tv.denoise_tv(echoes, sigma_bg, 2e-4, 200, 2, "f32")[0]
    assert np.array_equal(_read(out_tv, "t2"), t2.fit_volume(den, mask, te, "gaussian", table).t2)
    out_plain = run("plain", [])[0]
    assert calls == [] and len(os.listdir(out_plain)) == 4
    assert np.array_equal(_read(out_plain, "t2"), t2.fit_volume(echoes, mask, te, "gaussian", table).t2)
    # --denoise mppca --write_noise_map: the fit of the statement's output, and the statement's maps beside it
    want = _mppca.mppca(echoes, 1, 3)
    out_mp, _, _, _, text = run("mppca", ["--denoise", "mppca", "--denoise_patch", "1", "--denoise_dims", "3", "--write_noise_map"])
    line = [ln for ln in text.splitlines() if ln.startswith("Denoising:")]
    assert len(line) == 1 and "MP-PCA 3-D, radius 1 (27 voxels per window)" in line[0] and "median sigma" in line[0]
    assert calls == [True] and len(os.listdir(out_mp)) == 6
    assert np.array_equal(_read(out_mp, "t2"), t2.fit_volume(want[0], mask, te, "gaussian", table).t2)
    assert _read(out_mp, "mppcasigma").tobytes() == want[1].tobytes() and np.array_equal(_read(out_mp, "mppcarank"), want[2])
    # denoise_subject alone
    vols = R.denoise_subject([e for e in echoes], [mask] * 3, method="mppca", radius=1, dims=3)
    assert np.stack(vols).tobytes() == want[0].tobytes()
    capsys.readouterr()
    # --write_noise_map alone: the maps of the fit of the stack as read, and the noise map from one estimate-only call
    want2 = _mppca.mppca(echoes, 2, 2)
    out_nm = run("noise", ["--write_noise_map"])[0]
    assert calls == [False] and len(os.listdir(out_nm)) == 6
    assert np.array_equal(_read(out_nm, "t2"), _read(out_plain, "t2"))
    assert _read(out_nm, "mppcasigma").tobytes() == want2[1].tobytes() and np.array_equal(_read(out_nm, "mppcarank"), want2[2])
    # --bootstrap_noise mppca: the replicas of bootstrap_volume given the statement's sigma map
    out_bt, _, _, _, text = run("boot", ["--bootstrap", "4", "--bootstrap_noise", "mppca", "--denoise_patch", "1"])
    assert calls == [False] and "the MP-PCA sigma map (mppca)" in text
    want1 = _mppca.mppca(echoes, 1, 2)
    boot = t2.bootstrap_volume(echoes, mask, te, "gaussian", table, n_replicas=4, seed=0, alpha=0.05, noise_sigma=want1[1])
    assert _read(out_bt, "T2std").tobytes() == np.asarray(boot.boot_std).tobytes() and np.isfinite(boot.boot_std[mask != 0]).any()
    assert np.array_equal(_read(out_bt, "t2"), _read(out_plain, "t2"))
    # --denoise_sigma mppca: the TV weight from the median of the statement's sigma inside the mask
    out_ts, _, _, _, text = run("tvs", ["--denoise", "tv", "--denoise_weight", "1sigma", "--denoise_sigma", "mppca"])
    level = float(np.median(want2[1][mask != 0]))
    assert calls == [False] and f"MP-PCA median sigma {level:.4g}" in text
    den = _tv.denoise_tv(echoes, level, 2e-4, 200, 2, "f32")[0]
    assert np.array_equal(_read(out_ts, "t2"), t2.fit_volume(den, mask, te, "gaussian", table).t2)
    assert not np.array_equal(_read(out_ts, "t2"), _read(out_tv, "t2"))
