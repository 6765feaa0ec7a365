"""The T2-spectrum fit on the device (csrc/t2fit_nnls.hip: nnls_kernel) against its numpy statement
(fetal_t2mapping_amd/_nnls.py): x, every functional, amp, rmse, nit and status bit for bit, and equal from call to call, over
basis and echo counts (the smallest, odd ones, the largest), voxel counts (one, around a 64-voxel chunk, around the voxels
a workgroup takes at once, and several chunks per wave of a capped persistent grid), three values of mu (the last fills the
passive set), masks with empty and full chunks, zero / negative / NaN / Inf voxels and samples at the ends of float32, 0
and 8 functionals, the spectrum written or not into guarded buffers, the hand-built problems of tests/nnls_cases.py (a
first insertion that leaves, a banned column, the step limit), plane offsets beyond 2^31, the refusals that need the
device, fit_volume_nnls and the CLI.  Every test needs the entry points this stage adds: without them the whole file fails.
(BREAKDOWN is not reached by any case here: no input is known that makes a kept row's pivot fail.)"""
import ctypes as C
import os

import numpy as np
import pytest

import nnls_cases as K
from fetal_t2mapping_amd import _abi, _nnls as N

pytestmark = pytest.mark.gpu

CHUNK = _abi.NNLS_CHUNK  # voxels a wave takes per counter increment


@pytest.fixture(scope="module")
def t2():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X")
    import fetal_t2mapping_amd as t2
    from fetal_t2mapping_amd._gpu import require

    require(*_abi.NNLS_SYMBOLS)  # the feature: a library without these entry points fails every test here
    return t2


def _same(got, want, what, keys=("x", "func", "amp", "rmse", "nit", "status")):
    for k in keys:
        g, w = got[k].cpu().numpy(), want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g.reshape(-1).view(np.uint32) != w.reshape(-1).view(np.uint32))
        assert bad.size == 0, (what, k, bad.size, bad[:5], g.reshape(-1)[bad[:5]], w.reshape(-1)[bad[:5]])


def _check(t2, y, b, mask, what, want=None, **kw):
    want = N.solve(y, b, mask) if want is None else want
    first = t2.spectrum.solve(y, b, mask, spectrum=True, **kw)
    _same(first, want, what)
    again = t2.spectrum.solve(y, b, mask, spectrum=True, **kw)
    for k in first:
        assert first[k].cpu().numpy().tobytes() == again[k].cpu().numpy().tobytes(), (what, k, "call to call")
    return want


@pytest.mark.parametrize("n_te,n_basis", [(2, 2), (3, 3), (2, 64), (32, 2), (8, 17), (8, 40), (31, 63), (32, 64), (3, 40), (31, 17)])
def test_shapes(t2, n_te, n_basis):
    b = K.basis(n_te, n_basis, 1e-3)
    edge, _ = K.edge_voxels(n_te)
    y = np.concatenate([K.decays(n_te, 61, seed=n_te * 100 + n_basis), edge], axis=1)
    want = _check(t2, y, b, K.holes_mask(y.shape[1], n_basis), f"n_te {n_te} n_basis {n_basis}")
    assert (want["status"] == N.ST_OK).sum() > 40 and want["nit"].max() > 1


def _flight(n_basis):
    from fetal_t2mapping_amd import _gpu_nnls

    return _gpu_nnls.workgroup_waves(n_basis) * CHUNK  # voxels a workgroup has taken when every wave holds a chunk


@pytest.mark.parametrize("which", ["1", "chunk-1", "chunk", "chunk+1", "flight-1", "flight", "flight+1", "refetch"])
def test_voxel_counts(t2, which):
    """Counts named from the kernel's constants.  `refetch`: the persistent grid is capped at two workgroups and the volume
    holds three chunks for each of their waves and a ragged one, so that waves come back to the counter."""
    from fetal_t2mapping_amd import _gpu_nnls

    n_basis = 17
    b = K.basis(3, n_basis, 1e-3)
    waves = _gpu_nnls.workgroup_waves(n_basis)
    n_vox = {"1": 1, "chunk-1": CHUNK - 1, "chunk": CHUNK, "chunk+1": CHUNK + 1, "flight-1": _flight(n_basis) - 1, "flight": _flight(n_basis),
             "flight+1": _flight(n_basis) + 1, "refetch": 2 * waves * CHUNK * 3 + 5}[which]
    mask = None if which != "refetch" else K.holes_mask(n_vox, 4)
    y, want = K.tiled(K.decays(3, 96, seed=17), b, n_vox, mask)
    kw = {"solver_params": _gpu_nnls.params(max_blocks=2)} if which == "refetch" else {}
    _check(t2, y, b, mask, f"{which}: {n_vox} voxels", want=want, **kw)


@pytest.mark.parametrize("mu", K.MUS)
def test_regularisation(t2, mu):
    b = K.basis(8, 40, mu)
    y = K.decays(8, 96, seed=40)
    stats = []
    want = N.solve(y, b, None, stats=stats)
    _check(t2, y, b, None, f"mu {mu}", want=want)
    if mu < K.MUS[-1]:
        assert sum(s["removals"] > 0 for s in stats) >= 48  # the removal path is hot
    else:
        assert any(s["max_p"] == 40 for s in stats)  # the passive set fills: no cap below n_basis is safe


def test_the_largest_problem_with_a_large_passive_set(t2):
    b = K.basis(32, 64, 1e-1)
    y = K.decays(32, 24, seed=1007)
    stats = []
    want = N.solve(y, b, None, stats=stats)
    _check(t2, y, b, None, "32 x 64, mu 0.1", want=want)
    assert max(s["max_p"] for s in stats) >= 40 and want["nit"].max() >= 40


def test_masks_with_empty_and_full_chunks(t2):
    b = K.basis(8, 17, 1e-3)
    n_vox = 20 * CHUNK + 7
    mask = K.holes_mask(n_vox, 9)
    mask[CHUNK:2 * CHUNK] = 0            # an empty chunk
    mask[2 * CHUNK:3 * CHUNK] = 1        # a full one
    mask[4 * CHUNK:4 * CHUNK + _flight(17)] = 0  # nothing for a whole workgroup's worth of chunks
    mask[-7:] = 0                        # the ragged last chunk is empty
    y, want = K.tiled(K.decays(8, 128, seed=90), b, n_vox, mask)
    _check(t2, y, b, mask, "masks", want=want)
    none = np.zeros(n_vox, np.uint8)
    out = t2.spectrum.solve(y, b, none, spectrum=True)
    assert bool((out["status"] == N.ST_MASKED).all()) and not bool(out["x"].any()) and not bool(out["func"].any())
    assert not bool(out["amp"].any()) and not bool(out["rmse"].any()) and not bool(out["nit"].any())


@pytest.mark.parametrize("mu", [0.0, 1e-3])
def test_edge_voxels(t2, mu):
    b = K.basis(8, 40, mu)
    y, names = K.edge_voxels(8)
    want = _check(t2, y, b, None, f"edge voxels, mu {mu}")
    st = dict(zip(names, want["status"]))
    assert st["nan"] == st["inf"] == st["minus_inf_last"] == N.ST_NONFINITE and st["zeros"] == st["negative"] == st["huge"] == N.ST_OK
    at = names.index
    assert want["nit"][at("zeros")] == 0 and want["nit"][at("negative")] == 0 and want["nit"][at("minus_zero")] == 0
    assert want["amp"][at("huge")] > 1e38 and want["amp"][at("subnormal")] > 0 and want["rmse"][at("negative")] > 0


@pytest.mark.parametrize("n_func", [0, 8])
def test_functional_counts(t2, n_func):
    b = K.basis(8, 40, 1e-3, n_func)
    y = K.decays(8, 70, seed=8 + n_func)
    want = _check(t2, y, b, K.holes_mask(70, n_func), f"{n_func} functionals")
    assert want["func"].shape == (n_func, 70) and (n_func == 0 or np.all(np.any(want["func"] != 0, axis=1)))


def test_hand_built_problems_and_the_step_limit(t2):
    from fetal_t2mapping_amd import _gpu_nnls

    for name, A, y, mu in (("first leaves", K.FIRST_LEAVES_A, K.FIRST_LEAVES_Y, 0.0), ("ban", K.BAN_A, K.BAN_Y, 0.0),
                           ("by hand", K.HAND_A, K.HAND_Y, K.HAND_MU)):
        b = N.Basis(A, mu, np.ones((1, A.shape[1])), ("sum",))
        want = _check(t2, y[:, None], b, None, name)
        assert want["status"][0] == N.ST_OK
    assert N.solve(K.BAN_Y[:, None], N.Basis(K.BAN_A, 0.0))["x"][:, 0].tolist() == [1.0, 0.0]
    b = K.basis(8, 40, 1e-3)
    y = K.decays(8, 70, seed=3)
    for limit in (1, 5):
        want = N.solve(y, b, None, max_iter=limit)
        _same(t2.spectrum.solve(y, b, None, spectrum=True, solver_params=_gpu_nnls.params(max_iter=limit)), want, f"max_iter {limit}")
        assert (want["status"] == N.ST_MAXITER).sum() > 35 and want["nit"].max() == limit
    want = N.solve(y, b, None, tol_rel=1e-3, piv_rel=1e-4)
    _same(t2.spectrum.solve(y, b, None, spectrum=True, solver_params=_gpu_nnls.params(tol_rel=1e-3, piv_rel=1e-4)), want, "tol_rel, piv_rel")
    assert not np.array_equal(want["nit"], N.solve(y, b, None)["nit"])


def test_mu_and_functionals_replace_the_basis_own(t2):
    b = K.basis(8, 40, 1e-3)
    y = K.decays(8, 40, seed=77)
    W, names = K.functionals(b.t2_grid, 2)
    got = t2.spectrum.solve(y, b, None, mu=1e-2, functionals=(W, names), spectrum=True)
    _same(got, N.solve(y, N.Basis(b.A, 1e-2, W, names)), "mu= and functionals=")
    assert t2.spectrum.solve(y, b, None, mu=1e-3)["func"].shape == (4, 40) and list(b._packed_dev) == ["cuda:0"]  # packed once, kept
    with pytest.raises(ValueError, match="8 echoes|echoes"):
        t2.spectrum.solve(y[:5], b)


GUARD = 0x5A5A5A5A


def test_spectrum_on_and_off_into_guarded_buffers(t2):
    """Raw calls: every output lies between guard words that must stay; with x_dev NULL nothing else changes."""
    import torch

    from fetal_t2mapping_amd import _gpu_nnls
    from fetal_t2mapping_amd._gpu import current_stream
    from fetal_t2mapping_amd._lib import load

    lib = load()
    b = K.basis(8, 17, 1e-3, 3)
    n_vox = 2 * CHUNK + 3
    y = K.decays(8, n_vox, seed=5)
    mask = K.holes_mask(n_vox, 6)
    want = N.solve(y, b, mask)
    dev = torch.device("cuda", 0)
    packed = torch.from_numpy(_gpu_nnls.pack(b)).to(dev)
    yd, md = torch.from_numpy(y).to(dev), torch.from_numpy(mask).to(dev)
    pad = 16

    def guarded(n, dtype):
        t = torch.full((n + 2 * pad,), GUARD, dtype=torch.int32, device=dev)
        return t, t[pad:pad + n].view(dtype)

    p = _gpu_nnls.params()
    for with_x in (True, False):
        bufs = {"x": guarded(17 * n_vox, torch.float32), "func": guarded(3 * n_vox, torch.float32), "amp": guarded(n_vox, torch.float32),
                "rmse": guarded(n_vox, torch.float32), "nit": guarded(n_vox, torch.int32), "status": guarded(n_vox, torch.int32)}
        rc = lib.t2fit_nnls_dev(C.byref(p), yd.data_ptr(), 8, n_vox, md.data_ptr(), packed.data_ptr(), bufs["x"][1].data_ptr() if with_x else None,
                                bufs["func"][1].data_ptr(), bufs["amp"][1].data_ptr(), bufs["rmse"][1].data_ptr(), bufs["nit"][1].data_ptr(),
                                bufs["status"][1].data_ptr(), current_stream())
        assert rc == _abi.OK, lib.t2fit_last_error()
        torch.cuda.synchronize()
        for k, (whole, view) in bufs.items():
            assert bool((whole[:pad] == GUARD).all()) and bool((whole[-pad:] == GUARD).all()), (k, with_x)
            if k == "x" and not with_x:
                assert bool((whole == GUARD).all())
                continue
            assert view.cpu().numpy().tobytes() == want[k].tobytes(), (k, with_x)


def test_refusals_that_read_the_header(t2):
    import torch

    from fetal_t2mapping_amd import _gpu_nnls
    from fetal_t2mapping_amd._gpu import current_stream
    from fetal_t2mapping_amd._lib import load

    lib = load()
    dev = torch.device("cuda", 0)
    b = K.basis(8, 17, 1e-3, 3)
    good = _gpu_nnls.pack(b)
    y = torch.zeros(8 * 10, device=dev)
    f32 = lambda n: torch.full((n,), 7.0, dtype=torch.float32, device=dev)
    i32 = lambda n: torch.full((n,), 7, dtype=torch.int32, device=dev)
    outs = (f32(170), f32(30), f32(10), f32(10), i32(10), i32(10))
    p = _gpu_nnls.params()

    def call(block, n_te=8, func=True):
        t = torch.from_numpy(block).to(dev)
        return lib.t2fit_nnls_dev(C.byref(p), y.data_ptr(), n_te, 10, None, t.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr() if func else None,
                                  *(o.data_ptr() for o in outs[2:]), current_stream())

    err = lambda: lib.t2fit_last_error().decode()
    bad = good.copy()
    bad[0] ^= 1
    assert call(bad) == _abi.E_INVALID and "magic" in err()
    assert call(good, n_te=7) == _abi.E_INVALID and "n_te 8" in err()
    bad = good.copy()
    bad[8:12] = np.frombuffer(np.int32(65).tobytes(), np.uint8)  # n_basis
    assert call(bad) == _abi.E_INVALID and "out of range" in err()
    bad = good.copy()
    bad[32:40] = np.frombuffer(np.uint64(1 << 20).tobytes(), np.uint8)  # off_g
    assert call(bad) == _abi.E_INVALID and "header" in err()
    bad = good.copy()
    bad[16:24] = np.frombuffer(np.float64(-1.0).tobytes(), np.uint8)  # mu
    assert call(bad) == _abi.E_INVALID and "header" in err()
    assert call(good, func=False) == _abi.E_INVALID and "func_dev" in err()
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)  # nothing was launched
    assert call(good) == _abi.OK
    torch.cuda.synchronize()
    assert bool((outs[5] == 0).all()) and not bool(outs[2].any())  # all-zero voxels: status 0, amp 0


def test_plane_offsets_beyond_2_31(t2):
    """64 planes of 2^25 + 2^20 + 3 voxels: the last plane of x starts beyond 2^31 elements.  All but five voxels are outside the mask."""
    import torch

    n_vox = (1 << 25) + (1 << 20) + 3
    b = K.basis(2, 64, 1e-2, 1)
    assert 63 * n_vox > 1 << 31
    where = np.array([0, 1, n_vox // 2, n_vox - 2, n_vox - 1])
    ys = K.decays(2, 5, seed=31)
    want = N.solve(ys, b)
    dev = torch.device("cuda", 0)
    y = torch.zeros((2, n_vox), dtype=torch.float32, device=dev)
    mask = torch.zeros(n_vox, dtype=torch.uint8, device=dev)
    idx = torch.from_numpy(where).to(dev)
    y[:, idx] = torch.from_numpy(ys).to(dev)
    mask[idx] = 1
    out = t2.spectrum.solve(y, b, mask, spectrum=True)
    _same({k: v[..., idx] for k, v in out.items()}, want, "beyond 2^31")
    assert int((out["status"] == N.ST_MASKED).sum()) == n_vox - 5 and int((out["x"] != 0).sum()) == int((want["x"] != 0).sum())
    assert int((out["amp"] != 0).sum()) == 5 and int((out["func"] != 0).sum()) == 5 and int((out["nit"] != 0).sum()) == 5


def _ulps(a, b):
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and np.all(a >= 0) and np.all(b >= 0)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))  # (not negative: the bit patterns are ordered)


SHAPE = (12, 10, 9)


def test_fit_volume_nnls_against_the_statement(t2):
    import torch

    from fetal_t2mapping_amd import synth

    echoes, mask, te = synth.brain_volume(SHAPE, 6, seed=synth.SEED_BASE, low_field=True)
    echoes = np.asarray(echoes, np.float32)
    echoes[2, 3, 4, 5] = np.nan
    mask[3, 4, 5] = 1
    b = t2.spectrum.spectrum_basis(te, t2.spectrum.log_grid(10.0, 2000.0, 40), windows={"csf": (600.0, 2000.0), "short": (10.0, 50.0)})
    assert b.mu == t2.spectrum.DEFAULT_MU and b.names == ("lnT2", "csf", "short")
    want = N.solve(echoes, b, mask)
    d = N.derived(want["func"], want["amp"], b.names)
    maps, extras = t2.spectrum.fit_volume_nnls(echoes, mask, b, spectrum=True)
    assert isinstance(maps, t2.T2Maps) and set(extras) == {"csffraction", "shortfraction", "nnlsiter", "nnlsstatus", "t2spectrum"}
    assert maps.k.tobytes() == want["amp"].tobytes() and maps.res.tobytes() == want["rmse"].tobytes() and not maps.sigma.any()
    assert extras["nnlsiter"].tobytes() == want["nit"].tobytes() and extras["nnlsstatus"].tobytes() == want["status"].tobytes()
    assert extras["t2spectrum"].shape == (40,) + SHAPE and extras["t2spectrum"].tobytes() == want["x"].tobytes()
    assert _ulps(maps.t2, d["gmt2"]).max() <= 1 and _ulps(extras["csffraction"], d["csffraction"]).max() <= 1
    assert _ulps(extras["shortfraction"], d["shortfraction"]).max() <= 1
    fitted = want["status"] == N.ST_OK
    assert fitted.sum() > 200 and np.all(maps.t2[fitted] >= 10.0 * (1 - 1e-6)) and np.all(maps.t2[fitted] <= 2000.0 * (1 + 1e-6))
    assert np.all(maps.t2[mask == 0] == 0) and float(np.median(extras["csffraction"][fitted])) < 0.5
    status = np.where(want["status"] == N.ST_OK, _abi.ST_CONVERGED, np.where(want["status"] == N.ST_MASKED, _abi.ST_MASKED,
                      np.where(want["status"] == N.ST_NONFINITE, _abi.ST_NONFINITE, _abi.ST_NOT_CONV))).astype(np.uint8)
    assert np.array_equal(maps.status, status) and status[3, 4, 5] == _abi.ST_NONFINITE
    plain, fewer = t2.spectrum.fit_volume_nnls(echoes, mask, b)
    assert "t2spectrum" not in fewer and plain.t2.tobytes() == maps.t2.tobytes()
    maps_t, extras_t = t2.spectrum.fit_volume_nnls(torch.from_numpy(echoes).cuda(), torch.from_numpy(mask).cuda(), b)
    assert maps_t.t2.is_cuda and maps_t.t2.cpu().numpy().tobytes() == maps.t2.tobytes()
    with pytest.raises(ValueError, match="lnT2"):
        t2.spectrum.fit_volume_nnls(echoes, mask, N.Basis(b.A, b.mu))


def _tree(tmp_path):
    """A tiny BIDS tree: three echoes of a synthetic brain volume and their masks."""
    import pandas as pd

    from fetal_t2mapping_amd import cli as R
    from fetal_t2mapping_amd import nifti, synth

    echoes, mask, te = synth.brain_volume(SHAPE, 3, seed=synth.SEED_BASE, low_field=True)
    root = str(tmp_path)
    bids = os.path.join(root, "projects") + "/"
    os.makedirs(os.path.join(bids, "prj-906"))
    os.makedirs(os.path.join(root, "dicom", "logs"))
    rows = []
    for i, t in enumerate(te):
        acq = {"prj": "prj-906", "sub": "sub-007", "ses": "ses-01", "run": f"run-{i + 1:02d}", "EchoTime": t / 1000.0, "CoilString": "HeadNeck"}
        rows.append(acq)
        for arr, dirname in ((echoes[i], R.recon_dirname), (mask, R.mask_dirname)):
            nifti.WriteImage(nifti.GetImageFromArray(arr), R.get_img_path(bids, acq, dirname).replace(" ", ""))
    pd.DataFrame(rows).to_csv(os.path.join(root, "dicom", "logs", "log.csv"), index=False)
    out_dir = os.path.join(bids, "prj-906", "derivatives", R.t2map_dirname, "sub-007", "ses-01", "anat")
    return root, out_dir, np.asarray(echoes, np.float32), mask, te


def _read(out_dir, tag, series=False):
    from fetal_t2mapping_amd import nifti

    name = [f for f in os.listdir(out_dir) if f"_{tag}map_" in f]
    assert len(name) == 1, (tag, os.listdir(out_dir))
    return nifti.ReadImage(os.path.join(out_dir, name[0]), series=series).arr


def test_cli_writes_the_maps_of_the_statement(t2, tmp_path, monkeypatch):
    import sys

    from fetal_t2mapping_amd import cli as R

    monkeypatch.setitem(sys.modules, "SimpleITK", None)
    tags = lambda out: sorted(f.split("_ada-")[0].split("_")[-1] for f in os.listdir(out))

    def run(name, extra):
        root, out, echoes, mask, te = _tree(tmp_path / name)
        base = ["--csv", "log.csv", "--in_vivo", "--gaussian", "--lf", "--sim", "n1", "--TEs"] + [str(int(t)) for t in te]
        R.main(["--path", root] + base + extra)
        return out, echoes, mask, te

    out, echoes, mask, te = run("plain", ["--solver", "nnls", "--nnls_t2", "10:2000:40"])
    union = t2.stack_mask_flatten(list(echoes), [mask] * 3)[1]
    b = t2.spectrum.spectrum_basis(te, N.log_grid(10.0, 2000.0, 40), R.NNLS_DEFAULT_MU)
    want = N.solve(echoes, b, union)
    assert tags(out) == ["kmap", "nnlsitermap", "nnlsstatusmap", "resmap", "sigmamap", "t2map"]
    assert _read(out, "k").tobytes() == want["amp"].tobytes() and _read(out, "res").tobytes() == want["rmse"].tobytes()
    assert not _read(out, "sigma").any() and _ulps(_read(out, "t2"), N.derived(want["func"], want["amp"], b.names)["gmt2"]).max() <= 1
    nit, status = _read(out, "nnlsiter"), _read(out, "nnlsstatus")
    assert nit.dtype == np.int32 and nit.tobytes() == want["nit"].tobytes() and status.tobytes() == want["status"].tobytes()
    assert (want["status"] == N.ST_OK).sum() > 100

    out, echoes, mask, te = run("windows", ["--solver", "nnls", "--nnls_t2", "20:1500:24", "--nnls_mu", "0.1", "--nnls_window", "csf=600:1500",
                                            "--nnls_window", "short=20:60", "--write_spectrum"])
    b = t2.spectrum.spectrum_basis(te, N.log_grid(20.0, 1500.0, 24), 0.1, {"csf": (600.0, 1500.0), "short": (20.0, 60.0)})
    want = N.solve(echoes, b, union)
    d = N.derived(want["func"], want["amp"], b.names)
    assert tags(out) == ["csffractionmap", "kmap", "nnlsitermap", "nnlsstatusmap", "resmap", "shortfractionmap", "sigmamap", "t2map", "t2spectrummap"]
    assert _read(out, "k").tobytes() == want["amp"].tobytes() and _ulps(_read(out, "t2"), d["gmt2"]).max() <= 1
    assert _ulps(_read(out, "csffraction"), d["csffraction"]).max() <= 1 and _ulps(_read(out, "shortfraction"), d["shortfraction"]).max() <= 1
    spectrum = _read(out, "t2spectrum", series=True)
    assert spectrum.shape == (24,) + SHAPE and spectrum.tobytes() == want["x"].tobytes()
