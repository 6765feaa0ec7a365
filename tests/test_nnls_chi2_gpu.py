"""The chi^2 rule of the T2-spectrum fit on the device (csrc/t2fit_nnls.hip: nnls_kernel<true>, t2fit_nnls_chi2_dev) against
its numpy statement (fetal_t2mapping_amd/_nnls.py: solve_chi2): x, every functional, amp, rmse, nit, status, mu, ratio, solves
and rule bit for bit on every voxel, and equal from call to call, over basis and echo counts, voxel counts around a chunk
and around the voxels a workgroup takes at once and several chunks per wave of a capped grid, the parameter sets that
reach each rule code (tests/nnls_chi2_cases.py), no bisection, no growth, a step limit, masks with empty and full chunks,
edge voxels with non-finite samples, raw calls into guarded buffers with the spectrum written or not, the refusals that read
the header (a packed mu that is not 0 among them), fit_volume_nnls(chi2=...) and the CLI.  The statement runs on at most
48 distinct voxels per case and is tiled."""
import ctypes as C
import os

import numpy as np
import pytest

import nnls_chi2_cases as Q
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

    require(*_abi.NNLS_CHI2_SYMBOLS)  # the feature: a library without these entry points fails every test here
    return t2


def _same(got, want, what, keys=Q.OUTPUTS):
    for k in keys:
        g, w = got[k].cpu().numpy(), want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g.reshape(-1).view(np.uint32) != w.reshape(-1).view(np.uint32))
        assert bad.size == 0, (what, k, bad.size, bad[:5], g.reshape(-1)[bad[:5]], w.reshape(-1)[bad[:5]])


def _check(t2, n_vox, mask, what, n_func=4, solver_params=None, **case):
    """The device on `n_vox` tiled voxels of the case against the statement, twice."""
    from fetal_t2mapping_amd import _gpu_nnls

    y, want = Q.tiled(n_vox, mask, n_func=n_func, **case)
    b = K.basis(case["n_te"], case["n_basis"], 0.0, n_func)
    chi2 = _gpu_nnls.chi2_params(**Q.PARAMS[case.get("params", "default")][0])
    if case.get("max_iter"):
        solver_params = _gpu_nnls.params(max_iter=case["max_iter"])
    kw = {"spectrum": True, "chi2": chi2, "solver_params": solver_params}
    first = t2.spectrum.solve_chi2(y, b, mask, **kw)
    _same(first, want, what)
    again = t2.spectrum.solve_chi2(y, b, mask, **kw)
    for k in first:
        assert first[k].cpu().numpy().tobytes() == again[k].cpu().numpy().tobytes(), (what, k, "call to call")
    return want


@pytest.mark.parametrize("n_te,n_basis,n_unique", [(2, 2, 48), (3, 17, 48), (8, 40, 48), (31, 63, 16), (32, 64, 16)])
def test_shapes(t2, n_te, n_basis, n_unique):
    n_vox = 2 * CHUNK + 9
    want = _check(t2, n_vox, K.holes_mask(n_vox, n_basis), f"n_te {n_te} n_basis {n_basis}", n_te=n_te, n_basis=n_basis, kind="edge",
                  n_unique=n_unique, seed=n_te * 100 + n_basis)
    assert (want["status"] == N.ST_OK).sum() > 60 and (want["status"] == N.ST_NONFINITE).sum() >= 3 and want["solves"].max() >= 2
    if n_te >= 8:
        assert (want["rule"] == N.RULE_FOUND).sum() > 20 and want["solves"].max() >= 10


def _flight(n_basis):
    from fetal_t2mapping_amd import _gpu_nnls

    return _gpu_nnls.workgroup_waves(n_basis) * CHUNK  # voxels a workgroup has taken when every wave holds a chunk


@pytest.mark.parametrize("which", ["1", "chunk-1", "chunk", "chunk+1", "flight-1", "flight", "flight+1", "refetch"])
def test_voxel_counts(t2, which):
    """Counts named from the kernel's constants.  `refetch`: the persistent grid is capped at two workgroups and the volume
    holds three chunks for each of their waves and a ragged one, so that waves come back to the counter.  Three echoes
    and 17 columns: exact fits (two solves) and bisected ones (ten and more) side by side, so the waves' voxels differ in cost."""
    from fetal_t2mapping_amd import _gpu_nnls

    n_basis = 17
    waves = _gpu_nnls.workgroup_waves(n_basis)
    n_vox = {"1": 1, "chunk-1": CHUNK - 1, "chunk": CHUNK, "chunk+1": CHUNK + 1, "flight-1": _flight(n_basis) - 1, "flight": _flight(n_basis),
             "flight+1": _flight(n_basis) + 1, "refetch": 2 * waves * CHUNK * 3 + 5}[which]
    mask = None if which != "refetch" else K.holes_mask(n_vox, 4)
    sp = _gpu_nnls.params(max_blocks=2) if which == "refetch" else None
    want = _check(t2, n_vox, mask, f"{which}: {n_vox} voxels", solver_params=sp, n_te=3, n_basis=n_basis, kind="noisy", n_unique=48, seed=17)
    if n_vox >= 48:
        assert {N.RULE_EXACT, N.RULE_FOUND} <= set(want["rule"].tolist())


@pytest.mark.parametrize("params", sorted(Q.PARAMS))
def test_rules_and_parameters(t2, params):
    """Every parameter set of the host tests on 8 x 40; `default` bisects five times, `no_bisect` not at all."""
    kind = "noisier" if params == "other" else "noisy"
    want = _check(t2, 70, None, params, n_te=8, n_basis=40, kind=kind, n_unique=35, seed=5, params=params)
    rule = Q.PARAMS[params][1]
    if rule is not None:
        assert (want["rule"] == rule).sum() >= 50
    else:
        assert len(set(want["rule"].tolist())) >= 2


def test_exact_fits_and_the_step_limit(t2):
    want = _check(t2, 70, None, "exact decays", n_te=8, n_basis=40, kind="exact", n_unique=35, seed=5)
    assert (want["rule"] == N.RULE_EXACT).sum() >= 35 and np.all(want["mu"][want["rule"] == N.RULE_EXACT] == np.float32(0.03))
    want = _check(t2, 70, None, "max_iter 12", n_te=8, n_basis=40, kind="noisy", n_unique=35, seed=5, max_iter=12)
    assert (want["status"] == N.ST_MAXITER).sum() >= 35 and (want["status"] == N.ST_OK).sum() >= 1 and want["nit"].max() > 12
    want = _check(t2, 70, None, "max_iter 1", n_te=8, n_basis=40, kind="noisy", n_unique=35, seed=5, max_iter=1)
    assert np.all(want["status"] == N.ST_MAXITER) and np.all(want["nit"] == want["solves"])


@pytest.mark.parametrize("n_func", [0, 8])
def test_functional_counts(t2, n_func):
    want = _check(t2, 70, K.holes_mask(70, n_func), f"{n_func} functionals", n_func=n_func, n_te=8, n_basis=40, kind="noisy", n_unique=24, seed=9)
    assert want["func"].shape == (n_func, 70) and (n_func == 0 or np.all(np.any(want["func"] != 0, axis=1)))


def test_masks_with_empty_and_full_chunks(t2):
    n_vox = 20 * CHUNK + 7
    mask = K.holes_mask(n_vox, 9)
    mask[CHUNK:2 * CHUNK] = 0            # an empty chunk
    mask[2 * CHUNK:3 * CHUNK] = 1        # a full one
    mask[4 * CHUNK:4 * CHUNK + _flight(17)] = 0  # nothing for a whole workgroup's worth of chunks
    mask[-7:] = 0                        # the ragged last chunk is empty
    case = dict(n_te=8, n_basis=17, kind="edge", n_unique=48, seed=90)
    _check(t2, n_vox, mask, "masks", **case)
    y, _ = Q.tiled(n_vox, **case)
    out = t2.spectrum.solve_chi2(y, K.basis(8, 17, 0.0), np.zeros(n_vox, np.uint8), spectrum=True)
    assert bool((out["status"] == N.ST_MASKED).all()) and bool((out["rule"] == N.RULE_NONE).all())
    assert not any(bool(out[k].any()) for k in Q.OUTPUTS if k not in ("status", "rule"))


def test_edge_voxels(t2):
    """K.edge_voxels alone, in their order: zeros, negative, NaN, Inf, -Inf in the last echo, the ends of float32, -0.0, one sample."""
    y, names = K.edge_voxels(8)
    b = K.basis(8, 40, 0.0)
    want = N.solve_chi2(y, b)
    got = t2.spectrum.solve_chi2(y, b, spectrum=True)
    _same(got, want, "edge voxels")
    st, rule = dict(zip(names, want["status"])), dict(zip(names, want["rule"]))
    assert st["nan"] == st["inf"] == st["minus_inf_last"] == N.ST_NONFINITE and rule["nan"] == rule["inf"] == rule["minus_inf_last"] == N.RULE_NONE
    assert rule["zeros"] == rule["minus_zero"] == N.RULE_EXACT and rule["negative"] == N.RULE_HIGH and st["huge"] == st["subnormal"] == N.ST_OK
    assert want["amp"][names.index("huge")] > 1e38 and np.isfinite(want["ratio"]).all()


def test_a_basis_with_a_weight_is_repacked_at_zero(t2):
    y, want = Q.tiled(40, n_te=8, n_basis=40, kind="noisy", n_unique=35, seed=5)
    b = K.basis(8, 40, 1e-1)
    got = t2.spectrum.solve_chi2(y, b, spectrum=True)
    _same(got, want, "mu 0.1 repacked")
    assert b._mu0.mu == 0.0 and list(b._mu0._packed_dev) == ["cuda:0"] and t2.spectrum.solve_chi2(y, b)["mu"].shape == (40,)  # packed once, kept
    W, names = K.functionals(b.t2_grid, 2)
    got = t2.spectrum.solve_chi2(y, b, functionals=(W, names), spectrum=True)
    _same(got, {**want, "func": want["func"][:2]}, "functionals=")  # (the first two of the four the case was stated with)
    with pytest.raises(ValueError, match="echoes"):
        t2.spectrum.solve_chi2(y[:5], b)


GUARD = 0x5A5A5A5A


def test_raw_calls_into_guarded_buffers(t2):
    """Every output lies between guard words that must stay; with x_dev NULL nothing else changes."""
    import torch

    from fetal_t2mapping_amd import _gpu_nnls
    from fetal_t2mapping_amd._gpu import current_stream
    from fetal_t2mapping_amd._lib import load

    lib = load()
    n_vox = 2 * CHUNK + 3
    mask = K.holes_mask(n_vox, 6)
    y, want = Q.tiled(n_vox, mask, n_te=8, n_basis=17, kind="edge", n_unique=48, seed=90, n_func=3)
    b = K.basis(8, 17, 0.0, 3)
    dev = torch.device("cuda", 0)
    packed = torch.from_numpy(_gpu_nnls.pack(b)).to(dev)
    yd, md = torch.from_numpy(y).to(dev), torch.from_numpy(mask).to(dev)
    pad = 16

    def guarded(n, dtype):
        t = torch.full((n + 2 * pad,), GUARD, dtype=torch.int32, device=dev)
        return t, t[pad:pad + n].view(dtype)

    p, c = _gpu_nnls.params(), _gpu_nnls.chi2_params()
    f32, i32 = torch.float32, torch.int32
    for with_x in (True, False):
        bufs = {"x": guarded(17 * n_vox, f32), "func": guarded(3 * n_vox, f32), "amp": guarded(n_vox, f32), "rmse": guarded(n_vox, f32),
                "nit": guarded(n_vox, i32), "status": guarded(n_vox, i32), "mu": guarded(n_vox, f32), "ratio": guarded(n_vox, f32),
                "solves": guarded(n_vox, i32), "rule": guarded(n_vox, i32)}
        ptr = {k: v[1].data_ptr() for k, v in bufs.items()}
        rc = lib.t2fit_nnls_chi2_dev(C.byref(p), C.byref(c), yd.data_ptr(), 8, n_vox, md.data_ptr(), packed.data_ptr(), ptr["x"] if with_x else None,
                                     *(ptr[k] for k in Q.OUTPUTS[1:]), current_stream())
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
    good = _gpu_nnls.pack(K.basis(8, 17, 0.0, 3))
    y = torch.zeros(8 * 10, device=dev)
    f32 = lambda n: torch.full((n,), 7.0, dtype=torch.float32, device=dev)
    i32 = lambda n: torch.full((n,), 7, dtype=torch.int32, device=dev)
    outs = (f32(170), f32(30), f32(10), f32(10), i32(10), i32(10), f32(10), f32(10), i32(10), i32(10))
    p, c = _gpu_nnls.params(), _gpu_nnls.chi2_params()

    def call(block, n_te=8, func=True):
        t = torch.from_numpy(block).to(dev)
        return lib.t2fit_nnls_chi2_dev(C.byref(p), C.byref(c), y.data_ptr(), n_te, 10, None, t.data_ptr(), outs[0].data_ptr(),
                                       outs[1].data_ptr() if func else None, *(o.data_ptr() for o in outs[2:]), current_stream())

    err = lambda: lib.t2fit_last_error().decode()
    bad = good.copy()
    bad[0] ^= 1
    assert call(bad) == _abi.E_INVALID and "magic" in err() and "t2fit_nnls_chi2_dev" in err()
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
    assert call(_gpu_nnls.pack(K.basis(8, 17, 1e-3, 3))) == _abi.E_INVALID and "needs mu 0" in err()  # the rule owns the weight
    assert call(good, func=False) == _abi.E_INVALID and "func_dev" in err()
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)  # nothing was launched
    assert call(good) == _abi.OK
    torch.cuda.synchronize()
    # all-zero voxels: an exact fit, two solves without a step
    assert bool((outs[5] == 0).all()) and not bool(outs[2].any()) and bool((outs[9] == N.RULE_EXACT).all()) and bool((outs[8] == 2).all())


def _ulps(a, b):
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and np.all(a >= 0) and np.all(b >= 0)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))  # (not negative: the bit patterns are ordered)


def test_fit_volume_nnls_against_the_statement(t2):
    """A (4, 5, 6) volume of 40 distinct decays, a mask with holes and a NaN sample; with and without the rule."""
    import torch

    shape = (4, 5, 6)
    te = K.echo_times(8)
    unique = K.decays(8, 40, seed=12)
    echoes = np.ascontiguousarray(unique[:, np.arange(120) % 40]).reshape((8,) + shape)
    mask = K.holes_mask(120, 2).reshape(shape)
    echoes[2, 1, 2, 3] = np.nan
    mask[1, 2, 3] = 1
    b = t2.spectrum.spectrum_basis(te, t2.spectrum.log_grid(10.0, 2000.0, 40), windows={"csf": (600.0, 2000.0)})
    assert b.mu == t2.spectrum.DEFAULT_MU
    ref = N.solve_chi2(unique, b.with_mu(0.0), factor=1.05)
    want = {k: np.ascontiguousarray(v[..., np.arange(120) % 40]).reshape(v.shape[:-1] + shape) for k, v in ref.items()}
    for k, v in want.items():
        v[..., mask == 0] = {"status": N.ST_MASKED, "rule": N.RULE_NONE}.get(k, 0)
        v[..., 1, 2, 3] = {"status": N.ST_NONFINITE, "rule": N.RULE_NONE}.get(k, 0)
    d = N.derived(want["func"], want["amp"], b.names)
    maps, extras = t2.spectrum.fit_volume_nnls(echoes, mask, b, spectrum=True, chi2={"factor": 1.05})
    assert isinstance(maps, t2.T2Maps)
    assert set(extras) == {"csffraction", "nnlsiter", "nnlsstatus", "t2spectrum", "nnlsmu", "nnlschi2", "nnlsrule", "nnlssolves"}
    assert maps.k.tobytes() == want["amp"].tobytes() and maps.res.tobytes() == want["rmse"].tobytes() and not maps.sigma.any()
    for tag, k, dtype in (("nnlsiter", "nit", np.int32), ("nnlsstatus", "status", np.int32), ("t2spectrum", "x", np.float32),
                          ("nnlsmu", "mu", np.float32), ("nnlschi2", "ratio", np.float32), ("nnlsrule", "rule", np.int32),
                          ("nnlssolves", "solves", np.int32)):
        assert extras[tag].dtype == dtype and extras[tag].tobytes() == want[k].tobytes(), tag
    assert _ulps(maps.t2, d["gmt2"]).max() <= 1 and _ulps(extras["csffraction"], d["csffraction"]).max() <= 1
    assert maps.status[1, 2, 3] == _abi.ST_NONFINITE and np.all(maps.status[mask == 0] == _abi.ST_MASKED)
    assert (want["rule"] == N.RULE_FOUND).sum() > 60
    default, more = t2.spectrum.fit_volume_nnls(echoes, mask, b, chi2=True)  # the library's numbers: what solve_chi2 gives
    direct = t2.spectrum.solve_chi2(echoes, b, mask)
    assert default.k.tobytes() == direct["amp"].cpu().numpy().tobytes() and more["nnlsmu"].tobytes() == direct["mu"].cpu().numpy().tobytes()
    assert more["nnlsmu"].tobytes() != extras["nnlsmu"].tobytes()
    maps_t, extras_t = t2.spectrum.fit_volume_nnls(torch.from_numpy(echoes).cuda(), torch.from_numpy(mask).cuda(), b, chi2={"factor": 1.05})
    assert maps_t.t2.is_cuda and extras_t["nnlsmu"].is_cuda and extras_t["nnlsmu"].cpu().numpy().tobytes() == want["mu"].tobytes()
    # without the rule the call is what it was
    plain, fewer = t2.spectrum.fit_volume_nnls(echoes, mask, b)
    fixed = N.solve(echoes, b, mask)
    assert set(fewer) == {"csffraction", "nnlsiter", "nnlsstatus"} and plain.k.tobytes() == fixed["amp"].tobytes()
    assert fewer["nnlsiter"].tobytes() == fixed["nit"].tobytes()


SHAPE = (8, 7, 6)


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


def _read(out_dir, tag):
    from fetal_t2mapping_amd import nifti

    name = [f for f in os.listdir(out_dir) if f"_{tag}map_" in f]
    assert len(name) == 1, (tag, os.listdir(out_dir))
    return nifti.ReadImage(os.path.join(out_dir, name[0])).arr


def test_cli_writes_the_maps_of_the_statement(t2, tmp_path, monkeypatch):
    import sys

    from fetal_t2mapping_amd import cli as R

    monkeypatch.setitem(sys.modules, "SimpleITK", None)
    root, out, echoes, mask, te = _tree(tmp_path)
    R.main(["--path", root, "--csv", "log.csv", "--in_vivo", "--gaussian", "--lf", "--sim", "n1", "--TEs"] + [str(int(t)) for t in te]
           + ["--solver", "nnls", "--nnls_t2", "10:2000:24", "--nnls_chi2", "1.1", "--nnls_chi2_fallback", "0.05", "--nnls_window", "csf=600:2000"])
    union = t2.stack_mask_flatten(list(echoes), [mask] * 3)[1]
    b = t2.spectrum.spectrum_basis(te, N.log_grid(10.0, 2000.0, 24), 0.0, {"csf": (600.0, 2000.0)})
    want = N.solve_chi2(echoes, b, union, factor=1.1, mu_exact=0.05)
    d = N.derived(want["func"], want["amp"], b.names)
    tags = sorted(f.split("_ada-")[0].split("_")[-1] for f in os.listdir(out))
    assert tags == ["csffractionmap", "kmap", "nnlschi2map", "nnlsitermap", "nnlsmumap", "nnlsrulemap", "nnlssolvesmap", "nnlsstatusmap", "resmap",
                    "sigmamap", "t2map"]
    assert _read(out, "k").tobytes() == want["amp"].tobytes() and _read(out, "res").tobytes() == want["rmse"].tobytes()
    assert _ulps(_read(out, "t2"), d["gmt2"]).max() <= 1 and _ulps(_read(out, "csffraction"), d["csffraction"]).max() <= 1
    for tag, k, dtype in (("nnlsiter", "nit", np.int32), ("nnlsstatus", "status", np.int32), ("nnlsmu", "mu", np.float32),
                          ("nnlschi2", "ratio", np.float32), ("nnlsrule", "rule", np.int32), ("nnlssolves", "solves", np.int32)):
        arr = _read(out, tag)
        assert arr.dtype == dtype and arr.tobytes() == want[k].tobytes(), tag
    fitted = want["rule"] >= 0
    assert fitted.sum() > 50 and set(want["rule"][fitted].tolist()) <= {0, 1, 2, 3} and np.all(want["mu"][want["rule"] == N.RULE_EXACT] == np.float32(0.05))
