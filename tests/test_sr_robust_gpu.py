"""The outlier weighting of the super-resolution loop on the device (csrc/t2fit_sr_robust.hip) against its numpy statement
(fetal_t2mapping_amd/_sr.py robust_step), bit for bit on sums, slice weights, sigma2 and the residual: slices of 1, 35, 256,
257 and 21 x 19 samples, 1 and 5 echoes, masks with holes, N with zeros, empty / barely eligible / tied slices, non-finite
samples, the floor, robustness off, six stacks; the raw entry point on offset pointers into guarded buffers, on a second
stream, twice, and every refusal; ``reconstruct_sr(robust=...)`` stack-wise and with a pose per slice against the statement;
the four conditions on the corrupted phantom from device runs; ``reconstruct_svr(robust=True)``; recon.py --sr_robust.
tests/test_sr_robust_host.py covers what needs no device."""
import ctypes as C
import os

import numpy as np
import pytest

import sr_cases as K
import sr_robust_cases as RC
import svr_cases as W
from fetal_t2mapping_amd import _sr as S
from fetal_t2mapping_amd import _svr as V
from test_recon_gpu import GUARD, SENTINEL, _bits_equal, _guarded, _payload, _write_subject
from test_sr_gpu import _guarded64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def t2():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X")
    import fetal_t2mapping_amd as t2

    return t2


def _same_step(got, want):
    for a, b in zip(got[0], want[0]):
        assert RC.same_bits(a, b)
    for a, b in zip(got[1], want[1]):
        assert RC.same_bits(a, b)
    assert RC.same_bits(got[2], want[2]) and RC.same_bits(got[3], want[3])


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_the_step_equals_the_statement_bit_for_bit(t2, name):
    r, N, masks, params, ref = RC.case(name)
    want = S.robust_step(r, N, masks, params or True)
    _same_step(want, ref)  # the statement is the definition's
    before = [v.copy() for v in r]
    got = t2.sr.sr_robust_weights(r, N, masks=masks, **(params or {}))
    _same_step(got, want)
    assert all(RC.same_bits(a, b) for a, b in zip(r, before))  # the inputs stay as they are
    if name == "edges":
        assert want[2][1] == 0.0 and RC.same_bits(want[0][0][1], r[0][1])  # robustness off: the echo is untouched, NaN and -0.0 too
        assert np.signbit(want[0][0][0]).sum() < np.signbit(r[0][0]).sum()  # -inf became +0.0
    if name == "floor":
        assert np.all(want[2] == 100.0 * 100.0)
    if name == "none_eligible":
        assert np.all(want[2] == 0.0) and all(np.all(w == 1.0) for w in want[1])


def test_tensors_in_give_tensors_out_and_leave_the_inputs(t2):
    import torch

    r, N, masks, params, ref = RC.case("six_stacks")
    rt = [torch.from_numpy(v).cuda() for v in r]
    nt = [torch.from_numpy(v).cuda() for v in N]
    out, weights, sigma2, sums = t2.sr.sr_robust_weights(rt, nt, masks=masks, **params)
    assert all(v.is_cuda for v in out + weights) and sigma2.is_cuda and sums.is_cuda
    _same_step(([v.cpu().numpy() for v in out], [v.cpu().numpy() for v in weights], sigma2.cpu().numpy(), sums.cpu().numpy()), ref)
    assert all(RC.same_bits(a.cpu().numpy(), b) for a, b in zip(rt, r))
    single = t2.sr.sr_robust_weights([r[4][0]], [N[4]], masks=[masks[4]])  # (lz, ly, lx): one echo, the shape kept
    want = S.robust_step([r[4][:1]], [N[4]], [masks[4]], True)
    assert single[0][0].shape == r[4][0].shape and RC.same_bits(single[0][0], want[0][0][0]) and RC.same_bits(single[2], want[2])


def _params(t2, **kw):
    from fetal_t2mapping_amd import _abi
    from fetal_t2mapping_amd._lib import load

    p = _abi.T2FitSrRobustParams()
    assert load().t2fit_sr_robust_params_default(C.byref(p)) == 0
    assert (p.slice_threshold, p.huber, p.sigma_floor, p.min_count, p.flags) == (1.5, 2.5, 0.0, 16, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_raw_call_on_offset_pointers_second_stream_twice_and_refusals(t2):
    import torch

    from fetal_t2mapping_amd._lib import load

    lib = load()
    r, N, masks, params, ref = RC.case("tuned")
    n_vol, n_s = r[0].shape[0], len(r)
    n_slices = sum(v.shape[1] for v in r)
    par = _params(t2, **params)
    P = lambda v: (C.c_void_p * len(v))(*v)
    lo = (C.c_int32 * (3 * n_s))(*[d for v in r for d in v.shape[1:]])
    need = C.c_size_t(0)
    assert lib.t2fit_sr_robust_workspace_bytes(n_s, lo, n_vol, C.byref(need)) == 0
    up = lambda v: (v + 255) // 256 * 256
    assert need.value == up(16 * n_vol * n_slices) + up(8 * n_vol * n_slices) + up(8 * n_vol)
    side = torch.cuda.Stream()
    results = []
    for stream in (torch.cuda.current_stream(), side):
        with torch.cuda.stream(stream):
            rb = [_guarded(v.ravel()) for v in r]
            nb = []
            for v in N:
                buf, ptr, where = _guarded64(v.size)
                buf[where] = torch.from_numpy(v.ravel().view(np.int32)).cuda()
                nb.append((buf, ptr, where))
            mb = [None if m is None else torch.from_numpy(m.ravel().copy()).cuda() for m in masks]
            sb, wb, gb = _guarded64(2 * n_vol * n_slices), _guarded64(n_vol * n_slices), _guarded64(n_vol)
            stream.synchronize()
            rc = lib.t2fit_sr_robust_dev(n_s, P([b[1] for b in rb]), P([b[1] for b in nb]), P([None if m is None else m.data_ptr() for m in mb]),
                                         lo, n_vol, C.byref(par), sb[1], wb[1], gb[1], C.c_void_p(stream.cuda_stream))
            assert rc == 0, lib.t2fit_last_error().decode()
            stream.synchronize()
        got_r = [_payload(b[0], b[2]).view(np.float32).reshape(v.shape) for b, v in zip(rb, r)]
        for b, v in zip(nb, N):
            assert np.array_equal(_payload(b[0], b[2]).view(np.float64), v.ravel())
        sums = _payload(sb[0], sb[2]).view(np.float64).reshape(n_vol, n_slices, 2)
        weights = _payload(wb[0], wb[2]).view(np.float64).reshape(n_vol, n_slices)
        sigma2 = _payload(gb[0], gb[2]).view(np.float64)
        edges = np.cumsum([0] + [v.shape[1] for v in r])
        _same_step((got_r, [weights[:, edges[s]:edges[s + 1]] for s in range(n_s)], sigma2, sums), ref)
        results.append((got_r, weights, sigma2, sums))
    for a, b in zip(results[0][0], results[1][0]):  # twice, to the same bits
        assert RC.same_bits(a, b)
    assert all(RC.same_bits(a, b) for a, b in zip(results[0][1:], results[1][1:]))

    # every refusal comes before HIP is touched: nothing is written
    rb = [_guarded(v.ravel()) for v in r]
    nt = [torch.from_numpy(v).cuda() for v in N]
    sb, wb, gb = _guarded64(2 * n_vol * n_slices), _guarded64(n_vol * n_slices), _guarded64(n_vol)
    rp, npt = [b[1] for b in rb], [t.data_ptr() for t in nt]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(n_s=n_s, r=P(rp), N=P(npt), m=None, lo=lo, n_vol=n_vol, par=C.byref(par), sums=sb[1], w=wb[1], s2=gb[1])
    many = (C.c_int32 * 3)(4097, 2, 2)
    bad = [dict(r=None), dict(N=None), dict(lo=None), dict(par=None), dict(sums=None), dict(w=None), dict(s2=None),
           dict(n_s=0), dict(n_s=7), dict(n_vol=0), dict(lo=(C.c_int32 * (3 * n_s))(*([4, 0, 16] + list(lo)[3:]))),
           dict(n_s=1, lo=many), dict(r=P([None] + rp[1:])), dict(N=P([None] + npt[1:])), dict(r=P([rp[0] + 2] + rp[1:])),
           dict(N=P([npt[0] + 4] + npt[1:])), dict(sums=sb[1] + 4),
           dict(par=C.byref(_params(t2, slice_threshold=0.0))), dict(par=C.byref(_params(t2, slice_threshold=float("nan")))),
           dict(par=C.byref(_params(t2, huber=-1.0))), dict(par=C.byref(_params(t2, huber=float("inf")))),
           dict(par=C.byref(_params(t2, min_count=0))), dict(par=C.byref(_params(t2, sigma_floor=-1.0))),
           dict(par=C.byref(_params(t2, sigma_floor=float("inf")))), dict(par=C.byref(_params(t2, flags=1)))]
    for change in bad:
        a = {**good, **change}
        rc = lib.t2fit_sr_robust_dev(a["n_s"], a["r"], a["N"], a["m"], a["lo"], a["n_vol"], a["par"], a["sums"], a["w"], a["s2"], stream)
        assert rc == -1 and lib.t2fit_last_error(), change
    torch.cuda.synchronize()
    for b, v in zip(rb, r):
        assert RC.same_bits(_payload(b[0], b[2]).view(np.float32).reshape(v.shape), v)
    for b in (sb, wb, gb):
        assert np.all(_payload(b[0], b[2]) == SENTINEL)
    assert lib.t2fit_sr_robust_workspace_bytes(1, many, 1, C.byref(need)) == -1
    assert GUARD > 0


def _same_info(info, winfo):
    for a, b in zip(info["slice_weights"], winfo["slice_weights"]):
        assert RC.same_bits(a.cpu().numpy(), b)
    assert RC.same_bits(info["sigma2"].cpu().numpy(), winfo["sigma2"])
    assert RC.same_bits(info["robust_sums"].cpu().numpy(), winfo["robust_sums"])


def test_reconstruct_sr_robust_equals_the_statement_stack_wise_and_per_slice(t2):
    _, bad, geoms, _, _ = RC.corrupted_phantom()
    got, _, info = t2.reconstruct_sr(bad, geoms, n_iter=3, prox_iter=5, robust=True, return_info=True)
    want, _, winfo = S.reconstruct_sr(bad, geoms, n_iter=3, prox_iter=5, robust=True, return_info=True)
    assert _bits_equal(got.cpu().numpy(), want) == 0
    _same_info(info, winfo)
    again = t2.reconstruct_sr(bad, geoms, n_iter=3, prox_iter=5, robust=True)[0]
    assert _bits_equal(again.cpu().numpy(), want) == 0
    plain = t2.reconstruct_sr(bad, geoms, n_iter=3, prox_iter=5)[0].cpu().numpy()
    off = t2.reconstruct_sr(bad, geoms, n_iter=3, prox_iter=5, robust=None)[0].cpu().numpy()
    assert _bits_equal(off, plain) == 0 and not np.array_equal(plain, want)
    assert _bits_equal(plain, S.reconstruct_sr(bad, geoms, n_iter=3, prox_iter=5)[0]) == 0
    # a pose per slice, one corrupted slice, tuned parameters
    stacks, geoms, poses = RC.moved_corrupted()
    kw = dict(n_iter=3, prox_iter=5, slice_transforms=poses, robust={"slice_threshold": 1.25, "huber": 2.0}, return_info=True)
    got, _, info = t2.reconstruct_sr(stacks, geoms, **kw)
    want, _, winfo = S.reconstruct_sr(stacks, geoms, **kw)
    assert _bits_equal(got.cpu().numpy(), want) == 0
    _same_info(info, winfo)
    assert _bits_equal(t2.reconstruct_sr(stacks, geoms, **kw)[0].cpu().numpy(), want) == 0
    assert winfo["slice_weights"][1][0, 5] < 0.5  # cor slice 5 was dimmed


def test_the_four_phantom_conditions_from_device_runs(t2):
    clean, bad, geoms, truth, grid = RC.corrupted_phantom()
    rmse, info = {}, None
    for key, stacks, robust in (("pc", clean, None), ("pb", bad, None), ("rc", clean, True), ("rb", bad, True)):
        x, header, info = t2.reconstruct_sr(stacks, geoms, robust=robust, return_info=True)
        rmse[key] = K.interior_rmse(x.cpu().numpy(), truth, grid, header.GetOrigin())
    weights = [w.cpu().numpy() for w in info["slice_weights"]]
    RC.check_phantom_conditions(rmse["pc"], rmse["pb"], rmse["rc"], rmse["rb"], weights, ["ax", "cor", "sag"])


SVR_KW = dict(rounds=1, n_iter=2, prox_iter=3, robust=True)


def test_reconstruct_svr_passes_robust_through(t2):
    stacks, geoms, _ = RC.moved_corrupted()
    want, hi, want_found = V.reconstruct_svr(stacks, geoms, slice_masks=W.phantom_masks(), **SVR_KW)
    got, header, found = t2.sr.reconstruct_svr(stacks, geoms, slice_masks=W.phantom_masks(), **SVR_KW)
    assert header.GetOrigin() == hi.GetOrigin()
    for o in geoms:
        assert RC.same_bits(np.asarray(found.transforms[o]), np.asarray(want_found.transforms[o]))
    assert _bits_equal(got.cpu().numpy(), want) == 0
    plain = t2.sr.reconstruct_svr(stacks, geoms, slice_masks=W.phantom_masks(), **{**SVR_KW, "robust": None})[0]
    assert not np.array_equal(plain.cpu().numpy(), want)  # the keyword reached the reconstruction


def test_recon_sr_robust_writes_the_statement_and_the_weights(t2, tmp_path, monkeypatch):
    import sys

    monkeypatch.setitem(sys.modules, "SimpleITK", None)  # the package's NIfTI reader; an earlier test may have faked one

    from fetal_t2mapping_amd import nifti, recon

    stacks, geoms, _, _, _, _ = K._phantom_stacks(n_te=3, side=32, thick=4.0, seed=27)
    stacks = {o: np.array(v, np.float32) for o, v in stacks.items()}
    stacks["cor"][:, 3] *= np.float32(0.3)
    te_ms = [114, 202, 299]
    bids, md = _write_subject(tmp_path, stacks, geoms, te_ms, None)
    base = ["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo", "--lf", "--recon_method", "sr", "--sr_iter", "2", "--sr_weight", "8",
            "--sr_thickness", "4"]

    def run(extra):
        args = recon.parse_arguments(base + extra)
        written = recon.process_recon(md, bids, denoise=False, sr=args.sr_args)
        return [np.asarray(nifti.ReadImage(p).arr, np.float32) for p in written]

    csv = str(tmp_path / "weights" / "slices.csv")
    plain = run([])  # without the flag: the files of the existing test
    want_plain = S.reconstruct_sr(stacks, geoms, weight=8.0, n_iter=2, thickness=4.0)[0]
    for i in range(3):
        assert _bits_equal(plain[i], want_plain[i]) == 0
    assert not os.path.exists(csv)
    robust = run(["--sr_robust", "--sr_robust_huber", "2.0", "--sr_write_slice_weights", csv])
    want, _, winfo = S.reconstruct_sr(stacks, geoms, weight=8.0, n_iter=2, thickness=4.0, robust={"huber": 2.0}, return_info=True)
    for i in range(3):
        assert _bits_equal(robust[i], want[i]) == 0
    assert not np.array_equal(robust[0], plain[0])
    rows, sigma = recon.load_slice_weights(csv)
    order = ["ax", "cor", "sag"]
    assert len(rows) == 3 * sum(geoms[o].shape[0] for o in order)
    k0 = {o: int(np.sum([geoms[p].shape[0] for p in order[:i]])) for i, o in enumerate(order)}
    for o, k, e, w, c, ms in rows:
        assert w == winfo["slice_weights"][order.index(o)][e, k]
        cc, q2 = winfo["robust_sums"][e, k0[o] + k]
        assert c == int(cc) and ms == (q2 / cc if cc > 0 else 0.0)
    assert sigma == {e: float(np.sqrt(winfo["sigma2"][e])) for e in range(3)}
    assert min(r[3] for r in rows if r[0] == "cor" and r[1] == 3) < 1.0
