"""The super-resolution operator on the device (csrc/t2fit_sr.hip) against its numpy statement
(fetal_t2mapping_amd/_sr.py), bit for bit: normaliser, forward, residual, adjoint and update over the six stack
directions, both profiles, 1 / chunk / chunk + 1 / 8 volumes, with and without masks, through a rigid transform, with the
stack inside the grid and partly outside it; the raw entry points on pointers off a 256-byte boundary into
sentinel-guarded buffers; the whole loop on the phantom against the statement's loop, against itself and against the
averaged merge; one call at the workload's size against the statement on sample boxes; and recon.py --recon_method sr on
files.  tests/test_sr_host.py covers what needs no device."""
import ctypes as C
import os

import numpy as np
import pytest

import sr_cases as K
from fetal_t2mapping_amd import _resample as R
from fetal_t2mapping_amd import _sr as S
from test_recon_gpu import GUARD, SENTINEL, _bits_equal, _guarded, _payload, _stack_geometry, _write_subject

pytestmark = pytest.mark.gpu

CHUNK = 4  # kSrChunk of csrc/t2fit_sr.hip: echoes per walk of the candidates


@pytest.fixture(scope="module")
def t2():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X")
    import fetal_t2mapping_amd as t2

    return t2


@pytest.mark.parametrize("profile", K.PROFILE_NAMES)
@pytest.mark.parametrize("name", sorted(K.DIRECTIONS))
def test_normaliser_forward_adjoint_and_update_equal_the_statement_bit_for_bit(t2, name, profile):
    rng = np.random.default_rng(51)
    for outside in (False, True):
        c = K.gpu_case(name, outside)
        hr, lr = c.hr.shape, c.stack.shape
        x = rng.normal(500, 200, size=(8,) + hr).astype(np.float32)
        y = rng.normal(500, 200, size=(8,) + lr).astype(np.float32)
        r = rng.normal(0, 50, size=(8,) + lr).astype(np.float32)
        want_n = S.forward(None, c.B, lr, profile, c.rel, hr_shape=hr)[1]
        assert np.count_nonzero(want_n > 0) > 1000 and (not outside or np.count_nonzero(want_n == 0) > 500), (name, outside)
        got_n = t2.sr_forward(None, c.B, lr, profile=profile, rel_thickness=c.rel, hr_shape=hr)[1]
        assert got_n.dtype == np.float64 and np.array_equal(got_n, want_n), (name, outside)
        for mask in (None, c.mask):
            masks = None if mask is None else [mask]
            want_ax = S.forward(x, c.B, lr, profile, c.rel, mask=mask)[0]
            want_res = S.forward(x, c.B, lr, profile, c.rel, y=y, mask=mask)[0]
            want_adj = S.adjoint([r], [want_n], [c.B], profile, c.rel, hr, masks=masks)
            want_upd = S.adjoint([r], [want_n], [c.B], profile, c.rel, hr, masks=masks, x=x, tau=0.37)
            assert np.any(want_ax != 0) and np.any(want_adj != 0)
            for n_vol in (1, CHUNK, CHUNK + 1, 8):
                what = (name, profile, outside, mask is not None, n_vol)
                got, n2 = t2.sr_forward(x[:n_vol], c.B, lr, profile=profile, rel_thickness=c.rel, mask=mask)
                assert np.array_equal(n2, want_n) and _bits_equal(got, want_ax[:n_vol]) == 0, what
                got = t2.sr_forward(x[:n_vol], c.B, lr, profile=profile, rel_thickness=c.rel, y=y[:n_vol], mask=mask)[0]
                assert _bits_equal(got, want_res[:n_vol]) == 0, what
                got = t2.sr_adjoint([r[:n_vol]], [want_n], [c.B], profile, c.rel, hr, masks=masks)
                assert _bits_equal(got, want_adj[:n_vol]) == 0, what
                got = t2.sr_adjoint([r[:n_vol]], [want_n], [c.B], profile, c.rel, hr, masks=masks, x=x[:n_vol], tau=0.37)
                assert _bits_equal(got, want_upd[:n_vol]) == 0, what


def test_adjoint_of_several_stacks_in_one_pass_and_tensors(t2):
    """Six stacks (every direction, profiles and thicknesses mixed, two masked) through one launch, (Z, Y, X) inputs, CUDA
    tensors in and out."""
    import torch

    rng = np.random.default_rng(52)
    names = sorted(K.DIRECTIONS)
    cases = [K.gpu_case(n, outside=i % 2 == 1) for i, n in enumerate(names)]
    profiles = ["box", "bspline3", "bspline3", "box", "box", "bspline3"]
    rels = [c.rel * (1.0 + 0.1 * i) for i, c in enumerate(cases)]
    hr = cases[0].hr.shape
    masks = [c.mask if i in (1, 4) else None for i, c in enumerate(cases)]
    N = [S.forward(None, c.B, c.stack.shape, p, t, hr_shape=hr)[1] for c, p, t in zip(cases, profiles, rels)]
    r = [rng.normal(0, 50, size=c.stack.shape).astype(np.float32) for c in cases]
    x = rng.normal(500, 200, size=hr).astype(np.float32)
    want = S.adjoint(r, N, [c.B for c in cases], profiles, rels, hr, masks=masks, x=x, tau=0.21)
    got = t2.sr_adjoint(r, N, [c.B for c in cases], profiles, rels, hr, masks=masks, x=x, tau=0.21)
    assert got.shape == hr and _bits_equal(got, want) == 0
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    got = t2.sr_adjoint([dev(v) for v in r], [dev(v) for v in N], [c.B for c in cases], profiles, rels, hr,
                        masks=[None if m is None else dev(m) for m in masks], x=dev(x), tau=0.21)
    assert got.is_cuda and _bits_equal(got.cpu().numpy(), want) == 0
    ax, n = t2.sr_forward(dev(x), cases[2].B, cases[2].stack.shape, profile="bspline3", rel_thickness=rels[2])
    assert ax.is_cuda and n.is_cuda and np.array_equal(n.cpu().numpy(), N[2])
    assert _bits_equal(ax.cpu().numpy(), S.forward(x, cases[2].B, cases[2].stack.shape, "bspline3", rels[2])[0]) == 0
    box = t2.sr_box(cases[2].B, "bspline3", rels[2])
    ref = S.plan_box(cases[2].B, (1.0, 1.0, S.profile_params("bspline3", rels[2])[1]))
    assert box[1] == ref[1] and np.array_equal(box[0], ref[0])


def _guarded64(n):
    """A float64 output of n elements 8 bytes past a 256-byte boundary between sentinel words."""
    import torch

    buf = torch.full((2 + GUARD + 2 * n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 256 == 0
    where = slice(2 + GUARD, 2 + GUARD + 2 * n)
    ptr = buf.data_ptr() + 4 * (2 + GUARD)
    assert ptr % 256 == 8
    return buf, ptr, where


@pytest.mark.parametrize("profile", K.PROFILE_NAMES)
def test_raw_calls_on_offset_pointers_write_nothing_outside_their_outputs(t2, profile):
    import torch

    from fetal_t2mapping_amd import _abi
    from fetal_t2mapping_amd._lib import load

    lib = load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(53)
    n_vol = CHUNK + 1
    cases = [K.gpu_case("cor_oblique", outside=True), K.gpu_case("sag")]
    hr = cases[0].hr.shape
    n_h = int(np.prod(hr))
    x = rng.normal(500, 200, size=(n_vol,) + hr).astype(np.float32)
    xbuf, xptr, xw = _guarded(x.ravel())
    D = lambda a: (C.c_double * np.size(a))(*np.ravel(a))
    pid = _abi.SR_PROFILES[profile]
    held, res_ptrs, n_ptrs, mask_ptrs, want_res, want_n = [], [], [], [], [], []
    for c in cases:
        lr = c.stack.shape
        n_l = int(np.prod(lr))
        y = rng.normal(500, 200, size=(n_vol,) + lr).astype(np.float32)
        ybuf, yptr, yw = _guarded(y.ravel())
        mbuf = torch.from_numpy(c.mask.ravel().copy()).cuda()
        obuf, optr, ow = _guarded(None, n_vol * n_l)
        nbuf, nptr, nw = _guarded64(n_l)
        _, hw = S.profile_params(profile, c.rel)
        binv, radius = (C.c_double * 12)(), (C.c_int32 * 3)()
        assert lib.t2fit_sr_plan_host(D(c.B), D((1.0, 1.0, hw)), binv, radius) == 0
        rc = lib.t2fit_sr_forward_dev(xptr, *hr, n_vol, D(c.B), binv, radius, pid, c.rel, yptr, mbuf.data_ptr(), *lr, optr, nptr, stream)
        assert rc == 0, lib.t2fit_last_error().decode()
        torch.cuda.synchronize()
        res = _payload(obuf, ow).view(np.float32).reshape((n_vol,) + lr)
        n_got = _payload(nbuf, nw).view(np.float64).reshape(lr)
        _payload(ybuf, yw), _payload(xbuf, xw)
        wr, wn = S.forward(x, c.B, lr, profile, c.rel, y=y, mask=c.mask)
        assert np.array_equal(n_got, wn) and _bits_equal(res, wr) == 0
        held.append((obuf, ow, nbuf, nw, mbuf, ybuf))
        res_ptrs.append(optr), n_ptrs.append(nptr), mask_ptrs.append(mbuf.data_ptr())
        want_res.append(wr), want_n.append(wn)
    zbuf, zptr, zw = _guarded(None, n_vol * n_h)
    P = lambda v: (C.c_void_p * len(v))(*v)
    lo = (C.c_int32 * 6)(*[v for c in cases for v in c.stack.shape])
    rc = lib.t2fit_sr_adjoint_dev(2, P(res_ptrs), P(n_ptrs), P(mask_ptrs), lo, D(np.concatenate([c.B.ravel() for c in cases])),
                                  (C.c_int32 * 2)(pid, pid), D([c.rel for c in cases]), xptr, 0.4, zptr, *hr, n_vol, stream)
    assert rc == 0, lib.t2fit_last_error().decode()
    torch.cuda.synchronize()
    z = _payload(zbuf, zw).view(np.float32).reshape((n_vol,) + hr)
    for obuf, ow, nbuf, nw, _, _ in held:
        _payload(obuf, ow), _payload(nbuf, nw)
    _payload(xbuf, xw)
    want = S.adjoint(want_res, want_n, [c.B for c in cases], profile, [c.rel for c in cases], hr, masks=[c.mask for c in cases], x=x, tau=0.4)
    assert _bits_equal(z, want) == 0
    # the bare adjoint of the stacks' counted samples: the column sums the step size comes from; workspace arithmetic
    need = C.c_size_t(0)
    assert lib.t2fit_sr_workspace_bytes(2, lo, *hr, n_vol, C.byref(need)) == 0
    up = lambda v: (v + 255) // 256 * 256
    assert need.value == up(4 * n_vol * n_h) + sum(up(8 * int(np.prod(c.stack.shape))) + up(4 * n_vol * int(np.prod(c.stack.shape))) for c in cases)


def test_whole_loop_on_the_phantom_equals_the_statement_repeats_and_beats_the_merge(t2):
    stacks, geoms, truth, grid, _, _ = K.phantom()
    got, header, info = t2.reconstruct_sr(stacks, geoms, n_iter=3, prox_iter=5, return_info=True)
    again, _ = t2.reconstruct_sr(stacks, geoms, n_iter=3, prox_iter=5)
    want, hi, winfo = K.phantom_statement(3, 5)
    assert got.is_cuda and tuple(got.shape) == want.shape == (3, 48, 48, 48)
    assert header.GetOrigin() == hi.GetOrigin() and header.GetSpacing() == (1.0, 1.0, 1.0) and header.GetDirection() == hi.GetDirection()
    assert info["tau"] == winfo["tau"] and info["column_max"] == [float(m) for m in winfo["column_max"]]
    for a, b in zip(info["N"], winfo["N"]):
        assert np.array_equal(a.cpu().numpy(), b)
    got = got.cpu().numpy()
    assert _bits_equal(got, want) == 0
    assert _bits_equal(again.cpu().numpy(), got) == 0
    merged = t2.reconstruct_stacks(stacks, geoms)[0].cpu().numpy()
    sr, avg = K.interior_rmse(got, truth, grid, header.GetOrigin()), K.interior_rmse(merged, truth, grid, header.GetOrigin())
    print(f"interior RMSE after 3 iterations: super-resolution {sr:.3f}, averaged merge {avg:.3f}")
    assert sr < avg
    # weight 0 (plain iterative back-projection, in place), a B-spline profile, a thickness, masks, x0 and one stack fewer
    two_s, two_g = {o: stacks[o] for o in ("cor", "sag")}, {o: geoms[o] for o in ("cor", "sag")}
    x0 = t2.resample_volume(merged, hi, like=R.isotropic_geometry(two_g["cor"]))[0]
    kw = dict(weight=0.0, n_iter=2, profile="bspline3", thickness={"cor": 5.0}, x0=x0,
              stack_masks={"sag": (np.random.default_rng(54).random(geoms["sag"].shape) > 0.1)})
    got2, _ = t2.reconstruct_sr(two_s, two_g, fixed="cor", **kw)
    want2, _ = S.reconstruct_sr(two_s, two_g, fixed="cor", **kw)
    assert _bits_equal(got2.cpu().numpy(), want2) == 0 and not np.array_equal(want2, x0)


def test_workload_size_call_matches_the_statement_on_sample_boxes(t2):
    import torch

    n_vol, side, n_sl = 2, 256, 57
    g = torch.Generator(device="cuda").manual_seed(55)
    geoms = {o: _stack_geometry(K.DIRECTIONS[o], (side, side, n_sl), (1.0, 1.0, 4.5)) for o in ("ax", "cor", "sag")}
    order, hi, B, rels = S.sr_plan(geoms, thickness=4.0)
    assert hi.shape == (256, 256, 256)
    x = torch.rand((n_vol,) + hi.shape, generator=g, device="cuda") * 1000.0
    y = {o: torch.rand((n_vol, n_sl, side, side), generator=g, device="cuda") * 1000.0 for o in order}
    res, N = [], []
    for s, o in enumerate(order):
        r_s, n_s = t2.sr_forward(x, B[s], (n_sl, side, side), rel_thickness=rels[s], y=y[o])
        res.append(r_s), N.append(n_s)
    z = t2.sr_adjoint(res, N, B, "box", rels, hi.shape, x=x, tau=0.3)
    torch.cuda.synchronize()
    xh = x.cpu().numpy()
    resh, Nh = [r.cpu().numpy() for r in res], [n.cpu().numpy() for n in N]
    zh = z.cpu().numpy()
    rng = np.random.default_rng(55)
    for _ in range(2):
        for s, o in enumerate(order):  # a box of samples of every stack
            bz, by, bx = int(rng.integers(0, n_sl - 6)), int(rng.integers(0, side - 12)), int(rng.integers(0, side - 12))
            want, wn = S.forward(xh, B[s], (n_sl, side, side), "box", rels[s], y=y[o].cpu().numpy(), start=(bx, by, bz), shape=(6, 12, 12))
            assert np.array_equal(Nh[s][bz:bz + 6, by:by + 12, bx:bx + 12], wn), (o, bz, by, bx)
            assert _bits_equal(resh[s][:, bz:bz + 6, by:by + 12, bx:bx + 12], want) == 0, (o, bz, by, bx)
        bz, by, bx = (int(rng.integers(0, 256 - 12)) for _ in range(3))  # a box of voxels, from the device's own residuals
        want = S.adjoint(resh, Nh, B, "box", rels, hi.shape, x=xh, tau=0.3, start=(bx, by, bz), shape=(12, 12, 12))
        assert _bits_equal(zh[:, bz:bz + 12, by:by + 12, bx:bx + 12], want) == 0, (bz, by, bx)


def test_recon_method_sr_writes_the_statement_and_the_default_still_writes_the_merge(t2, tmp_path, monkeypatch):
    import sys

    monkeypatch.setitem(sys.modules, "SimpleITK", None)  # the package's NIfTI reader; an earlier test may have faked one

    from fetal_t2mapping_amd import nifti, recon

    stacks, geoms, _, _, _, _ = K._phantom_stacks(n_te=3, side=32, thick=4.0, seed=27)
    te_ms = [114, 202, 299]
    bids, md = _write_subject(tmp_path, stacks, geoms, te_ms, None)
    base = ["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo", "--lf"]

    def run(extra):
        args = recon.parse_arguments(base + extra)
        written = recon.process_recon(md, bids, denoise=False, sr=args.sr_args)
        assert [os.path.basename(p) for p in written] == [f"sub-001_ses-01_te-{t}_recon_1mm.nii.gz" for t in te_ms]
        return [np.asarray(nifti.ReadImage(p).arr, np.float32) for p in written]

    merged = run([])
    want_merge = R.reconstruct(stacks, geoms)[0]
    for i in range(3):
        assert _bits_equal(merged[i], want_merge[i]) == 0  # the default method: the averaged merge's bytes, as before
    sr = run(["--recon_method", "sr", "--sr_iter", "2", "--sr_weight", "8", "--sr_thickness", "4"])
    want_sr = S.reconstruct_sr(stacks, geoms, weight=8.0, n_iter=2, thickness=4.0)[0]
    for i in range(3):
        assert _bits_equal(sr[i], want_sr[i]) == 0
    assert not np.array_equal(sr[0], merged[0])
