"""The super-resolution operator with a rigid pose per slice on the device (sr_slice_forward_kernel and
sr_slice_adjoint_kernel of csrc/t2fit_sr.hip) against its numpy statement (fetal_t2mapping_amd/_sr.py: forward_slices,
adjoint_slices), bit for bit: normaliser, forward, residual, adjoint and update over the six stack directions and both
profiles with the poses mixed on purpose (the exact stack pose on an axis-aligned stack, large rotations, a slice wholly
off the grid, one partly off it, one fully masked), 1 and chunk + 1 volumes; several stacks with different slice counts
in one pass; a stack with more slices than one culling pass; equal slice affines against the stack-wise kernels; the raw
entry points on pointers off a 256-byte boundary into sentinel-guarded buffers; the whole loop on a phantom that moved
between slices; and recon.py --sr_slice_transforms on files.  tests/test_sr_slice_host.py covers what needs no device."""
import ctypes as C
import os

import numpy as np
import pytest

import sr_cases as K
import sr_slice_cases as L
from fetal_t2mapping_amd import _resample as R
from fetal_t2mapping_amd import _sr as S
from test_recon_gpu import _bits_equal, _guarded, _payload, _write_subject
from test_sr_gpu import CHUNK, _guarded64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def t2():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X")
    import fetal_t2mapping_amd as t2

    return t2


@pytest.mark.parametrize("profile", K.PROFILE_NAMES)
@pytest.mark.parametrize("name", sorted(K.DIRECTIONS))
def test_mixed_poses_equal_the_statement_bit_for_bit(t2, name, profile):
    c = L.MixedCase(name)
    hr, lr = c.hr.shape, c.stack.shape
    n_max = CHUNK + 1
    rng = np.random.default_rng(81)
    x = rng.normal(500, 200, size=(n_max,) + hr).astype(np.float32)
    y = rng.normal(500, 200, size=(n_max,) + lr).astype(np.float32)
    r = rng.normal(0, 50, size=(n_max,) + lr).astype(np.float32)
    want_n = S.forward_slices(None, c.B, lr, profile, c.rel, hr_shape=hr)[1]
    # what the case is for: slice 2 sees nothing, slice 3 is partly off the grid, the others are inside; slice 4 is masked
    assert np.all(want_n[2] == 0) and 50 < np.count_nonzero(want_n[3] == 0) < want_n[3].size - 50
    assert np.count_nonzero(want_n[0] > 0) > 300 and np.count_nonzero(want_n[1] > 0) > 200 and np.all(c.mask[4] == 0)
    got_n = t2.sr_forward_slices(None, c.B, lr, profile=profile, rel_thickness=c.rel, hr_shape=hr)[1]
    assert got_n.dtype == np.float64 and np.array_equal(got_n, want_n)
    for mask in (None, c.mask):
        masks = None if mask is None else [mask]
        want_ax = S.forward_slices(x, c.B, lr, profile, c.rel, mask=mask)[0]
        want_res = S.forward_slices(x, c.B, lr, profile, c.rel, y=y, mask=mask)[0]
        want_adj = S.adjoint_slices([r], [want_n], [c.B], profile, c.rel, hr, masks=masks)
        want_upd = S.adjoint_slices([r], [want_n], [c.B], profile, c.rel, hr, masks=masks, x=x, tau=0.37)
        assert np.any(want_ax != 0) and np.any(want_adj != 0) and (mask is None or np.all(want_ax[:, 4] == 0))
        for n_vol in (1, n_max):
            what = (name, profile, mask is not None, n_vol)
            got, n2 = t2.sr_forward_slices(x[:n_vol], c.B, lr, profile=profile, rel_thickness=c.rel, mask=mask)
            assert np.array_equal(n2, want_n) and _bits_equal(got, want_ax[:n_vol]) == 0, what
            got = t2.sr_forward_slices(x[:n_vol], c.B, lr, profile=profile, rel_thickness=c.rel, y=y[:n_vol], mask=mask)[0]
            assert _bits_equal(got, want_res[:n_vol]) == 0, what
            got = t2.sr_adjoint_slices([r[:n_vol]], [want_n], [c.B], profile, c.rel, hr, masks=masks)
            assert _bits_equal(got, want_adj[:n_vol]) == 0, what
            got = t2.sr_adjoint_slices([r[:n_vol]], [want_n], [c.B], profile, c.rel, hr, masks=masks, x=x[:n_vol], tau=0.37)
            assert _bits_equal(got, want_upd[:n_vol]) == 0, what


def _moved_stack(hr, name, size, spacing, seed, deg=8.0, mm=2.0):
    stack = K.centred_stack(K.DIRECTIONS[name], size, spacing, K.grid_centre(hr))
    t = S.compose_slice_transforms(K.rigid(), L.motion(size[2], deg, mm, seed), stack)
    return stack, S.slice_affines(hr, stack, t)


def test_several_stacks_with_different_slice_counts_in_one_pass_and_tensors(t2):
    import torch

    rng = np.random.default_rng(82)
    mixed = L.MixedCase("cor")
    hr = mixed.hr
    built = [(mixed.stack, mixed.B), _moved_stack(hr, "sag_oblique", (21, 19, 5), (1.0, 1.1, 4.5), 83),
             _moved_stack(hr, "ax", (17, 20, 3), (1.2, 1.0, 6.0), 84), _moved_stack(hr, "cor_oblique", (19, 16, 9), (1.1, 1.3, 2.5), 85),
             _moved_stack(hr, "sag", (20, 21, 1), (1.0, 1.0, 5.0), 86), _moved_stack(hr, "ax_oblique", (15, 14, 12), (1.5, 1.5, 2.0), 87)]
    shapes = [g.shape for g, _ in built]
    Bs = [b for _, b in built]
    assert sorted({s[0] for s in shapes}) == [1, 3, 5, 9, 12]
    profiles = ["box", "bspline3", "bspline3", "box", "box", "bspline3"]
    rels = [1.1, 1.2, 0.9, 1.6, 1.0, 2.0]
    masks = [mixed.mask, None, None, (rng.random(shapes[3]) > 0.3).astype(np.uint8), None, None]
    N = [S.forward_slices(None, b, s, p, t, hr_shape=hr.shape)[1] for b, s, p, t in zip(Bs, shapes, profiles, rels)]
    assert all(np.count_nonzero(n > 0) > n.size // 4 for n in N)
    r = [rng.normal(0, 50, size=s).astype(np.float32) for s in shapes]
    x = rng.normal(500, 200, size=hr.shape).astype(np.float32)
    want = S.adjoint_slices(r, N, Bs, profiles, rels, hr.shape, masks=masks, x=x, tau=0.21)
    got = t2.sr_adjoint_slices(r, N, Bs, profiles, rels, hr.shape, masks=masks, x=x, tau=0.21)
    assert got.shape == hr.shape and _bits_equal(got, want) == 0
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    got = t2.sr_adjoint_slices([dev(v) for v in r], [dev(v) for v in N], Bs, profiles, rels, hr.shape,
                               masks=[None if m is None else dev(m) for m in masks], x=dev(x), tau=0.21)
    assert got.is_cuda and _bits_equal(got.cpu().numpy(), want) == 0
    ax, n = t2.sr_forward_slices(dev(x), Bs[3], shapes[3], profile="box", rel_thickness=rels[3])
    assert ax.is_cuda and n.is_cuda and np.array_equal(n.cpu().numpy(), N[3])
    assert _bits_equal(ax.cpu().numpy(), S.forward_slices(x, Bs[3], shapes[3], "box", rels[3])[0]) == 0


@pytest.mark.parametrize("profile", K.PROFILE_NAMES)
def test_a_stack_with_more_slices_than_one_culling_pass(t2, profile):
    hr, stack, Bs, rel = L.thin_case()
    lr = stack.shape
    assert lr == (300, 8, 9) and hr.shape == (10, 9, 11)
    rng = np.random.default_rng(88)
    x = rng.normal(500, 200, size=(2,) + hr.shape).astype(np.float32)
    y = rng.normal(500, 200, size=(2,) + lr).astype(np.float32)
    want, want_n = S.forward_slices(x, Bs, lr, profile, rel, y=y)
    assert np.count_nonzero(want_n[:256].sum(axis=(1, 2)) > 0) > 20 and np.count_nonzero(want_n[256:].sum(axis=(1, 2)) > 0) > 20
    got, got_n = t2.sr_forward_slices(x, Bs, lr, profile=profile, rel_thickness=rel, y=y)
    assert np.array_equal(got_n, want_n) and _bits_equal(got, want) == 0
    want_upd = S.adjoint_slices([want], [want_n], [Bs], profile, rel, hr.shape, x=x, tau=0.02)
    got_upd = t2.sr_adjoint_slices([want], [want_n], [Bs], profile, rel, hr.shape, x=x, tau=0.02)
    assert _bits_equal(got_upd, want_upd) == 0 and not np.array_equal(want_upd, x)


@pytest.mark.parametrize("profile", K.PROFILE_NAMES)
@pytest.mark.parametrize("name", ["ax", "cor_oblique", "sag"])
def test_equal_slice_affines_give_the_bits_of_the_stack_wise_kernels(t2, name, profile):
    rng = np.random.default_rng(89)
    n_vol = CHUNK + 1
    for c in (K.gpu_case(name, outside=True), K.Case(name, (27, 23, 25), (21, 19, 5), (1.0, 1.1, 4.5), 5.0, None, seed=32)):
        hr, lr = c.hr.shape, c.stack.shape
        Bs = np.repeat(c.B[None], lr[0], axis=0)
        x = rng.normal(500, 200, size=(n_vol,) + hr).astype(np.float32)
        y = rng.normal(500, 200, size=(n_vol,) + lr).astype(np.float32)
        a, an = t2.sr_forward(x, c.B, lr, profile=profile, rel_thickness=c.rel, y=y, mask=c.mask)
        b, bn = t2.sr_forward_slices(x, Bs, lr, profile=profile, rel_thickness=c.rel, y=y, mask=c.mask)
        assert np.array_equal(an, bn) and _bits_equal(a, b) == 0 and np.any(a != 0)
        u = t2.sr_adjoint([a], [an], [c.B], profile, c.rel, hr, masks=[c.mask], x=x, tau=0.3)
        v = t2.sr_adjoint_slices([a], [an], [Bs], profile, c.rel, hr, masks=[c.mask], x=x, tau=0.3)
        assert _bits_equal(u, v) == 0 and not np.array_equal(u, x)
        assert _bits_equal(t2.sr_adjoint([a], [an], [c.B], profile, c.rel, hr), t2.sr_adjoint_slices([a], [an], [Bs], profile, c.rel, hr)) == 0


@pytest.mark.parametrize("profile", K.PROFILE_NAMES)
def test_raw_calls_on_offset_pointers_write_nothing_outside_their_outputs_and_repeat(t2, profile):
    import torch

    from fetal_t2mapping_amd import _abi
    from fetal_t2mapping_amd._lib import load

    lib = load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(90)
    n_vol = CHUNK + 1
    cases = [L.MixedCase("cor_oblique"), L.MixedCase("sag")]
    hr = cases[0].hr.shape
    n_h = int(np.prod(hr))
    x = rng.normal(500, 200, size=(n_vol,) + hr).astype(np.float32)
    xbuf, xptr, xw = _guarded(x.ravel())
    pid = _abi.SR_PROFILES[profile]
    held, res_ptrs, n_ptrs, mask_ptrs, table_ptrs, want_res, want_n = [], [], [], [], [], [], []
    for c in cases:
        lr = c.stack.shape
        n_l = int(np.prod(lr))
        y = rng.normal(500, 200, size=(n_vol,) + lr).astype(np.float32)
        ybuf, yptr, yw = _guarded(y.ravel())
        mbuf = torch.from_numpy(c.mask.ravel().copy()).cuda()
        table = t2.sr_slice_table(c.B, profile, c.rel)
        assert table.dtype == np.uint8 and table.size == 208 * lr[0]
        # the table 8 bytes past a 256-byte boundary: aligned to 8, not to 16
        tbuf = torch.zeros(8 + table.size, dtype=torch.uint8, device="cuda")
        tbuf[8:] = torch.from_numpy(table).cuda()
        tptr = tbuf.data_ptr() + 8
        assert tptr % 256 == 8
        runs = []
        for _ in range(2):
            obuf, optr, ow = _guarded(None, n_vol * n_l)
            nbuf, nptr, nw = _guarded64(n_l)
            rc = lib.t2fit_sr_slice_forward_dev(xptr, *hr, n_vol, tptr, pid, c.rel, yptr, mbuf.data_ptr(), *lr, optr, nptr, stream)
            assert rc == 0, lib.t2fit_last_error().decode()
            torch.cuda.synchronize()
            runs.append((_payload(obuf, ow).view(np.float32).reshape((n_vol,) + lr), _payload(nbuf, nw).view(np.float64).reshape(lr)))
        _payload(ybuf, yw), _payload(xbuf, xw)
        assert _bits_equal(runs[0][0], runs[1][0]) == 0 and np.array_equal(runs[0][1], runs[1][1])
        wr, wn = S.forward_slices(x, c.B, lr, profile, c.rel, y=y, mask=c.mask)
        assert np.array_equal(runs[0][1], wn) and _bits_equal(runs[0][0], wr) == 0
        held.append((obuf, ow, nbuf, nw, mbuf, ybuf, tbuf))
        res_ptrs.append(optr), n_ptrs.append(nptr), mask_ptrs.append(mbuf.data_ptr()), table_ptrs.append(tptr)
        want_res.append(wr), want_n.append(wn)
    P = lambda v: (C.c_void_p * len(v))(*v)
    lo = (C.c_int32 * 6)(*[v for c in cases for v in c.stack.shape])
    D = lambda a: (C.c_double * np.size(a))(*np.ravel(a))
    runs = []
    for _ in range(2):
        zbuf, zptr, zw = _guarded(None, n_vol * n_h)
        rc = lib.t2fit_sr_slice_adjoint_dev(2, P(res_ptrs), P(n_ptrs), P(mask_ptrs), P(table_ptrs), lo, (C.c_int32 * 2)(pid, pid),
                                            D([c.rel for c in cases]), xptr, 0.4, zptr, *hr, n_vol, stream)
        assert rc == 0, lib.t2fit_last_error().decode()
        torch.cuda.synchronize()
        runs.append(_payload(zbuf, zw).view(np.float32).reshape((n_vol,) + hr))
    for obuf, ow, nbuf, nw, _, _, _ in held:
        _payload(obuf, ow), _payload(nbuf, nw)
    _payload(xbuf, xw)
    want = S.adjoint_slices(want_res, want_n, [c.B for c in cases], profile, [c.rel for c in cases], hr, masks=[c.mask for c in cases],
                            x=x, tau=0.4)
    assert _bits_equal(runs[0], want) == 0 and _bits_equal(runs[0], runs[1]) == 0


def test_whole_loop_on_the_moved_phantom_equals_the_statement_and_beats_merge_and_stack_wise(t2):
    stacks, geoms, truth, grid, poses = L.moved_phantom()
    got, header, info = t2.reconstruct_sr(stacks, geoms, n_iter=2, slice_transforms=poses, return_info=True)
    want, hi, winfo = L.moved_statement(2, S.DEFAULT_PROX_ITER, True)
    assert got.is_cuda and tuple(got.shape) == want.shape == (1, 48, 48, 48) and header.GetOrigin() == hi.GetOrigin()
    assert info["tau"] == winfo["tau"] and info["column_max"] == [float(m) for m in winfo["column_max"]]
    for a, b in zip(info["N"], winfo["N"]):
        assert np.array_equal(a.cpu().numpy(), b)
    assert _bits_equal(got.cpu().numpy(), want) == 0
    aware = t2.reconstruct_sr(stacks, geoms, slice_transforms=poses)[0].cpu().numpy()
    plain = t2.reconstruct_sr(stacks, geoms)[0].cpu().numpy()
    merged = t2.reconstruct_stacks(stacks, geoms)[0].cpu().numpy()
    rmse = {k: K.interior_rmse(v, truth, grid, header.GetOrigin()) for k, v in (("aware", aware), ("plain", plain), ("merge", merged))}
    print(f"interior RMSE at the default iterations: merge {rmse['merge']:.3f}, without the poses {rmse['plain']:.3f}, "
          f"with them {rmse['aware']:.3f}")
    assert rmse["aware"] < rmse["merge"] and rmse["aware"] < rmse["plain"]
    # a fixed stack with an entry, a moving one without, a transform, masks, the B-spline, weight 0 (in place), two echoes
    two = {o: np.stack([stacks[o][0], stacks[o][0] * 0.5]) for o in ("ax", "cor")}
    kw = dict(fixed="ax", weight=0.0, n_iter=2, profile="bspline3", thickness={"cor": 5.0}, transforms={"cor": K.rigid(0.3)},
              stack_masks={"cor": (np.random.default_rng(91).random(geoms["cor"].shape) > 0.1)}, slice_transforms={"ax": poses["ax"]},
              x0=merged[0][None].repeat(2, axis=0))
    got2, _ = t2.reconstruct_sr(two, {o: geoms[o] for o in two}, **kw)
    want2, _ = S.reconstruct_sr(two, {o: geoms[o] for o in two}, **kw)
    assert _bits_equal(got2.cpu().numpy(), want2) == 0 and not np.array_equal(want2, kw["x0"])


def test_without_slice_transforms_the_bytes_are_those_of_the_stack_wise_path(t2):
    rng = np.random.default_rng(92)
    geoms = {o: K.centred_stack(K.DIRECTIONS[o], (14, 13, 4), (1.0, 1.0, 3.0), (0.0, 0.0, 0.0)) for o in ("ax", "cor", "sag")}
    stacks = {o: rng.normal(500, 100, size=(2,) + geoms[o].shape).astype(np.float32) for o in geoms}
    kw = dict(n_iter=2, prox_iter=3, weight=4.0, transforms={"sag": K.rigid(0.5)})
    want = S.reconstruct_sr(stacks, geoms, **kw)[0]
    a = t2.reconstruct_sr(stacks, geoms, **kw)[0].cpu().numpy()
    b = t2.reconstruct_sr(stacks, geoms, slice_transforms=None, **kw)[0].cpu().numpy()
    assert _bits_equal(a, want) == 0 and _bits_equal(b, want) == 0
    # every slice at its stack's transform: the slice kernels, the same bytes again
    same = {"ax": np.repeat(np.eye(4)[None], 4, axis=0), "sag": np.repeat(kw["transforms"]["sag"][None], 4, axis=0)}
    c = t2.reconstruct_sr(stacks, geoms, slice_transforms=same, **kw)[0].cpu().numpy()
    assert _bits_equal(c, want) == 0
    for bad in ({"ax": same["ax"][:3]}, {"cor2": same["ax"]}, {"sag": np.full((4, 4, 4), np.nan)}):
        with pytest.raises(ValueError):
            t2.reconstruct_sr(stacks, geoms, slice_transforms=bad, **kw)


def test_sr_slice_transforms_flag_writes_the_statement_and_the_default_still_writes_the_merge(t2, tmp_path, monkeypatch):
    import sys

    monkeypatch.setitem(sys.modules, "SimpleITK", None)  # the package's NIfTI reader; an earlier test may have faked one

    from fetal_t2mapping_amd import nifti, recon

    stacks, geoms, _, _, _, _ = K._phantom_stacks(n_te=3, side=32, thick=4.0, seed=27)
    te_ms = [114, 202, 299]
    bids, md = _write_subject(tmp_path, stacks, geoms, te_ms, None)
    poses = {o: S.compose_slice_transforms(None, L.motion(geoms[o].shape[0], 3.0, 1.5, 93 + i), geoms[o]) for i, o in enumerate(("ax", "sag"))}
    acq = {"sub": "sub-001", "ses": "ses-01"}
    pose_dir = str(tmp_path / "poses")
    os.makedirs(pose_dir)
    for o in poses:  # one file per (sub, ses): every echo finds it
        np.savetxt(recon.slice_transforms_path(pose_dir, acq, o), poses[o].reshape(-1, 16), fmt="%.17g")
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
    sr = run(["--recon_method", "sr", "--sr_iter", "1", "--sr_weight", "8", "--sr_thickness", "4", "--sr_slice_transforms", pose_dir])
    want_sr = S.reconstruct_sr(stacks, geoms, weight=8.0, n_iter=1, thickness=4.0, slice_transforms=poses)[0]
    plain = S.reconstruct_sr(stacks, geoms, weight=8.0, n_iter=1, thickness=4.0)[0]
    for i in range(3):
        assert _bits_equal(sr[i], want_sr[i]) == 0
    assert not np.array_equal(want_sr, plain)
    # a file with another row count than the stack has slices is an error that names it
    np.savetxt(recon.slice_transforms_path(pose_dir, acq, "sag"), poses["sag"][:-1].reshape(-1, 16), fmt="%.17g")
    with pytest.raises(ValueError, match=r"sub-001_ses-01_sag_slices\.txt"):
        run(["--recon_method", "sr", "--sr_iter", "1", "--sr_slice_transforms", pose_dir])
