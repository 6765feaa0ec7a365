"""The orthogonal-stack reconstruction on the device (csrc/t2fit_resample.hip) against its numpy statement
(fetal_t2mapping_amd/_resample.py), bit for bit: the single stage over orientations, odd sizes, a rigid transform,
both interpolations, the integer cast, one and eight volumes; the fused reconstruction against the statement, against
the chain of single stages and against itself; the raw entry points; a phantom whose merge beats every single stack; a
whole-size call; recon.py and cli.py --reconstruct on files; and the cases of tests/resample_cases.py (brick geometry of
each lane-axis kernel, lane-axis choice, rim and ties on every axis, patterns only a 32-bit copy carries, non-finite nodes
under interpolation, the saturating cast, small ragged reconstructions) bit-equal to the statement AND held to the
reference written from the definition, through raw calls on pointers 4 bytes off a 256-byte boundary into sentinel-guarded
buffers.  tests/test_recon_host.py covers what needs no device."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest

import resample_cases as K
from fetal_t2mapping_amd import _resample as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def t2():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X")
    import fetal_t2mapping_amd as t2

    return t2


def _rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    m = {0: [[1, 0, 0], [0, c, -s], [0, s, c]], 1: [[c, 0, s], [0, 1, 0], [-s, 0, c]], 2: [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis]
    return np.array(m, np.float64)


AX = np.eye(3)
COR = np.array([[1, 0, 0], [0, 0, 1], [0, 1, 0.0]])   # stack x = L, y = S, slices along P
SAG = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0.0]])   # stack x = P, y = S, slices along L
OBLIQUE = _rot(2, 9.0) @ _rot(0, -6.0)
DIRECTIONS = {"ax": AX, "cor": COR, "sag": SAG, "ax_oblique": OBLIQUE @ AX, "cor_oblique": OBLIQUE @ COR,
              "sag_oblique": OBLIQUE @ SAG}


def _bits_equal(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    return int(np.sum(got.view(np.uint32) != want.view(np.uint32)))


def _stack_geometry(direction, size=(21, 19, 5), spacing=(1.0, 1.1, 4.5)):
    d = np.asarray(direction, np.float64)
    centre = np.array([2.0, -3.0, 5.0])
    extent = d @ (np.array(spacing) * (np.array(size) - 1) / 2.0)
    return R.Geometry(size, spacing, centre - extent, d.ravel())


@pytest.mark.parametrize("name", sorted(DIRECTIONS))
@pytest.mark.parametrize("n_vol", [1, 8])
def test_single_stage_onto_a_fixed_axial_grid_is_bit_equal(t2, name, n_vol):
    """Every orientation onto one axial 1 mm grid (odd sizes, nx % 4 != 0): the kernel picks another lane axis for each."""
    rng = np.random.default_rng(21)
    src_g = _stack_geometry(DIRECTIONS[name])
    dst_g = R.Geometry((27, 23, 25), (1.0, 1.0, 1.0), (-11.0, -14.5, -7.2))
    v = rng.normal(500, 200, size=(n_vol,) + src_g.shape).astype(np.float32)
    for integer_cast in (False, True):
        got, g = t2.resample_volume(v, src_g, like=dst_g, integer_cast=integer_cast)
        want = R.resample(v, R.index_affine(dst_g, src_g), dst_g.shape, "linear", 0.0, integer_cast)
        assert g.GetSize() == dst_g.GetSize() and np.any(want != 0) and np.any(want == 0)
        assert _bits_equal(got, want) == 0, (name, n_vol, integer_cast)
    got, _ = t2.resample_volume(v, src_g, like=dst_g, interp="nearest", default=-5.0)
    assert _bits_equal(got, R.resample(v, R.index_affine(dst_g, src_g), dst_g.shape, "nearest", -5.0)) == 0


def test_single_stage_isotropic_rigid_transform_labels_and_tensors(t2):
    import torch

    rng = np.random.default_rng(22)
    for name in ("ax", "sag", "cor_oblique"):
        src_g = _stack_geometry(DIRECTIONS[name], size=(33, 18, 6))
        v = rng.normal(500, 200, size=src_g.shape).astype(np.float32)
        got, g = t2.resample_volume(v, src_g, res=1.0)  # the reference's resample_volume
        iso = R.isotropic_geometry(src_g, 1.0)
        assert g.GetSize() == iso.GetSize() == (33, 20, 27)
        assert _bits_equal(got, R.resample(v, R.index_affine(iso, src_g), iso.shape)) == 0
        T = np.eye(4)
        T[:3, :3] = _rot(1, 3.0) @ _rot(2, -5.0)
        T[:3, 3] = (1.25, -0.5, 2.0)
        got, _ = t2.resample_volume(v, src_g, res=0.9, transform=T, default=11.0)
        iso = R.isotropic_geometry(src_g, 0.9)
        assert _bits_equal(got, R.resample(v, R.index_affine(iso, src_g, T), iso.shape, default=11.0)) == 0
        lab = rng.integers(0, 12, size=src_g.shape).astype(np.int32)
        got, _ = t2.resample_volume(lab, src_g, res=1.0, interp="nearest", transform=T, default=-1)
        iso = R.isotropic_geometry(src_g, 1.0)
        want = R.resample(lab, R.index_affine(iso, src_g, T), iso.shape, "nearest", -1)
        assert got.dtype == np.int32 and np.array_equal(got, want)
        with pytest.raises(ValueError):
            t2.resample_volume(lab, src_g, res=1.0)  # labels are not interpolated linearly
    # the own grid is the identity, Inf and NaN included; a tensor in gives a tensor out
    v[2, 3, 4], v[1, 1, 1] = np.inf, np.nan
    got, _ = t2.resample_volume(torch.from_numpy(v).cuda(), src_g, like=src_g)
    assert got.is_cuda and _bits_equal(got.cpu().numpy(), v) == 0


def _three_stacks(n_vol, seed, oblique=False, size=(26, 22, 6), spacing=(1.0, 1.0, 4.5)):
    rng = np.random.default_rng(seed)
    geoms = {o: _stack_geometry(DIRECTIONS[o + ("_oblique" if oblique else "")], size, spacing) for o in ("ax", "cor", "sag")}
    if oblique:  # stacks that are not quite orthogonal to each other
        geoms["cor"] = R.Geometry(geoms["cor"].GetSize(), geoms["cor"].GetSpacing(), geoms["cor"].GetOrigin(),
                                  (_rot(1, 2.0) @ np.array(geoms["cor"].GetDirection()).reshape(3, 3)).ravel())
    stacks = {o: rng.normal(600, 150, size=(n_vol,) + geoms[o].shape).astype(np.float32) for o in geoms}
    return stacks, geoms


@pytest.mark.parametrize("case", ["aligned", "oblique", "transforms_cast", "fixed_sag"])
def test_reconstruction_fused_chain_statement_and_repeat_agree_bit_for_bit(t2, case):
    stacks, geoms = _three_stacks(3 if case != "aligned" else 8, 23, oblique=case in ("oblique", "transforms_cast"))
    kw = {}
    if case == "transforms_cast":
        T = np.eye(4)
        T[:3, :3] = _rot(0, 2.0) @ _rot(2, 1.5)
        T[:3, 3] = (0.6, -1.1, 0.4)
        kw = {"transforms": {"sag": T}, "integer_cast": True}
    if case == "fixed_sag":
        kw = {"fixed": "sag"}
    want, want_g, stages = R.reconstruct(stacks, geoms, return_stages=True, **kw)
    fused, header = t2.reconstruct_stacks(stacks, geoms, form="fused", **kw)
    chain, _ = t2.reconstruct_stacks(stacks, geoms, form="chain", **kw)
    again, _ = t2.reconstruct_stacks(stacks, geoms, form="fused", **kw)
    default, _ = t2.reconstruct_stacks(stacks, geoms, **kw)
    assert fused.is_cuda and tuple(fused.shape) == want.shape and header.GetOrigin() == want_g.GetOrigin()
    assert header.GetSpacing() == (1.0, 1.0, 1.0) and header.GetDirection() == want_g.GetDirection()
    assert np.any(stages["R"][0] != 0) and np.any(stages["R"][1] != 0)
    assert _bits_equal(chain.cpu().numpy(), want) == 0, case
    assert _bits_equal(fused.cpu().numpy(), want) == 0, case
    assert _bits_equal(again.cpu().numpy(), fused.cpu().numpy()) == 0 and _bits_equal(default.cpu().numpy(), want) == 0
    # the chain by hand: five calls of the single stage and numpy's mean
    order, hi, a1, a2 = R.plan(geoms, kw.get("fixed", "ax"), 1.0, kw.get("transforms"))
    cast = kw.get("integer_cast", False)
    H = [t2.resample_volume(stacks[o], geoms[o], res=1.0, integer_cast=cast)[0] for o in order]
    Rm = [t2.resample_volume(H[m], hi[m], like=hi[0], transform=(kw.get("transforms") or {}).get(order[m]), integer_cast=cast)[0]
          for m in (1, 2)]
    by_hand = np.mean([H[0].astype(np.float64), Rm[0].astype(np.float64), Rm[1].astype(np.float64)], axis=0).astype(np.float32)
    assert _bits_equal(by_hand, want) == 0


def test_raw_entry_points_equal_the_wrapper(t2):
    import torch

    from fetal_t2mapping_amd import _abi
    from fetal_t2mapping_amd._lib import load

    lib = load()
    stacks, geoms = _three_stacks(2, 24)
    order, hi, a1, a2 = R.plan(geoms)
    dev = [torch.from_numpy(stacks[o]).cuda() for o in order]
    lo_size = (C.c_int32 * 9)(*[v for o in order for v in stacks[o].shape[-3:]])
    hi_size = (C.c_int32 * 9)(*[v for g in hi for v in g.shape])
    A1 = (C.c_double * 36)(*np.concatenate([a.ravel() for a in a1]))
    A2 = (C.c_double * 24)(*np.concatenate([a.ravel() for a in a2]))
    ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in dev])
    out = torch.empty((2,) + hi[0].shape, dtype=torch.float32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.t2fit_reconstruct_dev(ptrs, lo_size, A1, hi_size, A2, out.data_ptr(), 2, 0, None, 0, stream) == 0
    wrapped, _ = t2.reconstruct_stacks(stacks, geoms, form="fused")
    assert _bits_equal(out.cpu().numpy(), wrapped.cpu().numpy()) == 0
    need = C.c_size_t(0)
    assert lib.t2fit_reconstruct_workspace_bytes(2, lo_size, hi_size, _abi.RECON_CHAIN, C.byref(need)) == 0
    ws = torch.empty(need.value + 256, dtype=torch.uint8, device="cuda")
    out2 = torch.empty_like(out)
    assert lib.t2fit_reconstruct_dev(ptrs, lo_size, A1, hi_size, A2, out2.data_ptr(), 2, _abi.RECON_CHAIN,
                                     (ws.data_ptr() + 255) // 256 * 256, need.value, stream) == 0
    assert _bits_equal(out2.cpu().numpy(), wrapped.cpu().numpy()) == 0
    one = torch.empty(hi[1].shape, dtype=torch.float32, device="cuda")
    A = (C.c_double * 12)(*a1[1].ravel())
    assert lib.t2fit_resample_dev(dev[1].data_ptr(), _abi.RESAMPLE_F32, *stacks[order[1]].shape[-3:], A, one.data_ptr(),
                                  *hi[1].shape, 1, _abi.INTERP_LINEAR, 0.0, 0, stream) == 0
    assert _bits_equal(one.cpu().numpy(), t2.resample_volume(stacks[order[1]][0], geoms[order[1]], res=1.0)[0]) == 0


def _phantom_stacks(n_te=3, side=48, thick=4.0, sigma=15.0, seed=25):
    """The vial phantom of synth.phantom_volume on a 1 mm cube, sampled into three thick-slice stacks (the mean
    over the slice thickness, Rician noise per stack) with the scanner's three direction matrices."""
    from fetal_t2mapping_amd import synth

    echoes, mask, _, te, _ = synth.phantom_volume((side, side, side), n_te=n_te, seed=seed, sigma=0.0)
    one = np.asarray(echoes, np.float64).reshape((n_te, side, side, side))
    # the vials run along z: three copies, one along each axis, so that no slice direction is favoured
    truth = (one + one.transpose(0, 2, 1, 3) + one.transpose(0, 3, 2, 1)) / 3.0
    rng = np.random.default_rng(seed)
    n_sl, t = int(side // thick), int(thick)
    origin = -(side - 1) / 2.0
    off = origin + (thick - 1) / 2.0  # centre of the first thick slice
    geoms = {"ax": R.Geometry((side, side, n_sl), (1, 1, thick), (origin, origin, off), AX.ravel()),
             "cor": R.Geometry((side, side, n_sl), (1, 1, thick), (origin, off, origin), COR.ravel()),
             "sag": R.Geometry((side, side, n_sl), (1, 1, thick), (off, origin, origin), SAG.ravel())}
    # truth is (te, z, y, x) in patient axes (x = L, y = P, z = S); a stack array is (slice, stack y, stack x)
    ax = truth.reshape(n_te, n_sl, t, side, side).mean(2)                                  # (S slices, P, L)
    cor = truth.reshape(n_te, side, n_sl, t, side).mean(3).transpose(0, 2, 1, 3)           # (P slices, S, L)
    sag = truth.reshape(n_te, side, side, n_sl, t).mean(4).transpose(0, 3, 1, 2)           # (L slices, S, P)
    stacks = {}
    for o, clean in (("ax", ax), ("cor", cor), ("sag", sag)):
        stacks[o] = np.hypot(clean + rng.normal(scale=sigma, size=clean.shape), rng.normal(scale=sigma, size=clean.shape)).astype(np.float32)
    grid = R.Geometry((side, side, side), (1, 1, 1), (origin, origin, origin))
    return stacks, geoms, truth, grid, te, mask


def test_merged_phantom_is_closer_to_the_truth_than_each_single_stack(t2):
    stacks, geoms, truth, grid, _, _ = _phantom_stacks()
    merged, header = t2.reconstruct_stacks(stacks, geoms)
    merged = merged.cpu().numpy()
    iso = R.isotropic_geometry(geoms["ax"], 1.0)
    assert merged.shape[1:] == iso.shape
    # compare on the voxels every stack covers, on the ax stack's 1 mm grid (origin: first slice centre)
    z0 = int(round(header.GetOrigin()[2] - grid.GetOrigin()[2] + 0.0))
    nz = iso.shape[0]
    ref = truth[:, z0:z0 + nz]
    inner = (slice(None), slice(4, nz - 6), slice(6, -6), slice(6, -6))
    rmse = lambda a: float(np.sqrt(np.mean((a[inner].astype(np.float64) - ref[inner]) ** 2)))
    single = {}
    for o in ("ax", "cor", "sag"):
        h, g = t2.resample_volume(stacks[o], geoms[o], res=1.0)
        single[o] = rmse(t2.resample_volume(h, g, like=iso)[0])
    assert rmse(merged) < min(single.values()), (rmse(merged), single)


def test_whole_size_call_matches_the_statement_on_a_sample(t2):
    import torch

    n_vol, side, n_sl = 8, 256, 57
    g = torch.Generator(device="cuda").manual_seed(26)
    geoms = {o: _stack_geometry(DIRECTIONS[o], (side, side, n_sl), (1.0, 1.0, 4.5)) for o in ("ax", "cor", "sag")}
    stacks = {o: torch.rand((n_vol, n_sl, side, side), generator=g, device="cuda") * 1000.0 for o in geoms}
    fused, header = t2.reconstruct_stacks(stacks, geoms, form="fused")
    chain, _ = t2.reconstruct_stacks(stacks, geoms, form="chain")
    torch.cuda.synchronize()
    assert tuple(fused.shape) == (n_vol, 256, side, side)  # round(57 * 4.5) = 256 (256.5 goes to the even neighbour)
    assert torch.equal(fused, chain)
    del chain
    # the statement on a seeded sample: one echo, 12-voxel boxes around random points (the other echoes are covered by
    # the equality with the chain above; the numpy statement of a whole 256^3 intermediate takes most of this test's time)
    rng = np.random.default_rng(26)
    v = int(rng.integers(0, n_vol))
    host = {o: stacks[o][v].cpu().numpy() for o in geoms}
    order, hi, a1, a2 = R.plan(geoms)
    out = fused[v].cpu().numpy()
    H = {m: R.resample(host[order[m]], a1[m], hi[m].shape) for m in (1, 2)}
    for _ in range(6):
        z, y, x = (int(rng.integers(0, 256 - 12)) for _ in range(3))
        Hf = R.resample(host[order[0]], a1[0], (12, 12, 12), start=(x, y, z))
        Rm = [R.resample(H[m], a2[m - 1], (12, 12, 12), start=(x, y, z)) for m in (1, 2)]
        assert _bits_equal(out[z:z + 12, y:y + 12, x:x + 12], R.merge(Hf, Rm[0], Rm[1])) == 0, (v, z, y, x)


def _write_subject(tmp_path, stacks, geoms, te_ms, mask):
    """The acquired stacks as NIfTI files under <prj>/<sub>/<ses>/anat, the metadata rows, a mask per echo."""
    from fetal_t2mapping_amd import cli, nifti

    bids = str(tmp_path / "projects") + "/"
    rows, run = [], 0
    for i, te in enumerate(te_ms):
        for o in ("ax", "cor", "sag"):
            run += 1
            acq = {"prj": "prj-900", "sub": "sub-001", "ses": "ses-01", "run": f"run-{run:02d}", "EchoTime": te / 1000.0,
                   "CoilString": "HeadNeck", "ImageOrientationPatientSTR": o}
            rows.append(acq)
            g = geoms[o]
            nifti.WriteImage(nifti.Image(stacks[o][i], g.GetSpacing(), g.GetOrigin(), g.GetDirection()),
                             cli.get_img_path(bids, acq, "anat"))
        if mask is not None:
            nifti.WriteImage(nifti.Image(mask.astype(np.uint8)), cli.get_img_path(bids, rows[-1], cli.mask_dirname).replace(" ", ""))
    return bids, pd.DataFrame(rows)


def test_recon_writes_recon_1mm_and_cli_reconstruct_fits_the_same_maps(t2, tmp_path, monkeypatch):
    import glob
    import sys

    monkeypatch.setitem(sys.modules, "SimpleITK", None)  # the package's NIfTI reader; an earlier test may have faked one

    from fetal_t2mapping_amd import cli, nifti, recon

    stacks, geoms, truth, grid, te, _ = _phantom_stacks(n_te=3, side=32, thick=4.0, seed=27)
    te_ms = [114, 202, 299]
    iso = R.isotropic_geometry(geoms["ax"], 1.0)
    mask = np.zeros(iso.shape, np.uint8)
    mask[4:-6, 6:-6, 6:-6] = 1
    bids, md = _write_subject(tmp_path, stacks, geoms, te_ms, mask)
    written = recon.process_recon(md, bids, denoise=False, write_resamp=True)
    assert len(written) == 3  # each echo once
    want, want_g = R.reconstruct(stacks, geoms)
    for i, path in enumerate(written):
        assert os.path.basename(path) == f"sub-001_ses-01_te-{te_ms[i]}_recon_1mm.nii.gz"
        img = nifti.ReadImage(path)
        assert img.GetSpacing() == (1.0, 1.0, 1.0) and np.allclose(img.GetOrigin(), geoms["ax"].GetOrigin(), atol=1e-4)
        assert np.allclose(img.GetDirection(), geoms["ax"].GetDirection(), atol=1e-6)
        assert _bits_equal(np.asarray(img.arr, np.float32), want[i]) == 0
    assert len(glob.glob(os.path.join(bids, "prj-900", "derivatives", "resamp_1mm", "sub-001", "ses-01", "anat", "*.nii.gz"))) == 9

    def maps(sim, extra):
        args = cli.parse_arguments(["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo", "--gaussian", "--lf", "--sim", sim] + extra)
        fit, fit_params = cli.t2map.set_fit_params(args)
        cli.process_t2maps(md, bids, te_ms, fit, fit_params, False, True, True, False, False, sim,
                           **({"reconstruct": args.reconstruct_args} if args.reconstruct_args else {}))
        files = sorted(glob.glob(os.path.join(bids, "prj-900", "derivatives", cli.t2map_dirname, "sub-001", "ses-01", "anat",
                                              f"*sim-{sim}_*map_*.nii.gz")))
        assert len(files) == 4
        return [nifti.ReadImage(f) for f in files]

    from_files = maps("files", [])
    in_memory = maps("memory", ["--reconstruct"])
    for a, b in zip(from_files, in_memory):
        assert a.arr.tobytes() == b.arr.tobytes() and a.arr.shape == iso.shape
        assert a.GetSpacing() == b.GetSpacing() and np.allclose(a.GetOrigin(), b.GetOrigin(), atol=1e-4)
    assert np.count_nonzero(from_files[0].arr) > 1000
    # a mask on another grid is refused with a clear message
    for path in glob.glob(os.path.join(bids, "prj-900", "derivatives", cli.mask_dirname, "sub-001", "ses-01", "anat", "*.nii.gz")):
        nifti.WriteImage(nifti.Image(np.ones((5, 6, 7), np.uint8)), path)
    args = cli.parse_arguments(["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo", "--gaussian", "--lf", "--sim", "bad",
                                "--reconstruct"])
    fit, fit_params = cli.t2map.set_fit_params(args)
    with pytest.raises(ValueError, match="the mask of sub-001_ses-01 has shape"):
        cli.process_t2maps(md, bids, te_ms, fit, fit_params, False, True, True, False, False, "bad",
                           reconstruct=args.reconstruct_args)


# ---- the cases of tests/resample_cases.py: the statement bit for bit (a NaN that arithmetic made by position: its sign and
# payload are not defined, numpy's inf - inf is 0xffc00000 on x86 and the device makes the positive quiet NaN) and the
# reference written from the definition ----------------------------------------------------------------------------------
SENTINEL = 0x5EA7C0DE
GUARD = 64  # sentinel words on each side of an output


def _guarded(words, n_words=None):
    """An int32 device buffer [1 word | GUARD sentinels | payload | GUARD sentinels], all sentinel but the payload when one
    is given: the payload starts 4 bytes past a 256-byte boundary.  Returns ``(buffer, payload pointer, payload slice)``."""
    import torch

    n = len(words) if words is not None else n_words
    buf = torch.full((1 + GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 256 == 0
    where = slice(1 + GUARD, 1 + GUARD + n)
    if words is not None:
        buf[where] = torch.from_numpy(np.ascontiguousarray(words).view(np.int32).ravel()).cuda()
    ptr = buf.data_ptr() + 4 * (1 + GUARD)
    assert ptr % 256 == 4
    return buf, ptr, where


def _payload(buf, where):
    """The payload of a guarded buffer after a call; everything around it must still be the sentinel."""
    host = buf.cpu().numpy()
    assert np.all(host[:where.start] == SENTINEL) and np.all(host[where.stop:] == SENTINEL), "written outside the output"
    return host[where]


def _raw_single_stage(case, volumes=None):
    """The case through t2fit_resample_dev: source and output 4 bytes off a 256-byte boundary, the output guarded."""
    import torch

    from fetal_t2mapping_amd import _abi
    from fetal_t2mapping_amd._lib import load

    lib = load()
    src = case.src if volumes is None or case.src.ndim == 3 else case.src[:volumes]
    n_vol = src.shape[0] if src.ndim == 4 else 1
    sbuf, sptr, _ = _guarded(src.ravel())
    n_out = n_vol * int(np.prod(case.out_shape))
    obuf, optr, where = _guarded(None, n_out)
    A = (C.c_double * 12)(*case.A.ravel())
    rc = lib.t2fit_resample_dev(sptr, _abi.RESAMPLE_I32 if src.dtype == np.int32 else _abi.RESAMPLE_F32, *src.shape[-3:], A, optr,
                                *case.out_shape, n_vol, _abi.INTERPS[case.interp], float(case.default),
                                _abi.RESAMPLE_INTEGER_CAST if case.integer_cast else 0,
                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.t2fit_last_error().decode()
    torch.cuda.synchronize()
    out = _payload(obuf, where).view(src.dtype if case.interp == "nearest" else np.float32)
    return out.reshape(((n_vol,) if src.ndim == 4 else ()) + case.out_shape)


def _statement(case, volumes=None):
    src = case.src if volumes is None or case.src.ndim == 3 else case.src[:volumes]
    with np.errstate(all="ignore"):
        return R.resample(src, case.A, case.out_shape, case.interp, case.default, case.integer_cast)



@pytest.mark.parametrize("group", sorted(K.SINGLE_STAGE_GROUPS))
def test_single_stage_cases_equal_the_statement_and_meet_the_reference(t2, group):
    """Each case once with all its volumes and, where it has three, once with the first alone (the per-volume offset then
    lands in the second and third volumes' bricks or does not exist).  Equality with the reference on the dyadic cases,
    the bar |got - e| <= ulp32(e)/2 + 32 * 2^-53 * M on the others; nearest by all 32 bits."""
    worst = (0.0, 0.0)
    for case in K.SINGLE_STAGE_GROUPS[group]():
        for volumes in ((None, 1) if case.n_vol == 3 else (None,)):
            got = _raw_single_stage(case, volumes)
            assert K.bits_differ(got, _statement(case, volumes), nan_by_position=case.interp == "linear") == 0, (case, volumes)
            worst = max(worst, K.check(case, got, volumes if case.src.ndim == 4 else None))
            if case.meta is not None:
                K.rim_facts(case, got)
    print(f"{group}: worst ratio to the bar {worst[0]:.4f}, excess over ulp32/2 in units of 32 * 2^-53 * M {worst[1]:.4f}")


def test_wrapper_carries_labels_bit_for_bit_and_refuses_ids_beyond_int32(t2):
    import torch

    lab_case, flt_case = K.nearest_cases()[0], K.nearest_cases()[2]
    g = R.Geometry(lab_case.src.shape[::-1], (2.0, 2.0, 2.0))
    h = R.isotropic_geometry(g, 1.0)
    A = R.index_affine(h, g)
    for src, default in ((lab_case.src, K.INT32_MAX), (lab_case.src, K.INT32_MIN), (flt_case.src, -0.0), (flt_case.src, 1e39)):
        got, _ = t2.resample_volume(src, g, res=1.0, interp="nearest", default=default)
        K.check_nearest(got, K.reference_sample(src, A, h.shape, "nearest"), default)
    # any integer type whose values fit goes through as int32 labels; one whose values do not is refused with their range
    small = np.abs(lab_case.src.astype(np.int64)) % 70000
    want, _ = t2.resample_volume(small.astype(np.int32), g, res=1.0, interp="nearest", default=-1)
    t64 = torch.from_numpy(small)
    for vol in (small, small.astype(np.uint32), small.astype(np.uint64), t64, t64.cuda(), t64.to(torch.uint32).cuda(),
                t64.to(torch.uint64).cuda()):
        got, _ = t2.resample_volume(vol, g, res=1.0, interp="nearest", default=-1)
        if torch.is_tensor(got):
            assert got.dtype == torch.int32 and (got.is_cuda or not vol.is_cuda)
            got = got.cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.any(want > 2 ** 16)
    big = small.copy()
    big[1, 2, 3] = 2 ** 32 + 7
    for vol in (torch.from_numpy(big), torch.from_numpy(big).cuda(), torch.from_numpy(-big).cuda(),
                torch.from_numpy(big).to(torch.uint64).cuda()):
        with pytest.raises(ValueError, match="int32") as err:
            t2.resample_volume(vol, g, res=1.0, interp="nearest")
        assert str(2 ** 32 + 7) in str(err.value)
    big[1, 2, 3] = 2 ** 31 + 5  # fits uint32, not int32
    with pytest.raises(ValueError, match="int32") as err:
        t2.resample_volume(torch.from_numpy(big).to(torch.uint32).cuda(), g, res=1.0, interp="nearest")
    assert f"[0, {2 ** 31 + 5}]" in str(err.value) or str(2 ** 31 + 5) in str(err.value)


def _device_stages(t2, stacks, geoms, kw):
    """The five single-stage calls of the chain, by hand."""
    order, hi, a1, a2 = R.plan(geoms, kw["fixed"], kw["res"], kw["transforms"])
    cast = kw.get("integer_cast", False)
    H = [t2.resample_volume(stacks[o], geoms[o], res=kw["res"], integer_cast=cast)[0] for o in order]
    Rm = [t2.resample_volume(H[m], hi[m], like=hi[0], transform=kw["transforms"].get(order[m]), integer_cast=cast)[0] for m in (1, 2)]
    return {"H": H, "R": Rm}


RECON_REFERENCED = [(f, r, 1, "both") for f in K.RECON_FIXED for r in K.RECON_RES] + [("sag", 1.0, 3, "far"), ("ax", 1.0, 1, "cast")]
RECON_AGREEING = [(f, r, 3, "both") for f in K.RECON_FIXED for r in K.RECON_RES] + [("cor", 0.8, 1, "far"), ("sag", 0.8, 3, "cast")]


@pytest.mark.parametrize("fixed,res,n_vol,kind", RECON_REFERENCED + RECON_AGREEING)
def test_small_ragged_reconstructions_fused_chain_and_statement_agree_and_meet_the_reference(t2, fixed, res, n_vol, kind):
    """(9, 8, 3) stacks of 1 x 1 x 2.5 mm, transforms on both moving stacks: the fixed grid is ragged against the fused
    kernel's 16 x 8 x 4 brick on every axis (at res 1.0 it is (8, 8, 9): two of the axes fill their bricks exactly), the last
    nodes of every stage-1 grid lie outside their stack.  The referenced cases also hold the device's own five stages and
    its merge to the reference, stage 2 from the very stage-1 arrays it read."""
    stacks, geoms, kw = K.recon_case(fixed, res, n_vol, kind)
    with np.errstate(all="ignore"):
        want, _, stages = R.reconstruct(stacks, geoms, return_stages=True, **kw)
    assert K.ragged(want.shape) if res != 1.0 else want.shape[-3:] == (8, 8, 9)
    K.recon_facts(kind, stages)
    fused = t2.reconstruct_stacks(stacks, geoms, form="fused", **kw)[0].cpu().numpy()
    chain = t2.reconstruct_stacks(stacks, geoms, form="chain", **kw)[0].cpu().numpy()
    assert K.bits_differ(fused, want) == 0 and K.bits_differ(chain, want) == 0, (fixed, res, n_vol, kind)
    if (fixed, res, n_vol, kind) in RECON_REFERENCED:
        dev = _device_stages(t2, stacks, geoms, kw)
        for name in ("H", "R"):
            for got, host in zip(dev[name], stages[name]):
                assert K.bits_differ(got, host) == 0, name
        print(f"worst ratio to the bar {K.check_reconstruction(stacks, geoms, kw, fused, dev):.6f}")


@pytest.mark.parametrize("form", ["fused", "chain"])
def test_raw_reconstruction_on_offset_pointers_writes_nothing_outside_its_output(t2, form):
    """Stacks and output 4 bytes off a 256-byte boundary, the output guarded by sentinels; the chain's workspace at the exact
    byte count with sentinels after it."""
    import torch

    from fetal_t2mapping_amd import _abi
    from fetal_t2mapping_amd._lib import load

    lib = load()
    stacks, geoms, kw = K.recon_case("cor", 0.8, 3, "both")
    order, hi, a1, a2 = R.plan(geoms, kw["fixed"], kw["res"], kw["transforms"])
    held = [_guarded(stacks[o].ravel()) for o in order]
    lo_size = (C.c_int32 * 9)(*[v for o in order for v in stacks[o].shape[-3:]])
    hi_size = (C.c_int32 * 9)(*[v for g in hi for v in g.shape])
    A1 = (C.c_double * 36)(*np.concatenate([a.ravel() for a in a1]))
    A2 = (C.c_double * 24)(*np.concatenate([a.ravel() for a in a2]))
    ptrs = (C.c_void_p * 3)(*[ptr for _, ptr, _ in held])
    obuf, optr, where = _guarded(None, 3 * int(np.prod(hi[0].shape)))
    flags = _abi.RECON_CHAIN if form == "chain" else 0
    need = C.c_size_t(0)
    assert lib.t2fit_reconstruct_workspace_bytes(3, lo_size, hi_size, flags, C.byref(need)) == 0
    assert (need.value > 0) == (form == "chain")
    ws = torch.full((need.value + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    rc = lib.t2fit_reconstruct_dev(ptrs, lo_size, A1, hi_size, A2, optr, 3, flags, ws.data_ptr() if need.value else None, need.value,
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.t2fit_last_error().decode()
    torch.cuda.synchronize()
    assert torch.all(ws[need.value:] == 0xA5), "written past the workspace"
    out = _payload(obuf, where).view(np.float32).reshape((3,) + hi[0].shape)
    for buf, _, src_where in held:
        _payload(buf, src_where)
    assert K.bits_differ(out, R.reconstruct(stacks, geoms, **kw)[0]) == 0
