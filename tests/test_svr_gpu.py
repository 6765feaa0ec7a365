"""Slice-to-volume registration on the device (svr_sums_kernel of csrc/t2fit_register.hip behind t2fit_svr_sums_dev) against
its numpy statement (fetal_t2mapping_amd/_svr.py), bit for bit: three stacks of unequal brick counts in one launch with the
poses mixed on purpose and the masks given and NULL; a slice of 257 bricks (two reduction passes); six stacks of 1 to 12
slices; inactive and out-of-range records; permuted records; the raw entry point on pointers off a 256-byte boundary, masks
at odd addresses, guarded outputs, a second stream and a NaN-filled workspace; the lockstep descent against the statement's;
and the driver on the phantom that moved between slices.  tests/test_svr_host.py covers what needs no device."""
import ctypes as C

import numpy as np
import pytest

import sr_slice_cases as L
import svr_cases as W
from fetal_t2mapping_amd import _resample as R
from fetal_t2mapping_amd import _svr as V
from test_bootstrap_edges_gpu import _odd_mask
from test_recon_gpu import _guarded, _payload
from test_sr_gpu import _guarded64
from test_svr_host import _same, check_recovery, check_status

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def t2():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X")
    import fetal_t2mapping_amd as t2

    return t2


@pytest.fixture(scope="module")
def mixed():
    b = W.mixed_batch()
    return b, V.slice_sums(b.stacks, b.volume, b.A, b.stack, b.slice, stack_masks=b.masks, volume_mask=b.volume_mask)


def test_mixed_batch_equals_the_statement_bit_for_bit(t2, mixed):
    b, want = mixed
    assert sorted({int(np.prod(V.slice_brick_counts(*g.shape[1:]))) for g in b.geoms}) == [1, 2, 4]  # the reduction is zero-padded
    assert want[2, 0] == 0 and want[4, 0] == 0 and 0 < want[3, 0] < want[0, 0] and np.all(want[5:, 0] > 0)
    got = t2.register.slice_sums(b.stacks, b.volume, b.A, b.stack, b.slice, stack_masks=b.masks, volume_mask=b.volume_mask)
    assert got.shape == (len(b.A), 43) and got.dtype == np.float64 and _same(got, want)
    assert not np.any(np.signbit(got[[2, 4]])) and not np.any(got[:, 42])
    for masks, vmask in ((None, None), ([b.masks[0], None, b.masks[2]], None), (None, b.volume_mask)):
        want_m = V.slice_sums(b.stacks, b.volume, b.A, b.stack, b.slice, stack_masks=masks, volume_mask=vmask)
        got_m = t2.register.slice_sums(b.stacks, b.volume, b.A, b.stack, b.slice, stack_masks=masks, volume_mask=vmask)
        assert _same(got_m, want_m) and not _same(got_m, want)


def test_permuted_inactive_and_out_of_range_records(t2, mixed):
    from fetal_t2mapping_amd._gpu_register import DeviceSlices

    import torch

    b, want = mixed
    n = len(b.A)
    order = np.random.default_rng(4).permutation(n)
    got = t2.register.slice_sums(b.stacks, b.volume, b.A[order], b.stack[order], b.slice[order], stack_masks=b.masks,
                                 volume_mask=b.volume_mask)
    assert _same(got, want[order])
    active = np.ones(n, np.uint8)
    active[[0, 6]] = 0
    got = t2.register.slice_sums(b.stacks, b.volume, b.A, b.stack, b.slice, active=active, stack_masks=b.masks, volume_mask=b.volume_mask)
    keep = [r for r in range(n) if r not in (0, 6)]
    assert _same(got[[0, 6]], np.zeros((2, 43))) and _same(got[keep], want[keep])
    # the packing refuses what is out of range; a table that holds it anyway is data: rows of +0.0, the rest untouched
    with pytest.raises(ValueError, match="stack index"):
        t2.register.slice_sums(b.stacks, b.volume, b.A, np.where(b.stack == 2, 3, b.stack), b.slice)
    with pytest.raises(ValueError, match="non-finite"):
        t2.register.slice_sums(b.stacks, b.volume, np.where(np.arange(12).reshape(3, 4) == 5, np.nan, b.A), b.stack, b.slice)
    table = V.pack_table(b.A, b.stack, b.slice, None, [g.shape for g in b.geoms]).reshape(n, 128).copy()
    words, doubles = table.view(np.int32), table.view(np.float64)
    words[1, 24], words[7, 24], words[8, 25], words[9, 25], words[10, 24] = 3, -1, 4, -2 ** 31, 2 ** 31 - 1
    doubles[5, 6], doubles[11, 0] = np.nan, np.inf
    zero = [1, 7, 8, 9, 10, 5, 11]
    dev = DeviceSlices(b.stacks, b.masks, b.volume, b.volume_mask, n, torch.device("cuda", 0))
    got = dev.sums_of_table(table)
    keep = [r for r in range(n) if r not in zero]
    assert _same(got[zero], np.zeros((len(zero), 43))) and _same(got[keep], want[keep])


def test_a_slice_of_257_bricks_takes_two_reduction_passes(t2):
    rng = np.random.default_rng(6)
    stack = rng.normal(500, 200, (1, 8224, 3)).astype(np.float32)
    volume = rng.normal(500, 200, (4, 5, 6)).astype(np.float32)
    mask = (rng.random(stack.shape) > 0.1).astype(np.uint8)
    a = np.array([[4.0 / 3, 0, 0, 0.3], [0, 3.0 / 8224, 0.1, 0.2], [0.01, 0, 1.0, 0.6]])[None]
    assert V.workspace_bytes([stack.shape], 1) == (43 * 8 * 257 + 255) // 256 * 256 + (43 * 8 * 2 + 255) // 256 * 256
    want = V.slice_sums([stack], volume, a, [0], [0], stack_masks=[mask])
    got = t2.register.slice_sums([stack], volume, a, [0], [0], stack_masks=[mask])
    assert want[0, 0] == np.count_nonzero(mask) and _same(got, want)


def test_six_stacks_of_1_to_12_slices(t2):
    rng = np.random.default_rng(7)
    hr = R.Geometry((20, 18, 16), (1.0, 1.0, 1.0), (-9.0, -8.0, -7.0))
    sizes = [(9, 7, 1), (70, 5, 12), (8, 35, 3), (5, 5, 7), (66, 34, 2), (3, 9, 5)]
    stacks = [rng.normal(500, 200, s[::-1]).astype(np.float32) for s in sizes]
    volume = rng.normal(500, 200, hr.shape).astype(np.float32)
    records = [(s, k) for s, size in enumerate(sizes) for k in range(size[2])]
    rng.shuffle(records)
    s_of, k_of = np.array(records, np.int32).T
    a = np.stack([[[16.0 / sizes[s][0], 0.05, 0.3, 1.0 + 0.1 * k], [-0.04, 14.0 / sizes[s][1], 0.2, 1.5], [0.02, 0.03, 0.9, 2.0 + 0.2 * s]]
                  for s, k in records])
    want = V.slice_sums(stacks, volume, a, s_of, k_of)
    got = t2.register.slice_sums(stacks, volume, a, s_of, k_of)
    assert len(records) == 30 and np.all(want[:, 0] > 0) and _same(got, want)


def test_raw_call_on_offset_pointers_guarded_outputs_and_a_second_stream(t2, mixed):
    import torch

    from fetal_t2mapping_amd._lib import load

    lib = load()
    b, want = mixed
    n, n_s = len(b.A), len(b.stacks)
    shapes = [g.shape for g in b.geoms]
    fixed = [_guarded(v.ravel()) for v in b.stacks]           # 4 bytes past a 256-byte boundary
    masks = [_odd_mask(m) for m in b.masks]                   # 1 byte past one
    moving, vmask = _guarded(b.volume.ravel()), _odd_mask(b.volume_mask)
    obuf, optr, where = _guarded64(43 * n)                    # 8 bytes past one, between sentinels
    table = torch.from_numpy(V.pack_table(b.A, b.stack, b.slice, None, shapes)).cuda()
    nbytes = V.workspace_bytes(shapes, n)
    ws = torch.full((nbytes // 8 + 32,), float("nan"), dtype=torch.float64, device="cuda")
    ws_ptr = (ws.data_ptr() + 255) // 256 * 256
    assert table.data_ptr() % 8 == 0 and all(f[1] % 256 == 4 for f in fixed) and all(m[1] % 2 == 1 for m in masks)
    lo = (C.c_int32 * (3 * n_s))(*[d for s in shapes for d in s])
    side = torch.cuda.Stream()
    results = []
    for stream in (torch.cuda.current_stream(), side, side):
        torch.cuda.synchronize()
        ws.fill_(float("nan"))
        obuf[where] = -1
        torch.cuda.synchronize()
        rc = lib.t2fit_svr_sums_dev(n_s, (C.c_void_p * n_s)(*[f[1] for f in fixed]), (C.c_void_p * n_s)(*[m[1] for m in masks]), lo,
                                    moving[1], vmask[1], *b.volume.shape, table.data_ptr(), n, optr, ws_ptr, nbytes,
                                    C.c_void_p(stream.cuda_stream))
        assert rc == 0, lib.t2fit_last_error().decode()
        stream.synchronize()
        results.append(_payload(obuf, where).copy().view(np.float64).reshape(n, 43))
        for buf, _, inside in fixed + [moving]:               # the inputs are untouched
            assert buf.cpu().numpy()[inside].tobytes() in (b.volume.tobytes(),) + tuple(v.tobytes() for v in b.stacks)
    assert _same(results[0], want) and _same(results[1], want) and _same(results[2], want)


@pytest.fixture(scope="module")
def problem_statement():
    c = W.problem()
    return c, V.register_slices(c.stacks, c.geoms, c.volume, c.hr, transforms=c.transforms, stack_masks=c.masks)


def test_register_slices_equals_the_statement_slice_for_slice(t2, problem_statement):
    c, want = problem_statement
    got = t2.register.register_slices(c.stacks, c.geoms, c.volume, c.hr, transforms=c.transforms, stack_masks=c.masks)
    for o in c.geoms:
        assert got.status[o] == want.status[o] and np.array_equal(got.iterations[o], want.iterations[o])
        assert _same(got.parameters[o], want.parameters[o]) and _same(got.transforms[o], want.transforms[o])
        assert _same(got.metric[o], want.metric[o]) and _same(got.centres[o], want.centres[o])
    assert max(int(v.max()) for v in want.iterations.values()) > 10
    # from the true poses nothing moves; tensors in, and the masks built on the device where none are given
    import torch

    stay = t2.register.register_slices({o: torch.from_numpy(v).cuda() for o, v in c.stacks.items()}, c.geoms, torch.from_numpy(c.volume).cuda(),
                                       c.hr, transforms=c.transforms, stack_masks=c.masks, init=c.true)
    for o in c.geoms:
        assert np.max(np.abs(stay.parameters[o] - c.true[o])) <= 1e-9 and np.max(np.abs(stay.metric[o] + 1.0)) <= 1e-12
    built = t2.register.register_slices(c.stacks, c.geoms, c.volume, c.hr, transforms=c.transforms, max_iter=3)
    built_want = V.register_slices(c.stacks, c.geoms, c.volume, c.hr, transforms=c.transforms, max_iter=3)
    for o in c.geoms:
        assert built.status[o] == built_want.status[o] and _same(built.parameters[o], built_want.parameters[o])


def test_status_of_slices_that_cannot_be_registered_on_the_device(t2):
    c = W.problem()
    plain = V.register_slices({"a": c.stacks["a"]}, {"a": c.geoms["a"]}, c.volume, c.hr, stack_masks={"a": c.masks["a"]})
    check_status(t2.register.register_slices, plain)


def test_one_round_on_the_moved_phantom_equals_the_statement_and_recovers(t2):
    stacks, geoms, truth, grid, _ = L.moved_phantom()
    want, hi, want_found = W.phantom_statement(1)
    got, header, found = t2.sr.reconstruct_svr(stacks, geoms, rounds=1, slice_masks=W.phantom_masks(), n_iter=W.SVR_N_ITER,
                                               prox_iter=W.SVR_PROX_ITER)
    got = got.cpu().numpy()
    assert header.GetOrigin() == hi.GetOrigin() and got.shape == (1, 48, 48, 48)
    for o in geoms:
        assert found.status[o] == want_found.status[o] and np.array_equal(found.iterations[o], want_found.iterations[o])
        assert _same(found.parameters[o], want_found.parameters[o]) and _same(found.transforms[o], want_found.transforms[o])
    assert np.array_equal(got.view(np.uint32), np.asarray(want).reshape(got.shape).view(np.uint32))
    merge = t2.reconstruct_stacks(stacks, geoms)[0].cpu().numpy()
    plain = t2.reconstruct_sr(stacks, geoms, n_iter=W.SVR_N_ITER, prox_iter=W.SVR_PROX_ITER)[0].cpu().numpy()
    check_recovery(got, None, header, found, None, merge, plain, None)


def test_estimate_slices_flag_writes_poses_that_the_slice_transforms_flag_reads_back(t2, tmp_path, monkeypatch):
    import os
    import sys

    monkeypatch.setitem(sys.modules, "SimpleITK", None)  # the package's NIfTI reader; an earlier test may have faked one

    import sr_cases as K
    from fetal_t2mapping_amd import nifti, recon
    from test_recon_gpu import _write_subject

    stacks, geoms, _, _, _, _ = K._phantom_stacks(n_te=2, side=32, thick=4.0, seed=27)
    te_ms = [114, 202]
    bids, md = _write_subject(tmp_path, stacks, geoms, te_ms, None)
    pose_dir = str(tmp_path / "found")
    base = ["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo", "--lf", "--recon_method", "sr", "--sr_iter", "1", "--sr_weight", "8"]

    def run(extra):
        args = recon.parse_arguments(base + extra)
        written = recon.process_recon(md, bids, denoise=False, sr=args.sr_args)
        return [np.asarray(nifti.ReadImage(p).arr, np.float32) for p in written]

    plain = run([])
    found = run(["--sr_estimate_slices", "1", "--sr_write_slice_transforms", pose_dir])
    names = sorted(os.listdir(pose_dir))
    assert names == [f"sub-001_ses-01_te-{t}_{o}_slices.txt" for t in te_ms for o in ("ax", "cor", "sag")]
    assert len(open(os.path.join(pose_dir, names[0])).read().splitlines()) == geoms["ax"].shape[0]
    again = run(["--sr_slice_transforms", pose_dir])
    for i in range(2):
        assert np.array_equal(again[i].view(np.uint32), found[i].view(np.uint32)) and not np.array_equal(found[i], plain[i])
    want = V.reconstruct_svr(stacks, geoms, rounds=1, weight=8.0, n_iter=1)
    got = recon.load_slice_transforms(pose_dir, {"sub": "sub-001", "ses": "ses-01", "EchoTime": 0.202}, geoms)
    for o in geoms:
        assert _same(got[o], want[2].transforms[o])
