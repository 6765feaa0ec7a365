"""The rigid registration's device half (csrc/t2fit_register.hip) against its numpy statement
(fetal_t2mapping_amd/_register.py), bit for bit: the 43 sums over sizes prime to the brick, several bricks, emptied
bricks, a volume pushed outside and nothing at all, two reduction passes with a ragged last group, degenerate and edge
geometry, unaligned pointers; and against the sums restated from their definition (register_cases.reference_sums), which
is all that holds the three-pass case; the pyramid levels; the whole registration against the statement's; raw calls on
a caller's stream; recon.py --register on files.  tests/test_register_host.py covers what needs no device."""
import ctypes as C
import os

import numpy as np
import pytest

import register_cases as K
from fetal_t2mapping_amd import _register as G
from fetal_t2mapping_amd import _resample as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def t2():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X")
    import fetal_t2mapping_amd as t2

    return t2


_case = K.case


def _place(t, offset):
    """A copy of the numpy array ``t`` in device memory that starts ``offset`` bytes past a 256-byte boundary:
    ``(keep-alive tensor, pointer)``."""
    import torch

    raw = np.ascontiguousarray(t).view(np.uint8).ravel()
    buf = torch.empty(raw.size + 512, dtype=torch.uint8, device="cuda")
    start = (-buf.data_ptr()) % 256 + offset
    buf[start:start + raw.size].copy_(torch.from_numpy(raw.copy()))
    assert (buf.data_ptr() + start) % 256 == offset % 256
    return buf, buf.data_ptr() + start


def _raw_sums(name, offsets=(0, 0, 0, 0)):
    """t2fit_register_sums_dev on a caller's stream and buffers; the workspace is exactly t2fit_register_workspace_bytes
    long and filled with NaN bytes, so a pass that reads a value no kernel wrote shows.  ``offsets``: bytes past a
    256-byte boundary of the fixed, fixed-mask, moving and moving-mask pointers."""
    import torch

    from fetal_t2mapping_amd._lib import load

    lib = load()
    fixed, moving, a, fmask, mmask = K.case(name)
    need = C.c_size_t(0)
    assert lib.t2fit_register_workspace_bytes(*fixed.shape, C.byref(need)) == 0 and need.value == G.workspace_bytes(fixed.shape)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        keep = [_place(v, o) for v, o in zip((fixed, fmask, moving, mmask), offsets)]
        ws = torch.full((need.value + 256,), 0xFF, dtype=torch.uint8, device="cuda")
        ws_ptr = (ws.data_ptr() + 255) // 256 * 256
        ws = ws[:ws_ptr - ws.data_ptr() + need.value]
        sums = torch.full((43,), np.nan, dtype=torch.float64, device="cuda")
        A = (C.c_double * 12)(*np.asarray(a).ravel())
        assert lib.t2fit_register_sums_dev(keep[0][1], keep[1][1], *fixed.shape, keep[2][1], keep[3][1], *moving.shape, A,
                                           sums.data_ptr(), ws_ptr, need.value, C.c_void_p(stream.cuda_stream)) == 0
    stream.synchronize()
    return sums.cpu().numpy()


def _device_sums(t2, name):
    fixed, moving, a, fmask, mmask = K.case(name)
    return t2.register.registration_sums(fixed, moving, a, fixed_mask=fmask, moving_mask=mmask)


def _assert_bits(got, want, name):
    diff = np.flatnonzero(K.bits(got) != K.bits(want))
    assert diff.size == 0, (name, diff, got[diff], want[diff])


@pytest.mark.parametrize("name", ["prime", "bricks", "empty_bricks", "outside", "nothing"])
def test_sums_are_bit_equal_to_the_statement_and_repeat(t2, name):
    fixed, moving, a, fmask, mmask = _case(name)
    want = G.registration_sums(fixed, moving, a, fmask, mmask)
    got = t2.register.registration_sums(fixed, moving, a, fixed_mask=fmask, moving_mask=mmask)
    again = t2.register.registration_sums(fixed, moving, a, fixed_mask=fmask, moving_mask=mmask)
    assert got.dtype == np.float64 and got.shape == (43,)
    diff = np.flatnonzero(K.bits(got) != K.bits(want))
    assert diff.size == 0, (name, diff, got[diff], want[diff])
    assert got.tobytes() == again.tobytes()
    if name != "nothing":
        K.assert_within_reference(got, name)  # independent of the statement: how far the kernel may ever drift
    n_all = fmask.sum()
    if name == "nothing":  # N = 0: zeros from the raw call, an error -- not a NaN transform -- from the registration
        assert got.tobytes() == np.zeros(43).tobytes()
        g = R.Geometry(fixed.shape[::-1])
        far = R.Geometry(moving.shape[::-1], origin=(900.0, 0.0, 0.0))
        with pytest.raises(ValueError, match="no voxel to compare"):
            t2.register.register_rigid(fixed, moving, g, far, fixed_mask=fmask, moving_mask=mmask, levels=(1,))
    else:  # the case is not a trivial one: many voxels count, many do not, and every defined sum is something
        assert 1000 < got[0] < 0.6 * n_all and np.all(got[1:42] != 0) and got[42] == 0


def test_masks_default_to_all_ones_and_tensors_are_taken(t2):
    import torch

    fixed, moving, a, _, _ = _case("prime")
    want = G.registration_sums(fixed, moving, a)
    got = t2.register.registration_sums(torch.from_numpy(fixed).cuda(), torch.from_numpy(moving).cuda(), a)
    assert np.array_equal(K.bits(got), K.bits(want))


@pytest.mark.parametrize("name", K.TWO_PASS)
def test_two_reduction_passes_with_a_ragged_last_group(t2, name):
    """774 slabs reduce as [774, 4] (the last group of the first pass holds 6 values), 257 as [257, 2] (one value): the
    second pass, its workspace offset, the stride of an intermediate pass and the zero fill beyond n all run."""
    fixed, _, _, fmask, _ = K.case(name)
    slabs = int(np.prod(G.brick_counts(fixed.shape)))
    passes = G.pass_sizes(slabs)
    print(f"{name}: fixed {fixed.shape}, {slabs} slabs, passes {passes}")
    assert passes == {"tail774": [774, 4], "tail257": [257, 2]}[name]
    assert np.all(K.counted_per_slab(name)[slabs // 256 * 256:] > 0)  # the ragged group is not a group of zeros
    want = K.statement_sums(name)
    got, again, raw = _device_sums(t2, name), _device_sums(t2, name), _raw_sums(name)
    _assert_bits(got, want, name)
    assert got.tobytes() == again.tobytes()
    _assert_bits(raw, want, name)  # on a caller's stream, the workspace NaN before the call
    K.assert_within_reference(got, name)
    assert 1000 < got[0] < 0.6 * fmask.sum() and np.all(got[1:42] != 0) and got[42] == 0


def test_three_reduction_passes_against_the_reference(t2):
    """(2035, 1034, 3): 255 x 259 x 1 = 66045 slabs, passes [66045, 258, 2].  The numpy statement pads every brick to 64
    lanes and is too slow here, so no bit-equality is claimed: the device is held to the reference under the tolerance
    of the statement.  The fixed mask is sparse, but every group of 256 slabs of the first pass, and so every value of
    the second and the third, has voxels that count."""
    name = "three_pass"
    fixed = K.case(name)[0]
    slabs = int(np.prod(G.brick_counts(fixed.shape)))
    assert G.brick_counts(fixed.shape) == (255, 259, 1) and G.pass_sizes(slabs) == [66045, 258, 2]
    per_slab = K.counted_per_slab(name)
    groups = np.add.reduceat(per_slab, np.arange(0, slabs, 256))
    assert per_slab[0] > 0 and per_slab[-1] > 0 and groups.size == 258 and np.all(groups > 0)
    got = _raw_sums(name)
    print(f"{name}: {slabs} slabs, passes {G.pass_sizes(slabs)}, {per_slab.sum()} voxels count, at least {groups.min()} per group")
    K.assert_within_reference(got, name)
    assert got[0] == per_slab.sum() > 10000 and np.all(got[1:42] != 0) and got[42] == 0
    assert _raw_sums(name).tobytes() == got.tobytes()


@pytest.mark.parametrize("name", K.DEGENERATE + ("integer_eps",))
def test_edge_geometry_is_bit_equal_to_the_statement(t2, name):
    """A moving axis of one voxel, fixed volumes smaller than a brick down to one voxel, a second x-brick of one lane,
    one exact brick, whole-voxel translations next to Inf and NaN, coordinates exactly on the rim."""
    want = K.statement_sums(name)
    got = _device_sums(t2, name)
    if name == "integer_eps":  # off the nodes by 2^-40 the non-finite nodes have a weight: the same sums are lost
        assert np.array_equal(np.isfinite(got), np.isfinite(want)) and not np.all(np.isfinite(got))
        _assert_bits(got[np.isfinite(got)], want[np.isfinite(want)], name)
        return
    _assert_bits(got, want, name)
    assert np.all(np.isfinite(got)) and got[0] == K.counted_per_slab(name).sum()
    K.assert_within_reference(got, name)
    _assert_bits(_raw_sums(name), want, name)
    if name.startswith("moving_"):
        assert got[0] > 5000


def test_unaligned_volumes_and_masks(t2):
    """Volumes 4 bytes past a 256-byte boundary and masks at odd addresses (all the ABI asks of them): byte for byte the
    result of the aligned call."""
    for name in ("prime", "fixed_9x6x65"):
        aligned = _raw_sums(name)
        _assert_bits(aligned, K.statement_sums(name), name)
        assert _raw_sums(name, offsets=(4, 1, 260, 3)).tobytes() == aligned.tobytes()
        assert _raw_sums(name, offsets=(252, 255, 4, 129)).tobytes() == aligned.tobytes()


@pytest.mark.parametrize("s", K.PYRAMID_FACTORS)
def test_pyramid_levels_at_odd_factors_and_the_limits(t2, s):
    """s = 3 and 5 divide by 27 and 125, which rounds; s = 1 copies; s = 32 is the largest the ABI takes.  Raw calls and
    DevicePyramid.level against the statement bit for bit, and -- independently of it -- against the exactly summed block
    means: at most 1 float32 ulp from the correctly rounded mean (tests/test_register_host.py derives the bound)."""
    import torch

    from fetal_t2mapping_amd._gpu_register import DevicePyramid
    from fetal_t2mapping_amd._lib import load

    lib = load()
    v, m = K.pyramid_case(s)
    shape = G.level_shape(v.shape, s)
    tv, tm = torch.from_numpy(v).cuda(), torch.from_numpy(m).cuda()
    ov = torch.full(shape, np.nan, dtype=torch.float32, device="cuda")
    om = torch.full(shape, 7, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.t2fit_shrink_dev(tv.data_ptr(), *v.shape, s, ov.data_ptr(), st) == 0
    assert lib.t2fit_shrink_mask_dev(tm.data_ptr(), *m.shape, s, om.data_ptr(), st) == 0
    lv, lm = DevicePyramid(v, m, v, m, torch.device("cuda", 0)).level(s)[:2]
    want_v, want_m = G.shrink(v, s), G.shrink_mask(m, s)
    for got_v, got_m in ((ov, om), (lv, lm)):
        assert tuple(got_v.shape) == tuple(got_m.shape) == shape
        assert np.array_equal(got_v.cpu().numpy().view(np.uint32), want_v.view(np.uint32))
        assert np.array_equal(got_m.cpu().numpy(), want_m)
    ulps = np.abs(K.ordered(ov.cpu().numpy()) - K.ordered(K.block_means(s)))
    print(f"s = {s}: level {shape}, {np.count_nonzero(ulps)} of {ulps.size} block means are not the correctly rounded one")
    assert ulps.max() <= 1
    assert 0 < int(om.sum().item()) < om.numel() and set(np.unique(om.cpu().numpy())) == {0, 1}


def test_registration_with_an_odd_level_equals_the_statement(t2):
    fixed, moving, g, fmask, mmask = K.recovery_pair()
    kw = dict(fixed_mask=fmask, moving_mask=mmask, levels=(3, 1), max_iter=25)
    want = G.register_rigid(fixed, moving, g, g, **kw)
    got = t2.register.register_rigid(fixed, moving, g, g, **kw)
    assert got.parameters.tobytes() == want.parameters.tobytes() and got.transform.tobytes() == want.transform.tobytes()
    assert got.iterations == want.iterations and got.stops == want.stops and got.metric == want.metric
    assert got.iterations[0] > 0 and got.iterations[1] > 0


@pytest.mark.parametrize("s", [2, 4])
def test_pyramid_levels_are_bit_equal_to_the_statement(t2, s):
    import torch

    from fetal_t2mapping_amd._gpu_register import DevicePyramid

    rng = np.random.default_rng(32)
    v = rng.normal(300, 80, (19, 23, 37)).astype(np.float32)
    m = (rng.random(v.shape) < 0.03).astype(np.uint8)
    p = DevicePyramid(v, m, v, m, torch.device("cuda", 0))
    lv, lm = p.level(s)[:2]
    assert tuple(lv.shape) == G.level_shape(v.shape, s)
    assert np.array_equal(lv.cpu().numpy().view(np.uint32), G.shrink(v, s).view(np.uint32))
    assert np.array_equal(lm.cpu().numpy(), G.shrink_mask(m, s)) and 0 < lm.sum().item() < lm.numel()


def test_registration_equals_the_statement_and_recovers_the_transform(t2):
    fixed, moving, g, fmask, mmask = K.recovery_pair()
    kw = dict(fixed_mask=fmask, moving_mask=mmask, levels=(2, 1), max_iter=40)
    want = G.register_rigid(fixed, moving, g, g, **kw)
    got = t2.register.register_rigid(fixed, moving, g, g, **kw)
    assert got.parameters.tobytes() == want.parameters.tobytes() and got.transform.tobytes() == want.transform.tobytes()
    assert got.iterations == want.iterations and got.stops == want.stops and got.metric == want.metric
    tre = G.target_registration_error(got.transform, K.RECOVERY_TRUE, fmask, g)
    print(got, f"TRE {tre:.4f} mm")
    assert tre < 0.5
    # masks built on the device are the statement's
    auto = t2.register.register_rigid(fixed, moving, g, g, levels=(2, 1), max_iter=40)
    assert auto.parameters.tobytes() == want.parameters.tobytes()


def test_raw_calls_with_caller_owned_buffers_on_another_stream(t2):
    import torch

    from fetal_t2mapping_amd._lib import load

    lib = load()
    fixed, moving, a, fmask, mmask = _case("prime")
    want = G.registration_sums(fixed, moving, a, fmask, mmask)
    need = C.c_size_t(0)
    assert lib.t2fit_register_workspace_bytes(*fixed.shape, C.byref(need)) == 0 and need.value == G.workspace_bytes(fixed.shape)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        f, fm = torch.from_numpy(fixed).cuda(), torch.from_numpy(fmask).cuda()
        m, mm = torch.from_numpy(moving).cuda(), torch.from_numpy(mmask).cuda()
        ws = torch.empty(need.value + 256, dtype=torch.uint8, device="cuda")
        sums = torch.full((43,), np.nan, dtype=torch.float64, device="cuda")
        half = torch.empty(G.level_shape(fixed.shape, 2), dtype=torch.float32, device="cuda")
        A = (C.c_double * 12)(*np.asarray(a).ravel())
        st = C.c_void_p(stream.cuda_stream)
        assert lib.t2fit_register_sums_dev(f.data_ptr(), fm.data_ptr(), *fixed.shape, m.data_ptr(), mm.data_ptr(), *moving.shape, A,
                                           sums.data_ptr(), (ws.data_ptr() + 255) // 256 * 256, need.value, st) == 0
        assert lib.t2fit_shrink_dev(f.data_ptr(), *fixed.shape, 2, half.data_ptr(), st) == 0
    stream.synchronize()
    assert np.array_equal(K.bits(sums.cpu().numpy()), K.bits(want))
    assert np.array_equal(half.cpu().numpy().view(np.uint32), G.shrink(fixed, 2).view(np.uint32))


def test_recon_register_undoes_a_moved_cor_stack(t2, tmp_path, monkeypatch):
    import sys

    monkeypatch.setitem(sys.modules, "SimpleITK", None)  # the package's NIfTI reader

    import test_recon_gpu as RG
    from fetal_t2mapping_amd import nifti, recon

    true = K.rigid((2.0, -1.5, 2.5), (1.5, -1.0, 1.2))
    stacks, geoms, _, _, _, _ = RG._phantom_stacks(n_te=1, side=48, thick=4.0, seed=25)
    cor = geoms["cor"]
    moved = dict(geoms, cor=R.Geometry(cor.GetSize(), cor.GetSpacing(), true[:3, :3] @ np.array(cor.GetOrigin()) + true[:3, 3],
                                       (true[:3, :3] @ np.array(cor.GetDirection()).reshape(3, 3)).ravel()))
    unmoved, _ = R.reconstruct(stacks, geoms)

    def run(name, geoms_on_disk, **kw):
        bids, md = RG._write_subject(tmp_path / name, stacks, geoms_on_disk, [114], None)
        (path,) = recon.process_recon(md, bids, denoise=False, **kw)
        return np.asarray(nifti.ReadImage(path).arr, np.float32), md

    tdir = str(tmp_path / "found")
    plain, _ = run("plain", moved)
    registered, md = run("registered", moved, register=True, write_transforms=tdir)
    inner = (slice(6, -6),) * 3
    mae = lambda a: float(np.mean(np.abs(a[inner].astype(np.float64) - unmoved[0][inner])))
    acq = md[md["ImageOrientationPatientSTR"] == "ax"].iloc[0]
    found = recon.load_transforms(tdir, acq, "ax")
    iso = R.isotropic_geometry(geoms["ax"], 1.0)
    h_ax = R.resample(stacks["ax"][0], R.index_affine(iso, geoms["ax"]), iso.shape)
    tre = G.target_registration_error(found["cor"], true, G.build_mask(h_ax), iso)
    print(f"MAE plain {mae(plain):.3f} registered {mae(registered):.3f}; TRE cor {tre:.3f} mm")
    assert sorted(found) == ["cor", "sag"] and os.path.basename(recon.transform_path(tdir, acq, "cor", echo=True)) == \
        "sub-001_ses-01_te-114_cor.txt"
    assert mae(registered) < mae(plain)
    assert tre < 1.0
    # the written transforms read back through --transforms give the registered merge again, byte for byte
    reread, _ = run("reread", moved, transforms_dir=tdir)
    assert reread.tobytes() == registered.tobytes()
    # the merge given the true transform is the yardstick the found one is measured against
    np.savetxt(recon.transform_path(str(tmp_path), acq, "cor"), true, fmt="%.17g")
    ideal, _ = run("ideal", moved, transforms_dir=str(tmp_path))
    assert mae(ideal) < mae(plain)
    # every echo onto the first: the same volume twice stays where it is
    import torch

    merged, _, _ = recon.merge_echoes({o: np.concatenate([stacks[o], stacks[o]]) for o in stacks}, geoms, [acq, acq],
                                      register_echoes=True)
    torch.cuda.synchronize()
    assert torch.equal(merged[0], merged[1])
