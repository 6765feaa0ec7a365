"""The rigid registration's device half (csrc/t2fit_register.hip) against its numpy statement
(fetal_t2mapping_amd/_register.py), bit for bit: the 43 sums over sizes prime to the brick, several bricks, emptied
bricks, a volume pushed outside and nothing at all; the pyramid levels; the whole registration against the statement's;
raw calls on a caller's stream; recon.py --register on files.  tests/test_register_host.py covers what needs no device."""
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


def _case(name):
    """(fixed, moving, A, fixed mask, moving mask) of a named case."""
    rng = np.random.default_rng(31)
    fshape, mshape = ((40, 48, 70), (37, 50, 66)) if name == "bricks" else ((19, 23, 37), (21, 18, 41))
    fg = R.Geometry(fshape[::-1], (1.0, 1.1, 1.2), tuple(-0.5 * np.array(fshape[::-1])), K.OBLIQUE.ravel())
    mg = R.Geometry(mshape[::-1], (1.1, 1.0, 0.9), tuple(-0.5 * np.array(mshape[::-1])), (K.rot(1, 4.0) @ K.OBLIQUE).ravel())
    shift = {"outside": (14.0, -9.0, 6.0), "nothing": (400.0, 0.0, 0.0)}.get(name, (0.4, -0.7, 0.3))
    a = R.index_affine(fg, mg, K.rigid((3.0, -2.0, 4.0), shift))
    fixed = rng.normal(400, 120, fshape).astype(np.float32)
    moving = rng.normal(400, 120, mshape).astype(np.float32)
    fmask = (rng.random(fshape) < 0.8).astype(np.uint8)
    mmask = (rng.random(mshape) < 0.9).astype(np.uint8)
    if name == "empty_bricks":  # whole bricks of 64 x 4 x 8 without a voxel, and a mask that ends inside a brick
        fmask[:8], fmask[:, 4:13], fmask[9:, :, 30:] = 0, 0, 0
    return fixed, moving, a, fmask, mmask


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
