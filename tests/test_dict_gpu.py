"""The dictionary fit on the device (csrc/t2fit_dict.hip: dict_match_kernel) against its numpy statement
(fetal_t2mapping_amd/_dict.py): index, scale and rmse bit for bit, and equal from call to call, over echo counts (odd
padding, several k-steps), atom counts (a single atom, ragged last tiles), voxel counts (ragged groups and waves), masks
that empty whole groups and workgroups, duplicates, the near-tie case of tests/dict_cases.py, zero / NaN / Inf voxels,
samples over seven decades, raw calls through the C ABI, sample offsets beyond 2^31, fit_volume_dict and the CLI; tables
that take several chunks (near ties, every echo count from 2 to 32 with one and with two chunks, the boundaries of waves
that hold two groups, idle waves, ties between copies in different chunks, 65536 atoms) and magnitudes (samples next to
the largest float, subnormal samples, -0.0, atoms far from unit norm).  tests/test_dict_host.py holds the statement to a
brute-force matcher; tests/test_dict_scores_gpu.py holds the float32 scores of the matrix instruction to their bound."""
import ctypes as C
import os

import numpy as np
import pytest

import dict_cases as K
from fetal_t2mapping_amd import _abi, _dict

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def t2():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X")
    import fetal_t2mapping_amd as t2

    return t2


def _same(got, want, what):
    names = ("index", "scale", "rmse")
    for g, w, n in zip(got, want, names):
        g = g.cpu().numpy() if hasattr(g, "cpu") else np.asarray(g)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, n)
        bad = np.flatnonzero(g.reshape(-1).view(np.uint32) != w.reshape(-1).view(np.uint32))
        assert bad.size == 0, (what, n, bad.size, bad[:5], g.reshape(-1)[bad[:5]], w.reshape(-1)[bad[:5]])


def _check(t2, y, atoms, mask, what):
    want = _dict.match(y, atoms, mask)
    first = t2.dictionary.match(y, atoms, mask)
    _same(first, want, what)
    _same(t2.dictionary.match(y, atoms, mask), want, what + " (again)")
    return want


@pytest.mark.parametrize("n_te", [2, 3, 5, 8, 9, 32])
def test_echo_counts(t2, n_te):
    d = K.atoms_for(100, n_te)
    y = K.decays(n_te, 257, seed=n_te, negate_every=9)
    want = _check(t2, y, d.atoms, K.holes_mask(257, n_te), f"n_te {n_te}")
    assert len(np.unique(want[0])) > 10


@pytest.mark.parametrize("n_atoms", [1, 31, 32, 33, 100, 512])
def test_atom_counts(t2, n_atoms):
    d = K.atoms_for(n_atoms, 6)
    # negated decays: all their scores are negative, so a padded atom of the ragged last tile (score 0) would win if it competed
    y = K.decays(6, 4 * 128 + 1, seed=100 + n_atoms, negate_every=3 if n_atoms == 100 else 7)
    want = _check(t2, y, d.atoms, K.holes_mask(y.shape[1], n_atoms), f"{n_atoms} atoms")
    assert want[0].max() < n_atoms and np.all(want[1][::3 if n_atoms == 100 else 7] == 0)


@pytest.mark.parametrize("n_vox", [1, 31, 33, 257, 4 * 128 + 1])
def test_voxel_counts_without_a_mask(t2, n_vox):
    d = K.atoms_for(33, 5)
    want = _check(t2, K.decays(5, n_vox, seed=n_vox), d.atoms, None, f"{n_vox} voxels")
    assert np.all(want[0] >= 0)


def test_masks_that_empty_groups_waves_and_workgroups(t2):
    d = K.atoms_for(100, 8)
    n_vox = 3 * 512 + 40
    y = K.decays(8, n_vox, seed=77)
    mask = K.holes_mask(n_vox, 78)
    mask[32:64] = 0       # one 32-voxel group
    mask[128:256] = 0     # a whole wave
    mask[512:1024] = 0    # a whole workgroup
    mask[1536:] = 0       # the ragged last workgroup
    want = _check(t2, y, d.atoms, mask, "emptied groups")
    assert np.all(want[0][mask == 0] == -1) and np.all(want[0][mask != 0] >= 0)
    _check(t2, y, d.atoms, np.zeros(n_vox, np.uint8), "an empty mask")
    # 9 echoes are five k-steps (an odd count padded to 10), still four groups per wave: holes at other places
    d9 = K.atoms_for(40, 9)
    y9 = K.decays(9, 700, seed=79)
    m9 = K.holes_mask(700, 80)
    m9[64:128] = 0
    m9[256:512] = 0
    _check(t2, y9, d9.atoms, m9, "emptied groups, 9 echoes")


def test_duplicates_zero_and_non_finite_voxels_and_seven_decades(t2):
    d = K.atoms_for(60, 6)
    atoms = np.concatenate([d.atoms[:40], d.atoms[[5, 17]], d.atoms[40:], d.atoms[[17]]])  # copies of 5 and 17 further up
    rng = np.random.default_rng(5)
    y = K.decays(6, 200, seed=6)
    y[:, 10] = 3.0 * atoms[41]   # exactly a duplicated atom: the lowest index (17) wins
    y[:, 11] = 0.5 * atoms[40]   # (5)
    y[:, 20] = 0.0               # an all-zero voxel: index 0, scale 0
    y[3, 33] = np.nan            # non-finite samples next to good voxels of the same group
    y[0, 40] = np.inf
    y[5, 47] = -np.inf
    y[:, 100:] *= (10.0 ** rng.uniform(-6, 1, 100)).astype(np.float32)[None, :]  # samples from 1e-3 to 1e4
    want = _check(t2, y, atoms, None, "special data")
    assert want[0][10] == 17 and want[0][11] == 5 and want[0][20] == 0 and want[1][20] == 0
    assert list(want[0][[33, 40, 47]]) == [-1, -1, -1] and np.all(want[0][[32, 34, 39, 41, 46, 48]] >= 0)
    span = np.abs(y[:, 100:])
    assert span.max() > 1e3 and span[span > 0].min() < 1e-2


def test_near_ties_need_the_float64_stage(t2):
    atoms, y, index, info = K.near_tie_case()
    y = y.copy()  # (the shared case is read-only; torch wants a writable array)
    want = _dict.match(y, atoms)
    assert np.array_equal(want[0], index) and info["differ"] >= 20
    _same(t2.dictionary.match(y, atoms), want, "near ties")
    _same(t2.dictionary.match(y, atoms), want, "near ties (again)")


@pytest.mark.parametrize("case", K.MULTI_CHUNK_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_near_ties_on_tables_of_several_chunks(t2, case):
    """The near-tie cases whose tables take 2, 7, 9, 16 and 32 chunks (tests/dict_cases.py: the builder asserts on the CPU
    that the float32 chain picks another atom on >= 20 voxels and that the rule with T = 0 misses the statement)."""
    atoms, y, index, info = K.near_tie_case(*case)
    y = y.copy()
    want = _check(t2, y, atoms, None, f"near ties, {info['n_chunks']} chunks")
    assert np.array_equal(want[0], index) and info["n_chunks"] >= 2 and info["differ"] >= 20 and info["t0_misses"] >= 1
    _check(t2, y, atoms, K.holes_mask(y.shape[1], case[3]), f"near ties, {info['n_chunks']} chunks, holes")


@pytest.mark.parametrize("n_te", range(2, 33))
def test_every_instance_with_one_and_two_chunks(t2, n_te):
    """All 16 k-step counts, odd and even echo counts: a table of one chunk, and one of two chunks whose second is short
    and whose last tile is ragged."""
    want = _check(t2, K.decays(n_te, 301, seed=200 + n_te, negate_every=7), K.atoms_for(70, n_te).atoms, K.holes_mask(301, 300 + n_te),
                  f"n_te {n_te}, 70 atoms")
    assert len(np.unique(want[0])) > 10
    tpc = 4096 // ((n_te + n_te % 2) * 32)
    n_atoms = 32 * tpc + 33
    assert K.chunks_of(n_atoms, n_te) == (tpc, 2) and n_atoms <= 2081
    want = _check(t2, K.decays(n_te, 130, seed=400 + n_te), K.atoms_for(n_atoms, n_te).atoms, None, f"n_te {n_te}, {n_atoms} atoms")
    assert len(np.unique(want[0])) > 10 and want[0].min() >= 0


@pytest.mark.parametrize("n_vox", [1, 31, 33, 63, 65, 255, 257, 513])
@pytest.mark.parametrize("n_te", [17, 32])
def test_voxel_counts_with_two_groups_per_wave(t2, n_te, n_vox):
    """Above 16 echoes a wave holds 64 voxels and a workgroup 256; 300 atoms are two chunks at 17 echoes, three at 32."""
    assert K.chunks_of(300, n_te)[1] >= 2
    want = _check(t2, K.decays(n_te, n_vox, seed=n_te * 1000 + n_vox), K.atoms_for(300, n_te).atoms, None, f"{n_te} echoes, {n_vox} voxels")
    assert np.all(want[0] >= 0)


@pytest.mark.parametrize("n_te", [17, 32])
def test_masks_that_empty_groups_waves_and_workgroups_with_two_groups_per_wave(t2, n_te):
    atoms = K.atoms_for(300, n_te).atoms
    n_vox = 3 * 256 + 40
    y = K.decays(n_te, n_vox, seed=500 + n_te)
    mask = K.holes_mask(n_vox, 600 + n_te)
    mask[32:64] = 0       # one 32-voxel group
    mask[128:192] = 0     # a whole wave: it sits through the barriers of every chunk
    mask[256:512] = 0     # a whole workgroup
    mask[768:] = 0        # the ragged last workgroup
    want = _check(t2, y, atoms, mask, f"emptied groups, {n_te} echoes")
    assert np.all(want[0][mask == 0] == -1) and np.all(want[0][mask != 0] >= 0) and len(np.unique(want[0])) > 10
    _check(t2, y, atoms, np.zeros(n_vox, np.uint8), f"an empty mask, {n_te} echoes")


def test_an_idle_wave_sits_through_the_chunks_with_four_groups_per_wave(t2):
    atoms = K.atoms_for(1000, 8).atoms
    assert K.chunks_of(1000, 8) == (16, 2)
    n_vox = 3 * 512 + 40
    y = K.decays(8, n_vox, seed=91)
    mask = K.holes_mask(n_vox, 92)
    mask[128:256] = 0     # a whole wave of the first workgroup
    mask[1024 + 384:1536] = 0  # the last wave of the third
    want = _check(t2, y, atoms, mask, "an emptied wave, 8 echoes, two chunks")
    assert np.all(want[0][mask == 0] == -1) and np.all(want[0][mask != 0] >= 0)


def test_ties_across_chunks(t2):
    atoms, y, index, named = K.cross_chunk_tie_case()
    want = _check(t2, y.copy(), atoms, None, "ties across chunks")
    assert np.array_equal(want[0], index)
    got = t2.dictionary.match(y.copy(), atoms)[0]
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert {n: int(got[v]) for n, (v, _) in named.items()} == {"copy_met_first": 40, "lower_met_first": 110, "ragged_last_tile": 295,
                                                               "last_slot_before_the_break": 287}


def test_samples_next_to_the_largest_float(t2):
    """|y| dmax >= 1e38 on about half of the voxels: there the band is infinite and every atom is re-scored, whatever the
    float32 scores are; the other voxels of the same groups keep a finite band."""
    atoms, y, share = K.huge_case()
    assert 0.2 <= share <= 0.8
    want = _check(t2, y.copy(), atoms, None, "huge samples")
    assert np.all(np.isfinite(want[1])) and np.all(np.isfinite(want[2])) and len(np.unique(want[0])) > 10


@pytest.mark.parametrize("scale", K.TINY_SCALES)
def test_subnormal_samples(t2, scale):
    atoms, y, info = K.tiny_case(scale)
    want = _check(t2, y.copy(), atoms, None, f"samples times {scale}")
    sub = (want[2] > 0) & (want[2] < np.float32(K.SMALLEST_NORMAL))
    assert int(sub.sum()) == info["subnormal_rmse"] and (scale > 1e-40 or sub.any()) and len(np.unique(want[0])) > 10


def test_minus_zero_a_single_subnormal_sample_and_the_largest_float_over_8(t2):
    atoms, y, rows = K.special_rows_case()
    with np.errstate(over="ignore"):  # (one scale is beyond float32 and becomes inf, in the statement as on the device)
        want = _check(t2, y.copy(), atoms, None, "special rows")
    v = rows["minus_zero"]
    assert want[0][v] == 0 and want[1][v].view(np.uint32) == 0 and want[2][v].view(np.uint32) == 0
    assert np.isinf(want[1][rows["plus_minus_max_over_8"]]) and np.all(want[0] >= 0)


@pytest.mark.parametrize("factor", [1e-18, 1e18])
def test_atoms_far_from_unit_norm(t2, factor):
    y = K.decays(6, 300, seed=55)
    want = _check(t2, y, K.scaled_atoms(factor), K.holes_mask(300, 56), f"atoms times {factor}")
    unscaled = _dict.match(y, K.atoms_for(512, 6).atoms, K.holes_mask(300, 56))
    # (the scaled atoms are rounded to float32 once more, so a near tie may fall the other way; elsewhere the scale is the
    # unscaled one over the factor)
    same = (want[0] == unscaled[0]) & (want[0] >= 0)
    assert same.mean() > 0.5 and np.allclose(want[1][same].astype(np.float64) * factor, unscaled[1][same], rtol=1e-5)


@pytest.mark.parametrize("n_te", [2, 32])
def test_the_largest_table(t2, n_te):
    """65536 atoms (T2FIT_DICT_MAX_ATOMS) through the public entry: 2048 tiles in 32 chunks of 64 at 2 echoes, in 512 chunks of 4
    at 32 echoes; atom indices beyond 2^15."""
    atoms = K.atoms_for(_abi.DICT_MAX_ATOMS, n_te).atoms
    want = _check(t2, K.decays(n_te, 96, seed=700 + n_te), atoms, None, f"65536 atoms, {n_te} echoes")
    assert want[0].max() > 32767 and want[0].max() < 65536 and want[0].min() >= 0


def test_raw_calls_and_refusals(t2):
    import torch

    from fetal_t2mapping_amd._lib import load

    lib = load()
    d = K.atoms_for(70, 5)
    n_vox = 301
    y = K.decays(5, n_vox, seed=9)
    mask = K.holes_mask(n_vox, 10)
    want = _dict.match(y, d.atoms, mask)
    dev = torch.device("cuda", 0)
    packed = torch.from_numpy(_dict.pack(d.atoms)).to(dev)
    # buffers at odd element offsets: nothing but 4-byte alignment is asked of y and the outputs
    y_buf = torch.zeros(5 * n_vox + 3, dtype=torch.float32, device=dev)
    y_buf[3:] = torch.from_numpy(y).reshape(-1).to(dev)
    m_buf = torch.zeros(n_vox + 1, dtype=torch.uint8, device=dev)
    m_buf[1:] = torch.from_numpy(mask).to(dev)
    outs = [torch.full((n_vox + 2,), 77, dtype=dt, device=dev) for dt in (torch.int32, torch.float32, torch.float32)]
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        rc = lib.t2fit_dict_match_dev(y_buf.data_ptr() + 12, 5, n_vox, m_buf.data_ptr() + 1, packed.data_ptr(), outs[0].data_ptr() + 4,
                                      outs[1].data_ptr() + 4, outs[2].data_ptr() + 4, C.c_void_p(stream.cuda_stream))
    assert rc == _abi.OK, lib.t2fit_last_error()
    stream.synchronize()
    _same([o[1:-1] for o in outs], want, "raw call")
    assert all(float(o[0]) == 77 and float(o[-1]) == 77 for o in outs)  # nothing written beside the outputs
    args = (m_buf.data_ptr() + 1, packed.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), None)
    # a header that disagrees with n_te, a block that is no dictionary: refused, nothing launched
    assert lib.t2fit_dict_match_dev(y_buf.data_ptr(), 6, n_vox, *args) == _abi.E_INVALID and b"packed for n_te 5" in lib.t2fit_last_error()
    junk = torch.zeros(256, dtype=torch.uint8, device=dev)
    assert lib.t2fit_dict_match_dev(y_buf.data_ptr(), 5, n_vox, m_buf.data_ptr(), junk.data_ptr(), *args[2:]) == _abi.E_INVALID
    assert b"magic" in lib.t2fit_last_error()
    assert lib.t2fit_dict_match_dev(y_buf.data_ptr() + 2, 5, n_vox, *args) == _abi.E_INVALID
    assert lib.t2fit_dict_match_dev(y_buf.data_ptr(), 5, 0, *args) == _abi.OK
    torch.cuda.synchronize()
    assert all(float(o[0]) == 77 for o in outs)
    with pytest.raises(ValueError, match="echoes"):
        t2.dictionary.match(y[:4], d)


def test_sample_offsets_beyond_two_to_the_31(t2):
    """32 echoes of 2^26 + 37 voxels: the element offsets of the late echoes do not fit 32 bits.  Only the first 64 and the last
    600 voxels are in the mask (the rest are zeros and skipped), and those are held to the statement."""
    import torch

    n_te, n_vox = 32, (1 << 26) + 37
    d = K.atoms_for(40, n_te)
    head, tail = K.decays(n_te, 64, seed=31), K.decays(n_te, 600, seed=32)
    dev = torch.device("cuda", 0)
    y = torch.zeros((n_te, n_vox), dtype=torch.float32, device=dev)
    y[:, :64] = torch.from_numpy(head).to(dev)
    y[:, -600:] = torch.from_numpy(tail).to(dev)
    mask = torch.zeros(n_vox, dtype=torch.uint8, device=dev)
    mask[:64] = 1
    mask[-600:] = 1
    index, scale, rmse = t2.dictionary.match(y, d, mask)
    _same((index[:64], scale[:64], rmse[:64]), _dict.match(head, d), "the first voxels")
    _same((index[-600:], scale[-600:], rmse[-600:]), _dict.match(tail, d), "the last voxels")
    assert int((index[64:-600] != -1).sum()) == 0 and not bool(scale[64:-600].any()) and not bool(rmse[64:-600].any())


def test_fit_volume_dict_against_the_statement(t2):
    import torch

    shape = (12, 20, 33)
    n_vox = int(np.prod(shape))
    te = K.echo_times(6)
    d = _dict.biexp(te, _dict.log_grid(30.0, 600.0, 24), 2000.0, np.arange(8) / 8)
    y = K.decays(6, n_vox, seed=21).reshape((6,) + shape)
    mask = K.holes_mask(n_vox, 22).reshape(shape)
    y[2, 3, 4, 5] = np.nan
    mask[3, 4, 5] = 1
    index, scale, rmse = _dict.match(y, d, mask)
    want = _dict.lookup(d, index)
    maps, extras = t2.dictionary.fit_volume_dict(y, mask, d)
    assert isinstance(maps, t2.T2Maps) and set(extras) == {"fraction", "index"}
    assert maps.t2.tobytes() == want["t2"].tobytes() and extras["fraction"].tobytes() == want["fraction"].tobytes()
    assert extras["index"].tobytes() == index.tobytes() and maps.k.tobytes() == scale.tobytes() and maps.res.tobytes() == rmse.tobytes()
    assert maps.sigma.shape == shape and not maps.sigma.any()
    status = np.where(index >= 0, _abi.ST_CONVERGED, np.where(mask != 0, _abi.ST_NONFINITE, _abi.ST_MASKED)).astype(np.uint8)
    assert np.array_equal(maps.status, status) and status[3, 4, 5] == _abi.ST_NONFINITE
    # tensors in, tensors out
    maps_t, extras_t = t2.dictionary.fit_volume_dict(torch.from_numpy(y).cuda(), torch.from_numpy(mask).cuda(), d)
    assert maps_t.t2.is_cuda and maps_t.t2.cpu().numpy().tobytes() == want["t2"].tobytes()
    assert extras_t["index"].cpu().numpy().tobytes() == index.tobytes()
    with pytest.raises(ValueError, match="t2"):
        t2.dictionary.fit_volume_dict(y, mask, _dict.Dictionary(d.atoms, d.params[:, 1:], ("fraction",)))


def _tree(tmp_path, shape=(12, 20, 33)):
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


def test_cli_writes_the_maps_of_the_statement(t2, tmp_path, monkeypatch):
    import sys

    from fetal_t2mapping_amd import cli as R

    monkeypatch.setitem(sys.modules, "SimpleITK", None)

    def run(name, extra):
        root, out, echoes, mask, te = _tree(tmp_path / name)
        base = ["--csv", "log.csv", "--in_vivo", "--gaussian", "--lf", "--sim", "d1", "--TEs"] + [str(int(t)) for t in te]
        R.main(["--path", root] + base + extra)
        return out, echoes, mask, te

    out, echoes, mask, te = run("mono", ["--solver", "dict", "--dict_t2", "20:2000:96"])
    union = t2.stack_mask_flatten(list(echoes), [mask] * 3)[1]
    d = _dict.monoexp(te, _dict.log_grid(20.0, 2000.0, 96))
    index, scale, rmse = _dict.match(echoes, d, union)
    assert sorted(f.split("_ada-")[0].split("_")[-1] for f in os.listdir(out)) == ["dictindexmap", "kmap", "resmap", "sigmamap", "t2map"]
    assert _read(out, "t2").tobytes() == _dict.lookup(d, index)["t2"].tobytes() and _read(out, "k").tobytes() == scale.tobytes()
    assert _read(out, "res").tobytes() == rmse.tobytes() and not _read(out, "sigma").any()
    got_index = _read(out, "dictindex")
    assert got_index.dtype == np.int32 and got_index.tobytes() == index.tobytes() and (index >= 0).sum() > 100

    out, echoes, mask, te = run("csf", ["--solver", "dict", "--dict_t2", "30:600:24", "--dict_csf", "2000:8"])
    d = _dict.biexp(te, _dict.log_grid(30.0, 600.0, 24), 2000.0, np.arange(8) / 8)
    index, scale, rmse = _dict.match(echoes, d, union)
    want = _dict.lookup(d, index)
    assert len(os.listdir(out)) == 6
    assert _read(out, "t2").tobytes() == want["t2"].tobytes() and _read(out, "fraction").tobytes() == want["fraction"].tobytes()
    assert _read(out, "dictindex").tobytes() == index.tobytes() and _read(out, "k").tobytes() == scale.tobytes()
    assert _read(out, "res").tobytes() == rmse.tobytes()
