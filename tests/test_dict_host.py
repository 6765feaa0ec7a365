"""The dictionary fit without a GPU: the numpy statement (fetal_t2mapping_amd/_dict.py) against a brute-force matcher in
Python floats, the packed block against t2fit_dict_pack_host byte for byte, the refusals through both, the builders, the
two-compartment model against the mono-exponential one, save / load, the CLI flags, and the cases that show why the
float32 scores of the matrix instruction need the float64 re-score and that its bound holds, on a table of one chunk and
on tables of several, ties across chunks, and the conditions of the magnitude cases (tests/dict_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import dict_cases as K
from fetal_t2mapping_amd import _abi, _dict


@pytest.fixture(scope="module")
def lib():
    from fetal_t2mapping_amd import build
    from fetal_t2mapping_amd._lib import load

    build.build()
    return load()


def test_statement_equals_the_brute_force_matcher():
    d = K.atoms_for(37, 5)
    atoms = np.concatenate([d.atoms, d.atoms[[3, 20]]])  # duplicates: the lowest index wins
    y = K.decays(5, 41, seed=3, negate_every=5)
    y[:, 7] = 0.0
    y[2, 9] = np.nan
    y[0, 11] = np.inf
    y[:, 13] = 2.0 * atoms[38]  # a decay that is exactly a duplicated atom (38 is a copy of 20)
    mask = K.holes_mask(41, 4)
    mask[[7, 9, 11, 13]] = 1
    want = K.brute_force(y, atoms, mask)
    got = _dict.match(y, atoms, mask)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    assert got[0][7] == 0 and got[1][7] == 0 and got[0][9] == -1 and got[0][11] == -1 and got[0][13] == 20
    assert np.all(got[0][mask == 0] == -1) and np.all(got[1][mask == 0] == 0) and np.all(got[2][mask == 0] == 0)
    neg = np.arange(0, 41, 5)
    neg = neg[(mask[neg] != 0) & (neg != 0)]
    assert neg.size and np.all(got[1][neg] == 0)  # the scale is not below 0
    no_mask = _dict.match(y.reshape(5, 1, 41), atoms)
    assert no_mask[0].shape == (1, 41) and np.array_equal(no_mask[0].reshape(-1)[mask != 0], got[0][mask != 0])


@pytest.mark.parametrize("n_atoms,n_te", [(1, 2), (31, 3), (32, 8), (33, 5), (100, 6), (512, 9), (70, 32)])
def test_pack_equals_the_library_byte_for_byte(lib, n_atoms, n_te):
    from fetal_t2mapping_amd import _gpu_dict

    atoms = K.atoms_for(n_atoms, n_te).atoms
    want = _dict.pack(atoms)
    need = C.c_size_t(0)
    assert lib.t2fit_dict_pack_bytes(n_atoms, n_te, C.byref(need)) == _abi.OK and need.value == want.size
    got = _gpu_dict.pack(atoms)
    assert got.dtype == np.uint8 and got.tobytes() == want.tobytes()
    k_pad, n_tiles, off_tiles, off_atoms, off_norm2, nbytes = _dict.layout(n_atoms, n_te)
    assert (k_pad, n_tiles, off_tiles) == (n_te + n_te % 2, -(-n_atoms // 32), 64) and nbytes == want.size
    tiles = want[off_tiles:off_atoms].view(np.float32).reshape(n_tiles, k_pad, 32)
    dh = _dict.normalise(atoms)[0]
    j = n_atoms - 1
    assert np.array_equal(tiles[j // 32, :n_te, j % 32], dh[j]) and np.all(tiles[:, n_te:, :] == 0)
    assert np.all(tiles.transpose(0, 2, 1).reshape(-1, k_pad)[n_atoms:] == 0)  # the padded rows of a ragged last tile


def test_refusals_through_the_statement_and_the_library(lib):
    from fetal_t2mapping_amd import _gpu_dict

    bad = [np.ones((4, 1), np.float32), np.ones((4, 33), np.float32), np.ones((0, 4), np.float32), np.ones((65537, 2), np.float32)]
    zero = np.ones((5, 4), np.float32)
    zero[3] = 0
    nan = np.ones((5, 4), np.float32)
    nan[2, 1] = np.nan
    for atoms, word in [(a, "1 .. 65536") for a in bad] + [(zero, "atom 3 has norm 0"), (nan, "atom 2 has a non-finite")]:
        for fn in (_dict.pack, _gpu_dict.pack):
            with pytest.raises(ValueError, match=word):
                fn(atoms)
    need = C.c_size_t(0)
    for a, m in ((0, 4), (65537, 4), (4, 1), (4, 33)):
        assert lib.t2fit_dict_pack_bytes(a, m, C.byref(need)) == _abi.E_INVALID
    assert lib.t2fit_dict_pack_bytes(4, 4, None) == _abi.E_INVALID
    good = np.ones((5, 4), np.float32)
    assert lib.t2fit_dict_pack_bytes(5, 4, C.byref(need)) == _abi.OK
    buf = np.zeros(need.value, np.uint8)
    assert lib.t2fit_dict_pack_host(5, 4, good.ctypes.data, buf.ctypes.data, need.value - 1) == _abi.E_INVALID
    assert b"bytes" in lib.t2fit_last_error()
    assert lib.t2fit_dict_pack_host(5, 4, None, buf.ctypes.data, need.value) == _abi.E_INVALID
    assert lib.t2fit_dict_pack_host(5, 4, good.ctypes.data, None, need.value) == _abi.E_INVALID
    assert lib.t2fit_dict_pack_host(5, 4, good.ctypes.data, buf.ctypes.data, need.value) == _abi.OK
    # the device entry refuses what needs no kernel before HIP is touched (no GPU here)
    p8, p16 = C.c_void_p(8), C.c_void_p(64)
    call = lib.t2fit_dict_match_dev
    assert call(None, 4, 10, None, p16, p8, p8, p8, None) == _abi.E_INVALID
    assert call(p8, 4, 10, None, None, p8, p8, p8, None) == _abi.E_INVALID
    assert call(p8, 4, 10, None, p16, None, p8, p8, None) == _abi.E_INVALID
    assert call(p8, 1, 10, None, p16, p8, p8, p8, None) == _abi.E_INVALID and b"n_te" in lib.t2fit_last_error()
    assert call(p8, 33, 10, None, p16, p8, p8, p8, None) == _abi.E_INVALID
    assert call(p8, 4, -1, None, p16, p8, p8, p8, None) == _abi.E_INVALID
    assert call(C.c_void_p(6), 4, 10, None, p16, p8, p8, p8, None) == _abi.E_INVALID and b"aligned" in lib.t2fit_last_error()
    assert call(p8, 4, 10, None, p16, p8, C.c_void_p(10), p8, None) == _abi.E_INVALID
    assert call(p8, 4, 10, None, C.c_void_p(72), p8, p8, p8, None) == _abi.E_INVALID and b"16 bytes" in lib.t2fit_last_error()
    assert set(_abi.DICT_SYMBOLS) <= {n for n, _, _ in _abi.SYMBOLS} and _abi.DICT_MAX_ATOMS == 65536


def test_builders_and_exact_recovery_on_the_grid():
    grid = _dict.log_grid(20.0, 2000.0, 96)
    assert grid[0] == 20.0 and grid[-1] == 2000.0 and np.allclose(np.diff(np.log(grid)), np.log(100.0) / 95)
    d = _dict.monoexp(K.TE6, grid)
    assert d.atoms.shape == (96, 6) and d.atoms.dtype == np.float32 and d.names == ("t2",)
    assert np.array_equal(d.atoms, np.exp(-K.TE6[None, :] / grid[:, None]).astype(np.float32))
    pick = np.array([0, 17, 50, 95])
    # a power of two times the atom itself: the scale comes back exactly
    y = (4.0 * d.atoms[pick].astype(np.float64)).astype(np.float32).T
    index, scale, rmse = _dict.match(y, d)
    assert np.array_equal(index, pick) and np.all(scale == 4.0) and np.all(rmse == 0.0)
    assert np.array_equal(_dict.lookup(d, index)["t2"], grid[pick].astype(np.float32))
    with pytest.raises(ValueError):
        _dict.log_grid(0.0, 10.0, 4)
    with pytest.raises(ValueError):
        _dict.biexp(K.TE6, grid, 2000.0, [0.0, 1.0])
    with pytest.raises(ValueError, match="echoes"):
        _dict.match(np.ones((5, 3), np.float32), d)


def test_two_compartments_recover_t2_and_fraction_where_one_cannot():
    grid = _dict.log_grid(40.0, 400.0, 64)
    fractions = np.arange(32) / 32
    bi = _dict.biexp(K.TE6, grid, 2000.0, fractions)
    mono = _dict.monoexp(K.TE6, grid)
    assert bi.atoms.shape == (64 * 32, 6) and bi.names == ("t2", "fraction")
    assert np.array_equal(bi.params[:, 0].reshape(64, 32)[:, 0], grid.astype(np.float32))
    cases = [(10, 8), (30, 16), (50, 4), (20, 24)]  # (T2 index, fraction index), fraction > 0
    y = np.stack([512.0 * ((1 - fractions[f]) * np.exp(-K.TE6 / grid[t]) + fractions[f] * np.exp(-K.TE6 / 2000.0)) for t, f in cases],
                 axis=1).astype(np.float32)
    index, scale, _ = _dict.match(y, bi)
    maps = _dict.lookup(bi, index)
    want_t2 = np.array([grid[t] for t, _ in cases], np.float32)
    assert np.array_equal(maps["t2"], want_t2)
    assert np.array_equal(maps["fraction"], np.array([fractions[f] for _, f in cases], np.float32))
    assert np.allclose(scale, 512.0, rtol=1e-6)
    mono_t2 = _dict.lookup(mono, _dict.match(y, mono)[0])["t2"]
    assert np.all(np.abs(maps["t2"] - want_t2) == 0) and np.all(np.abs(mono_t2 - want_t2) > 0)
    assert np.all(mono_t2 > want_t2)  # the long component pulls a single exponential up


def test_dictionary_save_load_round_trip(tmp_path):
    d = _dict.biexp(K.TE6, _dict.log_grid(30.0, 300.0, 7), 1800.0, [0.0, 0.25, 0.5])
    path = str(tmp_path / "d.npz")
    d.save(path)
    back = _dict.Dictionary.load(path)
    assert back.names == d.names and back.atoms.tobytes() == d.atoms.tobytes() and back.params.tobytes() == d.params.tobytes()
    assert back.n_atoms == 21 and back.n_te == 6 and np.array_equal(back.column("fraction"), d.params[:, 1])
    with pytest.raises(KeyError):
        back.column("t1")
    with pytest.raises(ValueError):
        _dict.Dictionary(d.atoms, d.params[:5], d.names)
    with pytest.raises(ValueError):
        _dict.Dictionary(d.atoms, d.params, ("t2",))


def test_cli_flags(tmp_path, capsys):
    from fetal_t2mapping_amd import cli as R

    base = ["--path", str(tmp_path), "--csv", "log.csv", "--in_vivo", "--lf", "--sim", "1"]
    args = R.parse_arguments(base + ["--gaussian", "--solver", "dict", "--dict_t2", "20:2000:512"])
    assert args.solver == "dict" and args.dict_args == {"t2": (20.0, 2000.0, 512), "csf": None}
    args = R.parse_arguments(base + ["--gaussian", "--solver", "dict", "--dict_t2", "40:400:64", "--dict_csf", "2000:32"])
    assert args.dict_args == {"t2": (40.0, 400.0, 64), "csf": (2000.0, 32)}
    d = R.build_dictionary(args.dict_args, [114.0, 202.0, 299.0])
    assert d.atoms.shape == (2048, 3) and d.names == ("t2", "fraction") and d.params[:, 1].max() == np.float32(31 / 32)
    assert R.parse_arguments(base + ["--gaussian"]).dict_args is None
    three = str(tmp_path / "three.npz")
    _dict.monoexp([114.0, 202.0, 299.0], _dict.log_grid(20.0, 2000.0, 50)).save(three)
    args = R.parse_arguments(base + ["--gaussian", "--solver", "dict", "--dict_file", three])
    assert args.dict_args == {"file": three} and R.build_dictionary(args.dict_args, [114.0, 202.0, 299.0]).n_atoms == 50
    six = str(tmp_path / "six.npz")
    _dict.monoexp(K.TE6, [50.0, 100.0]).save(six)
    no_t2 = str(tmp_path / "no_t2.npz")
    _dict.Dictionary(np.ones((2, 3), np.float32), np.ones((2, 1), np.float32), ("t1",)).save(no_t2)
    refused = [
        (["--rician", "--solver", "dict", "--dict_t2", "20:2000:64"], "--gaussian only"),
        (["--gaussian_rician", "--solver", "dict", "--dict_t2", "20:2000:64"], "--gaussian only"),
        (["--gaussian", "--solver", "dict"], "needs a dictionary"),
        (["--gaussian", "--solver", "dict", "--dict_t2", "20:2000:64", "--dict_file", three], "needs a dictionary"),
        (["--gaussian", "--solver", "dict", "--dict_file", six], "6 echoes per atom, 3 echoes are fitted"),
        (["--gaussian", "--solver", "dict", "--dict_file", three, "--TEs", "100", "200"], "3 echoes per atom, 2 echoes are fitted"),
        (["--gaussian", "--solver", "dict", "--dict_file", no_t2], "no t2 column"),
        (["--gaussian", "--solver", "dict", "--dict_file", str(tmp_path / "missing.npz")], "missing.npz"),
        (["--gaussian", "--solver", "dict", "--dict_t2", "20:2000"], "expected LO:HI:N"),
        (["--gaussian", "--solver", "dict", "--dict_t2", "20:2000:64", "--dict_csf", "2000"], "expected T2LONG:NF"),
        (["--gaussian", "--solver", "dict", "--dict_t2", "20:2000:4096", "--dict_csf", "2000:32"], "more than 65536"),
        (["--gaussian", "--solver", "dict", "--dict_file", three, "--dict_csf", "2000:8"], "goes with --dict_t2"),
        (["--gaussian", "--solver", "lm", "--dict_t2", "20:2000:64"], "no effect without --solver dict"),
        (["--gaussian", "--solver", "dict", "--dict_t2", "20:2000:64", "--bootstrap", "8"], "--bootstrap"),
        (["--gaussian", "--solver", "dict", "--dict_t2", "20:2000:64", "--norm"], "--norm"),
    ]
    for extra, word in refused:
        with pytest.raises(SystemExit):
            R.parse_arguments(base + extra)
        assert word in capsys.readouterr().err, extra
    with pytest.raises(ValueError, match="6 echoes per atom"):
        R.build_dictionary({"file": six}, [114.0, 202.0, 299.0])


def test_float32_scores_need_the_float64_stage_and_the_bound_holds():
    """512 log-spaced atoms, 6 echoes, 2000 noisy voxels: the builder asserts that the exact float32 fma chain picks another
    atom than the statement on at least 20 voxels, that the statement's winner lies within T of the best float32 score on
    every voxel, and that the kernel's tile-by-tile rule on those scores returns the statement's index everywhere."""
    atoms, y, index, info = K.near_tie_case()
    assert atoms.shape == (512, 6) and y.shape == (6, 2000) and info["differ"] >= 20
    assert 1 <= info["rescored_mean"] <= 64 and info["rescored_max"] < 512  # the rule selects, it does not re-score everything
    # and a band of zero would not do: the rule then misses the statement's atom somewhere
    dh, _, dmax = _dict.normalise(atoms)
    got, _ = K.candidate_rule(K.chain32(dh, y, 6), _dict.scores(dh, y), np.zeros(2000, np.float32), 6)
    assert np.any(got != index)


@pytest.mark.parametrize("case", K.MULTI_CHUNK_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_float32_scores_need_the_float64_stage_on_tables_of_several_chunks(case):
    """The same three assertions of the builder on tables that the kernel walks in 2, 7, 9, 16 and 32 chunks (17 and 32
    echoes: two groups per wave; 65536 atoms: the largest table), where the tiles are visited out of index order; the builder
    also asserts that the table needs at least two chunks and that the rule with T = 0 misses the statement's atom."""
    n_atoms, n_te, n_vox, _ = case
    atoms, y, index, info = K.near_tie_case(*case)
    assert atoms.shape == (n_atoms, n_te) and y.shape == (n_te, n_vox) and index.shape == (n_vox,)
    assert info["n_chunks"] == K.chunks_of(n_atoms, n_te)[1] >= 2 and info["differ"] >= 20 and info["t0_misses"] >= 1
    assert info["rescored_max"] < n_atoms  # the rule selects, it does not re-score everything
    assert index.min() >= 0 and index.max() < n_atoms and len(np.unique(index)) > 10


def test_ties_across_chunks_go_to_the_lowest_index():
    """Duplicates whose copies sit in other chunks (the builder asserts the statement's index on the four named voxels, that
    the scores of the copies are equal, and that the tile-by-tile rule reproduces the statement)."""
    atoms, y, index, named = K.cross_chunk_tie_case()
    assert atoms.shape == (300, 32) and K.chunks_of(300, 32) == (4, 3)
    assert np.array_equal(atoms[104], atoms[40]) and np.array_equal(atoms[142], atoms[110])
    assert {n: int(index[v]) for n, (v, _) in named.items()} == {"copy_met_first": 40, "lower_met_first": 110,
                                                                 "ragged_last_tile": 295, "last_slot_before_the_break": 287}
    # the walk: tile 3 (chunk 0) before tile 1 (chunk 1); tile 3 before tile 4; tile 9 is ragged; tile 8 ends chunk 2
    order = [slot * 3 + c for c in range(3) for slot in range(4) if slot * 3 + c < 10]
    assert order == [0, 3, 6, 9, 1, 4, 7, 2, 5, 8]
    assert order.index(104 // 32) < order.index(40 // 32) and order.index(110 // 32) < order.index(142 // 32)
    for v, j in named.values():  # the brute-force matcher agrees on the ties
        assert K.brute_force(y[:, v:v + 1], atoms)[0][0] == j


def test_magnitude_cases_reach_what_they_are_for():
    """The builders of the magnitude cases assert their own conditions: the share of voxels beyond |y| dmax = 1e38 (between
    20 % and 80 %, finite samples, finite scale and rmse without a numpy warning), the subnormal shares of the tiny samples
    and a subnormal rmse, the special rows, and atoms far from unit norm with finite non-zero squared norms."""
    assert 0.2 <= K.huge_case()[2] <= 0.8
    shares = [K.tiny_case(s)[2] for s in K.TINY_SCALES]
    assert shares[0]["subnormal_samples"] < 0.01 < 0.1 < shares[1]["subnormal_samples"] < 0.5 < 0.9 < shares[2]["subnormal_samples"]
    assert any(s["subnormal_rmse"] >= 1 for s in shares)
    atoms, y, rows = K.special_rows_case()
    assert np.all(y[:, rows["minus_zero"]].view(np.uint32) == 0x80000000)
    for factor in (1e-18, 1e18):
        n2 = _dict.normalise(K.scaled_atoms(factor))[1]
        assert n2.max() < 1e-30 if factor < 1 else n2.min() > 1e20


def test_fma_emulation_is_exact_on_hard_roundings():
    # ties of the final rounding that only the sticky bit decides, and cancellation
    a = np.array([1 + 2.0 ** -23, 1 + 2.0 ** -12, 3.0, 1 + 2.0 ** -23], np.float32)
    b = np.array([1 + 2.0 ** -23, 1 + 2.0 ** -12, 1 / 3, 1 - 2.0 ** -24], np.float32)
    c = np.array([2.0 ** -24, -1.0, -1.0, -1.0], np.float32)
    from fractions import Fraction

    got = K.fma32(a, b, c)
    for i in range(4):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        near = np.float32(float(exact))  # (these cases are exact in float64 or far from a float32 tie after it)
        lo, hi = np.nextafter(near, np.float32(-np.inf)), np.nextafter(near, np.float32(np.inf))
        best = min((lo, near, hi), key=lambda f: (abs(Fraction(float(f)) - exact), int(np.float32(f).view(np.uint32)) & 1))
        assert got[i] == best, i
