"""N4 bias-field correction without a device: the numpy statement (fetal_t2mapping_amd/_bias.py) against the independent
reference of tests/bias_cases.py, mutations of the statement that must each fail it, the sharpening table against a
direct DFT, the refinement, degenerate masks, the recovery of a known field, the C ABI's symbols, workspace arithmetic and
refusals through the loaded library, the flags of recon.py and cli.py, and the driver over tests/fake_sitk.py."""
import ctypes as C
import sys

import numpy as np
import pytest

import bias_cases as K
from fetal_t2mapping_amd import _abi, _bias


# ---- the statement against the reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("side", K.SIDES)
@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_statement_equals_the_reference(shape, side):
    """Histogram exact; delta, omega, the field and the sums within TOL * sum |terms| (bias_cases.TOL)."""
    for kind in ("rows", "one"):
        ratios = K.check_statement(shape, side, kind)
        print(shape, side, kind, {k: f"{v:.2e}" for k, v in ratios.items()})
    K.check_cannot_hide(shape, side)


def test_the_measured_ratio_is_the_largest_the_statement_shows():
    """TOL is 16 times MEASURED_RATIO; the ratio is reached (to the digits written) on the case named beside it."""
    worst = max(K.statement_ratios((40, 48, 70), 7, "one").values())
    assert 0.9 * K.MEASURED_RATIO <= worst <= K.MEASURED_RATIO


@pytest.mark.parametrize("name", sorted(K.MUTATIONS))
def test_a_mutated_statement_fails(name):
    """Each mutation fails on the two shapes with a ragged group of lanes.  Two of them put a zero weight one node past
    the lattice / the table: numpy raises IndexError there, which fails the statement as an assertion does."""
    for shape, side in (((7, 5, 65), 5), ((2, 3, 257), 19)):
        K.check_statement(shape, side)
        with K.mutated(name), pytest.raises((AssertionError, IndexError)):
            K.check_statement(shape, side)
        K.check_statement(shape, side)  # (the statement is itself again)


def test_bin_coordinate_and_histogram_edges():
    u = np.array([[[1.0, 2.0, 1.5, 1.0 + 1.0 / 398.0, 2.0 - 1e-7, 0.5, 3.0]]], np.float32)
    m = np.ones(u.shape, np.uint8)
    slope = _bias.slope_of(1.0, 2.0)
    i, t = _bias.bin_coords(u, 1.0, slope)
    assert i.ravel().tolist()[:3] == [0, 198, 99] and t.ravel()[0] == 0.0 and t.ravel()[1] == 1.0  # c = B - 1: bin B - 2, t = 1
    assert i.ravel().tolist()[5:] == [0, 198] and t.ravel()[5] == 0.0 and t.ravel()[6] == 1.0      # clamped
    hist = _bias.histogram(u, m, 1.0, slope)
    assert int(hist.sum()) == 7 << 24 and int(hist[199]) >= 2 << 24 and int(hist[0]) >= 2 << 24
    assert [int(h) for h in hist] == K.ref_histogram(u, m, 1.0, slope, 200)
    m[0, 0, 1] = 0
    assert int(_bias.histogram(u, m, 1.0, slope).sum()) == 6 << 24
    with pytest.raises(ValueError, match="flat"):
        _bias.slope_of(1.0, 1.0)


def test_histogram_of_the_case_past_the_grid_cap_equals_the_reference():
    """The flat case of 1024 x 2048 + 2049 voxels that tests/test_bias_gpu.py holds the device to: its conditions (the
    extremes unique and past the 1024 x 2048 voxels of the kernels' first eight trips), and the statement's histogram
    against the Python loop."""
    u, m = K.capped_case()
    lo, hi, slope = K.check_capped()
    hist = _bias.histogram(u, m, float(lo), slope)
    assert [int(h) for h in hist] == K.ref_histogram(u, m, float(lo), slope, _bias.BINS)
    assert int(hist.sum()) == int(m.sum()) << 24 and int(hist[0]) >= 1 << 24 and int(hist[-1]) >= 1 << 24
    head = np.array(m)
    head[..., K.CAPPED_GRID_VOXELS:] = 0  # without the tail: another range and another histogram
    assert _bias.minmax(u, head) != (lo, hi) and not np.array_equal(_bias.histogram(u, head, float(lo), slope), hist)


# ---- the table -------------------------------------------------------------------------------------------------------------
def _dft(x, sign=-1.0):
    n = len(x)
    k = np.arange(n)
    return np.exp(sign * 2j * np.pi * np.outer(k, k) / n) @ np.asarray(x, complex)


def test_table_against_a_direct_dft():
    u0, m, lo, slope, _ = K.setup((19, 23, 37))
    hist = _bias.histogram(u0, m, lo, slope)
    for fwhm in (0.15, 0.5):
        fast = _bias.sharpen_table(hist, lo, slope, fwhm)
        slow = _bias.sharpen_table(hist, lo, slope, fwhm, fft=_dft, ifft=lambda x: _dft(x, 1.0) / len(x))
        assert fast.shape == (200,) and np.all(np.isfinite(fast))
        # Compared on the bins a voxel reads with a weight that is not 0 -- those with mass in the histogram.  Elsewhere
        # E is the quotient of two sums that both vanish, which no transform pins.  An O(P^2) DFT of P = 512 terms of
        # magnitude <= N = 1e4 carries about P eps N = 1e-9 absolute, against den of order 1 per voxel there.
        live = hist > 0
        print(fwhm, "table, fft against direct DFT:", np.max(np.abs(fast - slow)[live]))
        assert np.max(np.abs(fast - slow)[live]) <= 1e-9 * np.max(np.abs(fast))
    assert _bias.padded_size(200) == 512 and _bias.padded_size(256) == 512 and _bias.padded_size(257) == 1024
    # a sharpened value pulls towards the modes: the table is monotone where the histogram has mass
    live = hist > 0
    assert np.all(np.diff(_bias.sharpen_table(hist, lo, slope, 0.15)[live]) >= -1e-9)


# ---- refinement, degenerate masks --------------------------------------------------------------------------------------------
def test_refinement_keeps_the_field():
    shape = (9, 14, 21)
    lat = K.lattice_of(4)
    want = _bias.field_eval(lat, shape, store=np.float64)
    for side in K.SIDES[1:]:
        lat = _bias.refine(lat)
        assert lat.shape == (side,) * 3
        assert np.max(np.abs(_bias.field_eval(lat, shape, store=np.float64) - want)) <= 1e-12
    with pytest.raises(ValueError, match="above 19"):
        _bias.refine(lat)
    with pytest.raises(ValueError, match="max_iter"):
        _bias.check_options(0.15, (1,) * 6, 1e-3, 200, 0.01, 1.0)


def test_degenerate_masks():
    shape = (6, 7, 9)
    u = np.full(shape, 2.0, np.float32)
    one = np.zeros(shape, np.uint8)
    one[3, 3, 4] = 1
    for side in (4, 7):
        omega = _bias.fit_weights(one, side)
        delta = _bias.fit_delta(u, one, side)
        assert 0 < np.count_nonzero(omega) <= 64 and np.all(delta[omega == 0] == 0)
        lat = _bias.lattice_update(np.zeros((side,) * 3), delta, omega)
        assert np.all(lat[omega == 0] == 0) and np.all(np.isfinite(lat))  # omega = 0 nodes give 0
        # one voxel: MBA reproduces the value there exactly enough (phi = w v / sum w^2, then sum w phi = v)
        assert abs(float(_bias.field_eval(lat, shape)[3, 3, 4]) - 2.0) < 1e-6
    empty = np.zeros(shape, np.uint8)
    assert not _bias.fit_weights(empty, 4).any() and _bias.minmax(u, empty) == (np.inf, -np.inf)
    assert _bias.convergence(0.0, 0.0, 1) == 0.0 and _bias.convergence(0.0, 0.0, 0) == 0.0
    vol = np.full(shape, 100.0, np.float32)
    with pytest.raises(ValueError, match="flat"):  # a flat image has no histogram
        _bias.n4_correct(vol, np.ones(shape, np.uint8))
    with pytest.raises(ValueError, match="flat"):  # .. nor has one voxel
        _bias.n4_correct(vol, one)
    with pytest.raises(ValueError, match="finite"):
        _bias.n4_correct(np.where(one, np.nan, vol), np.ones(shape, np.uint8))
    u0, m = _bias.log_image(np.array([[[4.0, 0.0, -1.0, 1.0]]], np.float32), np.array([[[1, 1, 1, 0]]]))
    assert m.ravel().tolist() == [1, 0, 0, 0] and u0.ravel().tolist() == [np.float32(np.log(4.0)), 0.0, 0.0, 0.0]


# ---- recovery ----------------------------------------------------------------------------------------------------------------
def test_recovery_of_a_known_field():
    """Full defaults at fwhm = 0.15 on the 32 x 40 x 48 three-class ball.  Measured here with the statement (the bars in
    bias_cases.check_recovery are set from these): iterations (37, 11, 3, 3), 1 - corr 4.36e-4, CV of the brightest class
    0.0493 -> 0.00507.  Two facts about the method on this phantom, recorded and not chased: the budget (8, 6, 4) leaves
    1 - corr = 4.05e-3 and CV 0.00867; fwhm = 0.5 makes this phantom worse (corr 0.384, CV 0.0733)."""
    vol, mask, cls, logf = K.recovery_phantom()
    found = _bias.n4_correct(vol, mask)
    print("iterations", found.iterations)
    before, after, miss = K.check_recovery(found.corrected, found.log_field)
    assert found.iterations == (37, 11, 3, 3)
    assert abs(after - K.RECOVERY_CV_AFTER) < 5e-5 and abs(miss - K.RECOVERY_ONE_MINUS_CORR) < 5e-6  # the record is current
    assert found.lattice.shape == (11, 11, 11) and len(found.convergence) == 4
    assert all(c[-1] <= 1e-3 for c in found.convergence)
    # the whole-call test on the device needs every figure at least 1e-6 away from the threshold
    assert min(abs(c - 1e-3) for level in found.convergence for c in level) >= 1e-6
    assert np.array_equal(found.corrected, _bias.apply_field(vol, found.log_field))
    short = _bias.n4_correct(vol, mask, max_iter=(8, 6, 4), scale=0.25)
    assert short.iterations == (8, 6, 4) and short.lattice.shape == (7, 7, 7)
    assert np.array_equal(short.corrected, _bias.apply_field(vol, short.log_field, 0.25))
    print("short budget: 1 - corr", 1 - K.field_correlation(short.log_field, logf, mask), "CV", K.class_cv(short.corrected, cls))


# ---- the C ABI without a device ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from fetal_t2mapping_amd import build
    from fetal_t2mapping_amd._lib import load

    build.build()
    return load()


def test_symbol_group():
    assert len(_abi.N4_SYMBOLS) == 8 and all(n.startswith("t2fit_n4_") for n in _abi.N4_SYMBOLS)
    assert set(_abi.N4_SYMBOLS) <= {n for n, _, _ in _abi.SYMBOLS} and set(_abi.N4_SYMBOLS) <= set(_abi.LOOKED_UP)
    assert not set(_abi.N4_SYMBOLS) & set(_abi.ADDITIVE)
    assert sorted(n for n, _, _ in _abi.SYMBOLS if "_n4_" in n) == sorted(_abi.N4_SYMBOLS)


def test_workspace_arithmetic(lib):
    need = C.c_size_t(0)
    for shape in K.SHAPES + [(57, 256, 256), (256, 256, 256), (1, 1, 1), (300, 300, 3)]:
        for side in K.SIDES:
            assert lib.t2fit_n4_workspace_bytes(*shape, side, C.byref(need)) == _abi.OK
            assert need.value == K.expected_bytes(*shape, side) and need.value >= 8192 and need.value % 256 == 0
    for bad, word in (((0, 4, 4, 4), b"sizes"), ((4, -1, 4, 4), b"sizes"), ((4, 4, 4, 6), b"side"), ((4, 4, 4, 35), b"side"),
                      ((70000, 70000, 4, 4), b"rows"), ((2 ** 30, 2, 2 ** 30, 4), b"2^30")):
        assert lib.t2fit_n4_workspace_bytes(*bad, C.byref(need)) == _abi.E_INVALID
        assert word in lib.t2fit_last_error(), (bad, lib.t2fit_last_error())
    assert lib.t2fit_n4_workspace_bytes(4, 4, 4, 4, None) == _abi.E_INVALID


def test_every_refusal_comes_before_any_launch(lib):
    """No device here and made-up addresses: a call that got as far as a launch would fail otherwise, or fault."""
    seen = set()
    for name, args, word in K.refusals():
        assert getattr(lib, name)(*args) == _abi.E_INVALID, (name, args)
        msg = lib.t2fit_last_error().decode()
        assert msg.startswith(name + ": ") and word in msg, (name, args, msg)
        seen.add(name)
    assert seen == set(_abi.N4_SYMBOLS) - {"t2fit_n4_workspace_bytes"}


def test_namespace_and_python_refusals():
    import fetal_t2mapping_amd as t2

    assert t2.bias is t2.t2map.bias and "bias" in t2.__all__
    for name in ("n4_correct", "apply_field", "log_image", "minmax", "histogram", "fit_weights", "fit", "field_step", "N4Result"):
        assert hasattr(t2.bias, name)
    with pytest.raises(ValueError, match="bins"):
        _bias.check_options(0.15, (1,), 1e-3, 1, 0.01, 1.0)
    with pytest.raises(ValueError, match="fwhm"):
        _bias.check_options(0.0, (1,), 1e-3, 200, 0.01, 1.0)
    with pytest.raises(ValueError, match="3-D"):
        _bias.log_image(np.ones((3, 3), np.float32))
    with pytest.raises(ValueError, match="shape of the volume"):
        _bias.apply_field(np.ones((2, 2, 2), np.float32), np.ones((2, 2, 3), np.float32))


# ---- the drivers -----------------------------------------------------------------------------------------------------------
def test_recon_and_cli_flags(tmp_path):
    from fetal_t2mapping_amd import cli, recon

    base = ["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo", "--lf"]
    a = recon.parse_arguments(base)
    assert a.n4 is False and a.n4_args is None and a.write_n4 is False  # off by default
    a = recon.parse_arguments(base + ["--n4"])
    assert a.n4_args == {"fwhm_cor": 0.25, "fwhm": 0.5, "echo": None, "scale": 1.0} == recon.N4_DEFAULTS
    a = recon.parse_arguments(base + ["--n4", "--n4_fwhm_cor", "0.2", "--n4_fwhm", "0.4", "--n4_echo", "114", "--n4_scale", "0.25",
                                      "--write_n4"])
    assert a.n4_args == {"fwhm_cor": 0.2, "fwhm": 0.4, "echo": 114, "scale": 0.25} and a.write_n4
    for bad in (["--n4_fwhm", "0.4"], ["--n4_echo", "114"], ["--write_n4"], ["--n4_scale", "2"], ["--n4", "--n4_fwhm", "0"],
                ["--n4", "--n4_fwhm_cor", "-1"], ["--n4", "--n4_scale", "nan"]):
        with pytest.raises(SystemExit):
            recon.parse_arguments(base + bad)
    fit = base + ["--gaussian", "--sim", "x"]
    assert cli.parse_arguments(fit + ["--reconstruct"]).reconstruct_args.get("n4") is None
    assert cli.parse_arguments(fit + ["--reconstruct", "--recon_n4"]).reconstruct_args["n4"] == recon.N4_DEFAULTS
    with pytest.raises(SystemExit):
        cli.parse_arguments(fit + ["--recon_n4"])
    assert recon.n4_echo_index([114.0, 202.0, 255.0, 299.0]) == 2 and recon.n4_echo_index([114.0, 202.0]) == 0
    assert recon.n4_echo_index([114.0, 202.0, 255.0], 202) == 1
    with pytest.raises(ValueError, match="echo times"):
        recon.n4_echo_index([114.0, 202.0], 255)


def test_driver_divides_every_echo_of_an_orientation_by_the_same_field(tmp_path, monkeypatch):
    """The driver over fake_sitk, the device stage replaced by its numpy statement (tests/test_bias_gpu.py runs the
    device's): the echo and the widths it hands on, the mask file it reads, and the echo ratios, unchanged to 1 ulp."""
    import fake_sitk

    fake = fake_sitk.install()
    monkeypatch.setitem(sys.modules, "SimpleITK", fake)
    from fetal_t2mapping_amd import cli, recon

    vol, mask, _, _ = K.recovery_phantom((12, 16, 20))
    te_ms = [114, 255, 299]
    decay = [1.0, 0.55, 0.45]
    bids = str(tmp_path / "projects") + "/"
    rows, batch, run = {}, [], 0
    for te, d in zip(te_ms, decay):
        per = {}
        for o in ("ax", "cor", "sag"):
            run += 1
            per[o] = {"prj": "prj-900", "sub": "sub-001", "ses": "ses-01", "run": f"run-{run:02d}", "EchoTime": te / 1000.0,
                      "CoilString": "HeadNeck", "ImageOrientationPatientSTR": o}
        batch.append((te / 1000.0, per, None))
        rows[te] = per
    stacks = {o: np.stack([(vol * d).astype(np.float32) for d in decay]) for o in ("ax", "cor", "sag")}
    # a mask file for the cor stack of the 255 ms echo only: ax and sag fall back to build_mask (None is handed on)
    def write_mask(row, arr):  # (fake_sitk reads path + '.npy'; the driver looks for the file itself)
        path = cli.get_img_path(bids, row, recon.stack_mask_dirname)
        open(path, "w").close()
        np.save(path + ".npy", arr)

    write_mask(rows[255]["cor"], mask)
    seen = []

    def statement(v, m, *, fwhm, device):
        seen.append((fwhm, None if m is None else int(np.count_nonzero(m)), float(v.max())))
        return _bias.n4_correct(v, mask if m is None else m, fwhm=0.15, max_iter=(4, 2))

    monkeypatch.setattr(recon.t2map.bias, "n4_correct", statement)
    monkeypatch.setattr(recon.t2map.bias, "apply_field", lambda v, f, scale, device: _bias.apply_field(v, f, scale))
    out = recon.n4_batch(fake, bids, batch, stacks, dict(recon.N4_DEFAULTS, scale=0.25))
    top = float(stacks["ax"][1].max())
    assert seen == [(0.5, None, top), (0.25, int(mask.sum()), top), (0.5, None, top)]  # ax, cor, sag on the 255 ms echo
    inside = mask != 0
    for o in ("ax", "cor", "sag"):
        assert out[o].shape == stacks[o].shape and out[o].dtype == np.float32
        assert not np.array_equal(out[o][0], stacks[o][0])
        for a, b in ((0, 1), (0, 2), (1, 2)):
            got = out[o][a][inside].astype(np.float64) / out[o][b][inside]
            want = stacks[o][a][inside].astype(np.float64) / stacks[o][b][inside]
            assert np.max(np.abs(got / want - 1.0)) <= 2.0 ** -23  # two float32 roundings: 1 ulp
    write_mask(rows[255]["sag"], mask[1:])
    with pytest.raises(ValueError, match="has shape"):
        recon.n4_batch(fake, bids, batch, stacks, dict(recon.N4_DEFAULTS))
