"""The numpy statement of the mask-building stage (fetal_t2mapping_amd/_morph.py) against scipy.ndimage, exactly: run-list
dilation and erosion over footprints, borders and iterations, the two closings, hole filling in 3-D and per plane, the
run-list round trip, the ball's voxel counts and the SynthSeg -> FeTA table; the same on the balanced inputs of
tests/morph_cases.py, where about half of the voxels change, with mutations of the statement that only those inputs catch;
every run offset against a response pasted from the definition; the model of the hole filling's sweeps.  No device is
needed."""
import morph_cases as K
import numpy as np
import pytest
from scipy import ndimage as ndi

from fetal_t2mapping_amd import _morph as M

FOOTPRINTS = K.FOOTPRINTS


def _volume(shape=(20, 30, 37), seed=3):
    rng = np.random.default_rng(seed)
    a = rng.random(shape) < 0.02
    for ax in range(3):  # ones on every face
        for edge in (0, -1):
            idx = [slice(None)] * 3
            idx[ax] = edge
            a[tuple(idx)] |= rng.random(a[tuple(idx)].shape) < 0.05
            assert a[tuple(idx)].any()
    return a


def _shells(shape, seed=5, n=40):
    """Dilated random points minus their erosion: closed shells, some cut by the border."""
    rng = np.random.default_rng(seed)
    pts = np.zeros(shape, bool)
    pts[tuple(rng.integers(0, s, n) for s in shape)] = True
    blob = ndi.binary_dilation(pts, ndi.generate_binary_structure(3, 1), iterations=4)
    return blob & ~ndi.binary_erosion(blob, ndi.generate_binary_structure(3, 1), border_value=1)


@pytest.mark.parametrize("name", sorted(FOOTPRINTS))
@pytest.mark.parametrize("border", [0, 1])
@pytest.mark.parametrize("iterations", [1, 3])
def test_dilate_and_erode_equal_scipy(name, border, iterations):
    a, fp = _volume(), FOOTPRINTS[name]
    assert np.array_equal(M.dilate(a, fp, iterations, border), ndi.binary_dilation(a, fp, iterations=iterations, border_value=border))
    assert np.array_equal(M.erode(a, fp, iterations, border), ndi.binary_erosion(a, fp, iterations=iterations, border_value=border))


def test_scipy_form_close_and_open_equal_scipy():
    a, fp = _volume(), M.ball(2)
    assert np.array_equal(M.close(a, fp), ndi.binary_closing(a, fp))
    assert np.array_equal(M.open(a, fp, 1, 1), ndi.binary_opening(a, fp, border_value=1))
    assert np.array_equal(M.close(a, fp, 2), ndi.binary_closing(a, fp, iterations=2))


def test_unbounded_close_is_pad_dilate_erode_crop_and_not_the_scipy_form():
    a, fp = _volume(), M.ball(3)
    p = np.pad(a, 3)
    want = ndi.binary_erosion(ndi.binary_dilation(p, fp), fp)[3:-3, 3:-3, 3:-3]
    got = M.close(a, fp, unbounded=True)
    assert np.array_equal(got, want)
    assert not np.array_equal(got, M.close(a, fp))  # the erosion of the scipy form eats what touches the border
    assert not np.array_equal(got, ndi.binary_erosion(ndi.binary_dilation(a, fp), fp, border_value=1))  # nor is it this


def test_fill_holes_equals_scipy_in_3d_and_per_plane():
    a = _shells((24, 40, 45))
    want = ndi.binary_fill_holes(a)
    assert int(want.sum() - a.sum()) > 0
    assert np.array_equal(M.fill_holes(a), want)
    for axis in (0, 1, 2):
        want = np.stack([ndi.binary_fill_holes(np.take(a, i, axis)) for i in range(a.shape[axis])], axis)
        assert int(want.sum() - a.sum()) > 0
        assert np.array_equal(M.fill_holes(a, axis), want), axis


@pytest.mark.parametrize("name", sorted(FOOTPRINTS))
def test_footprint_runs_round_trip(name):
    fp = FOOTPRINTS[name]
    runs, size = M.footprint_runs(fp)
    assert size == fp.shape and runs.dtype == np.int32
    assert int((runs[:, 3] - runs[:, 2] + 1).sum()) == int(fp.sum())
    assert np.array_equal(M.runs_footprint(runs, size), fp)
    assert np.array_equal(M.runs_footprint(M.reflect_runs(runs), size), fp[::-1, ::-1, ::-1])
    with pytest.raises(ValueError, match="odd"):
        M.footprint_runs(np.ones((3, 4, 3), bool))


def test_ball_counts():
    b6, b15 = M.ball(6), M.ball(15)
    assert int(b6.sum()) == 1189 and len(M.footprint_runs(b6)[0]) == 137
    assert int(b15.sum()) == 15515
    runs = M.footprint_runs(b15)[0]
    assert len(runs) == 749 and len(set((runs[:, 3] - runs[:, 2]).tolist())) == 14
    assert np.array_equal(M.cross(1), ndi.generate_binary_structure(3, 1))
    assert np.array_equal(M.cross(2), ndi.generate_binary_structure(3, 2))
    assert np.array_equal(M.cross(3), ndi.generate_binary_structure(3, 3))


def test_seed_labels_take_the_maximum_and_clip():
    out = M.seed_labels((12, 14, 16), [(3, 4, 5), (5, 4, 5), (0, 0, 0)], [1, 2, 3], M.ball(2))
    assert out.dtype == np.uint8 and out[5, 4, 1] == 1 and out[5, 4, 2] == 1 and out[5, 4, 3] == 2 and out[5, 4, 7] == 2
    assert out[0, 0, 0] == 3 and int((out == 3).sum()) < int(M.ball(2).sum())
    assert int((out == 2).sum()) == int(M.ball(2).sum())  # the larger label wins the whole overlap


def test_feta_table():
    lut = M.feta_lut()
    want = {24: 1, 3: 2, 42: 2, 2: 3, 41: 3, 4: 4, 5: 4, 14: 4, 15: 4, 43: 4, 44: 4, 7: 5, 8: 5, 46: 5, 47: 5, 10: 6, 11: 6,
            12: 6, 13: 6, 17: 6, 18: 6, 26: 6, 28: 6, 49: 6, 50: 6, 51: 6, 52: 6, 53: 6, 54: 6, 58: 6, 60: 6, 16: 7}
    for i in range(lut.size):
        assert lut[i] == want.get(i, 0), i
    ids = np.array([[-1, 0, 24, 16], [60, 61, 1000, 42]])
    assert np.array_equal(M.relabel(ids, lut), [[0, 0, 1, 7], [6, 0, 0, 2]])


# ---- balanced inputs: about half of the voxels change (morph_cases.py) -----------------------------------------------------
HOST_SHAPES = [(24, 40, 48), (17, 33, 70), (20, 30, 37)]
HOST_ITERATIONS = (1, 3)


def _balanced_failures(shape):
    """The cases of a shape on which the statement differs from scipy."""
    bad = []
    for name, n, border, op in K.cases(shape, FOOTPRINTS, HOST_ITERATIONS):
        got = getattr(M, op)(K.balanced(shape, name, n, op), FOOTPRINTS[name], n, border)
        if not np.array_equal(got, K.expected(shape, name, n, border, op)):
            bad.append((name, n, border, op))
    return bad


def _sparse_failures():
    """The comparisons of test_dilate_and_erode_equal_scipy, on its 2 % volume, that fail: (op, footprint, border, n)."""
    a, bad = _volume(), []
    for name, fp in sorted(FOOTPRINTS.items()):
        for border in (0, 1):
            for n in (1, 3):
                for op, ref in (("dilate", ndi.binary_dilation), ("erode", ndi.binary_erosion)):
                    if not np.array_equal(getattr(M, op)(a, fp, n, border), ref(a, fp, iterations=n, border_value=border)):
                        bad.append((op, name, border, n))
    return bad


@pytest.mark.parametrize("shape", HOST_SHAPES)
def test_balanced_dilate_and_erode_equal_scipy(shape):
    assert _balanced_failures(shape) == []


def test_balance_and_thin_share_of_every_shape():
    for shape in K.GENERAL_SHAPES:
        share = K.minority_share(shape, tuple(K.ELEMENTS), (1, 2))  # asserts MIN_SHARE case by case, raises on the thin share
        print(f"{shape}: smallest minority share {100 * share:.1f} %")
        assert share >= K.MIN_SHARE
    for shape in HOST_SHAPES:
        assert K.minority_share(shape, tuple(FOOTPRINTS), HOST_ITERATIONS) >= K.MIN_SHARE
    for shape in K.FLAT_SHAPES:  # not general: the helper says so
        with pytest.raises(ValueError, match="thin"):
            K.cases(shape, K.ELEMENTS, (1, 2))
    assert K.is_thin((24, 40, 48), "ball3", 2) and not K.is_thin((26, 40, 48), "ball3", 2)  # 13 voxels against 12 and 13


def test_the_old_sparse_erosions_were_all_empty():
    a = _volume()
    for fp in FOOTPRINTS.values():
        for border in (0, 1):
            for n in (1, 3):
                assert not ndi.binary_erosion(a, fp, iterations=n, border_value=border).any()


@pytest.mark.parametrize("name", sorted(FOOTPRINTS))
def test_balanced_close_and_open_equal_scipy(name):
    shape, fp = (24, 40, 48), FOOTPRINTS[name]
    for n in HOST_ITERATIONS:
        for op, source in (("close", "dilate"), ("open", "erode")):
            a = K.balanced(shape, name, n, source)
            for border in (0, 1):
                want = K.scipy_close_open(op, a, fp, n, border, False)
                assert np.array_equal(getattr(M, op)(a, fp, n, border), want), (op, n, border)
                if not K.is_thin(shape, name, n):
                    assert want.any() and not want.all() and not np.array_equal(want, a), (op, n, border)


@pytest.mark.parametrize("name,n", [("two_runs", 3), ("ball234", 1), ("flat5x5", 2)])
def test_balanced_unbounded_close_and_open(name, n):
    shape, fp = (24, 40, 48), FOOTPRINTS[name]  # two_runs three times: a reach of 12 voxels
    for op, source in (("close", "dilate"), ("open", "erode")):
        a = K.balanced(shape, name, n, source)
        want = K.scipy_close_open(op, a, fp, n, 0, True)
        assert np.array_equal(getattr(M, op)(a, fp, n, unbounded=True), want), op
        assert want.any() and not want.all()
        # the closings differ: the scipy form's erosion eats what touches the border.  With zeros outside the openings agree
        assert np.array_equal(want, K.scipy_close_open(op, a, fp, n, 0, False)) == (op == "open")


@pytest.mark.parametrize("name", sorted(K.MUTATIONS))
def test_mutated_statement_fails_on_the_balanced_inputs(name):
    """Each mutation is caught by an erosion of the balanced inputs.  The erosions of the old 2 % volume, all of them empty,
    pass every mutant, and so do its dilations unless the mutation is in the dilation itself.  (Of the older tests only the
    closing of that volume sees the wrong border of the second mutant, and the two_runs dilation the third.)"""
    with K.mutated(name):
        balanced = _balanced_failures((20, 30, 37))
        sparse = _sparse_failures()
    assert balanced and any(op == "erode" for _, _, _, op in balanced), name
    assert [f for f in sparse if f[0] == "erode"] == []
    if name == "dilate_once_x_swapped":  # the dilation by the one asymmetric footprint shows this one on any input
        assert sparse and all(f[:2] == ("dilate", "two_runs") for f in sparse)
    else:
        assert sparse == []
    assert _balanced_failures((20, 30, 37)) == [] and _sparse_failures() == []  # the statement is itself again


# ---- every run offset ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.IMPULSES))
def test_every_run_offset_equals_the_pasted_response(name):
    a = K.impulse_volume(name)
    runs, size = M.footprint_runs(K.all_runs_footprint())
    assert len(runs) == 2145 and [tuple(r) for r in runs.tolist()] == list(K.all_runs())
    assert np.array_equal(M.dilate(a, (runs, size)), K.impulse_expected(name, "dilate"))
    assert np.array_equal(M.erode(~a, (runs, size), 1, 1), K.impulse_expected(name, "dual"))
    if name == "two_bit_tail":
        want = K.impulse_expected(name, "erode0")
        assert want.any() and np.array_equal(M.erode(~a, (runs, size), 1, 0), want)


# ---- the model of the hole filling's sweeps ----------------------------------------------------------------------------------
def test_sweep_model_fills_as_scipy_and_counts_a_sweep_per_tile():
    for name, (a, axis, by_hand) in K.CHANNELS.items():
        filled, sweeps = K.sweep_model(a, axis)
        want = ndi.binary_fill_holes(a) if axis is None else K.fill_per_plane(a, axis)
        assert np.array_equal(filled, want) and np.array_equal(M.fill_holes(a, axis), want), name
        assert sweeps == by_hand, name
    assert sorted(K.CHANNELS[f"y{n}"][2] % 4 for n in (32, 40, 48, 56)) == [0, 1, 2, 3]  # every place of a batch of four
    for name, a in K.DEGENERATE.items():
        for axis in (None, 0, 1, 2):
            want = ndi.binary_fill_holes(a) if axis is None else K.fill_per_plane(a, axis)
            assert np.array_equal(K.sweep_model(a, axis)[0], want), (name, axis)
            assert np.array_equal(M.fill_holes(a, axis), want), (name, axis)
    for end in ("high", "low"):
        a = K.DEGENERATE[f"word_run_from_{end}_end"]
        assert not ndi.binary_fill_holes(a)[1, 1, 64:192].any()  # the run is reached, all of it
    assert ndi.binary_fill_holes(K.DEGENERATE["enclosed_zero_x64"])[1, 1, 64]
