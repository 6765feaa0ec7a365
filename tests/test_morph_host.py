"""The numpy statement of the mask-building stage (fetal_t2mapping_amd/_morph.py) against scipy.ndimage, exactly: run-list
dilation and erosion over footprints, borders and iterations, the two closings, hole filling in 3-D and per plane, the
run-list round trip, the ball's voxel counts and the SynthSeg -> FeTA table.  No device is needed."""
import numpy as np
import pytest
from scipy import ndimage as ndi

from fetal_t2mapping_amd import _morph as M


def _two_runs():
    fp = np.zeros((3, 5, 9), bool)  # not convex, not symmetric: two runs in one row, a lone voxel in a corner
    fp[1, 2, 0:3] = True
    fp[1, 2, 6:9] = True
    fp[0, 4, 8] = True
    fp[2, 1, 2:5] = True
    return fp


FOOTPRINTS = {"ball1": M.ball(1), "ball3": M.ball(3), "ball234": M.ball((2, 3, 4)), "box": M.box((1, 2, 3)), "cross1": M.cross(1),
              "cross2": M.cross(2), "cross3": M.cross(3), "two_runs": _two_runs(), "flat5x5": np.ones((1, 5, 5), bool)}


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
