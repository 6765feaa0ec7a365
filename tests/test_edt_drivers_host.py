"""The island-reassignment keyword and flag without a GPU: recon.py --tissue_min_island parses and refuses as its
siblings do, _seg.segment_em(min_island=...) applies _edt.reassign_small to the hard labels and leaves everything else as
it was, and the tissue dict of atlas_labels passes the keyword on (tests/test_edt_gpu.py runs the device's)."""
import numpy as np
import pytest

import seg_cases as SC
from fetal_t2mapping_amd import _edt, _seg


def test_recon_flag(tmp_path):
    from fetal_t2mapping_amd import recon

    base = ["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo", "--lf"]
    template, ho, tis = (str(tmp_path / n) for n in ("t.nii.gz", "ho.nii.gz", "tissue.nii.gz"))
    for path in (template, ho, tis):
        open(path, "w").close()
    atlas = ["--atlas_labels", "--atlas_template", template, "--atlas", "ho=" + ho]
    good = atlas + ["--tissue_atlas", tis]
    a = recon.parse_arguments(base + good)
    assert a.tissue_min_island is None and "min_island" not in a.tissue_args  # off by default: the dict is today's
    assert "min_island" not in recon.parse_arguments(base + good + ["--tissue_min_island", "0"]).tissue_args
    a = recon.parse_arguments(base + good + ["--tissue_min_island", "30", "--tissue_iter", "5"])
    assert a.tissue_args["min_island"] == 30 and a.tissue_args["n_iter"] == 5
    for bad in (atlas + ["--tissue_min_island", "30"],  # alone: no effect without --tissue_atlas
                ["--tissue_min_island", "30"], good + ["--tissue_min_island", "-1"], good + ["--tissue_min_island", "2.5"],
                good + ["--tissue_min_island"]):
        with pytest.raises(SystemExit):
            recon.parse_arguments(base + bad)


def test_the_error_names_the_flag(tmp_path, capsys):
    from fetal_t2mapping_amd import recon

    with pytest.raises(SystemExit):
        recon.parse_arguments(["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo", "--lf", "--tissue_min_island", "3"])
    assert "--tissue_min_island has no effect without --tissue_atlas" in capsys.readouterr().err


@pytest.fixture(scope="module")
def phantom_run():
    y, mask, _, atlas = SC.phantom()
    prior = _seg.priors_from_labels(atlas, SC.PHANTOM_CLASSES, 2.0)
    kw = dict(n_iter=3, beta=0.0)  # no Potts term: the labels keep their specks
    return y, mask, prior, kw, _seg.segment_em(y, mask, prior, SC.PHANTOM_CLASSES, **kw)


def test_min_island_zero_is_todays_result(phantom_run):
    y, mask, prior, kw, plain = phantom_run
    assert _seg.SegResult._fields[:5] == ("labels", "model", "s0_trace", "n_iter", "posteriors")
    assert len(_seg.SegResult(1, 2, 3, 4, 5)) == 6 and _seg.SegResult(1, 2, 3, 4, 5).n_reassigned == 0  # five values still build one
    zero = _seg.segment_em(y, mask, prior, SC.PHANTOM_CLASSES, min_island=0, **kw)
    assert zero.n_reassigned == 0 and plain.n_reassigned == 0 and zero.posteriors is None
    assert np.array_equal(zero.labels, plain.labels) and zero.labels.dtype == plain.labels.dtype
    assert np.array_equal(zero.s0_trace, plain.s0_trace) and zero.n_iter == plain.n_iter
    assert np.array_equal(zero.model.mean, plain.model.mean)


def test_min_island_applies_the_statement(phantom_run):
    y, mask, prior, kw, plain = phantom_run
    want, changed = _edt.reassign_small(plain.labels, 20)
    assert changed > 0  # the phantom's noise leaves islands: the keyword has something to do
    res = _seg.segment_em(y, mask, prior, SC.PHANTOM_CLASSES, min_island=20, return_posteriors=True, **kw)
    assert res.n_reassigned == changed and np.array_equal(res.labels, want) and res.labels.dtype == np.int32
    assert np.array_equal(res.s0_trace, plain.s0_trace) and res.posteriors is not None
    assert np.array_equal(res.labels == 0, plain.labels == 0)  # the mask's outside stays 0
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError, match="min_island"):
            _seg.segment_em(y, mask, prior, SC.PHANTOM_CLASSES, min_island=bad, **kw)


def test_the_tissue_dict_passes_it_on():
    assert "min_island" in _seg.TISSUE_KEYS
    shape = (4, 5, 6)
    labels = np.ones(shape, np.int32)
    *_, em = _seg.tissue_arguments({"labels": labels, "classes": [1, 2], "channels": np.zeros(shape, np.float32), "min_island": 9},
                                   shape, shape)
    assert em == {"min_island": 9}
    res = _seg.SegResult("l", "m", "t", 3, None, 7)
    out = _seg.tissue_result("p", "q", res)
    assert out["n_reassigned"] == 7 and out["labels"] == "l" and out["n_iter"] == 3
