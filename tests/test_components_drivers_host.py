"""The connected-component flags of recon.py without a GPU: --mask_keep_largest / --mask_min_size and --phantom_find_seeds
with its sub-flags parse and refuse as documented; the seed finder runs over tests/fake_sitk.py with the device calls
replaced by their numpy statements (tests/test_components_gpu.py runs the device's) and its JSON goes through load_seeds;
the masks the registrations and the N4 step get."""
import inspect
import json
import os
import sys
import types

import numpy as np
import pandas as pd
import pytest

import components_cases as K
from fetal_t2mapping_amd import _components, _morph, _register


def test_flags(tmp_path):
    from fetal_t2mapping_amd import recon

    base = ["--path", str(tmp_path), "--csv", "x.csv", "--in_vitro", "--lf"]
    a = recon.parse_arguments(base)
    assert a.mask_clean is None and a.find_seeds is None and a.mask_keep_largest == 0 and a.mask_min_size == 0  # off by default
    assert recon.parse_arguments(base + ["--register", "--mask_keep_largest", "1"]).mask_clean == {"keep_largest": 1, "min_size": 0}
    assert recon.parse_arguments(base + ["--n4", "--mask_min_size", "50"]).mask_clean == {"keep_largest": 0, "min_size": 50}
    a = recon.parse_arguments(base + ["--register_echoes", "--mask_min_size", "9", "--mask_keep_largest", "2"])
    assert a.mask_clean == {"keep_largest": 2, "min_size": 9}
    out = str(tmp_path / "seeds.json")
    find = ["--phantom_masks", "--phantom_find_seeds", out]
    a = recon.parse_arguments(base + find + ["--phantom_vial_window", "300,1500"])
    assert a.find_seeds == {"window": (300.0, 1500.0), "erode": 2, "size": (1, 0)} and a.phantom_find_seeds == out
    a = recon.parse_arguments(base + find + ["--phantom_vial_window", "300,inf", "--phantom_vial_erode", "0", "--phantom_vial_size", "20,400"])
    assert a.find_seeds == {"window": (300.0, float("inf")), "erode": 0, "size": (20, 400)}
    for bad in (["--mask_keep_largest", "1"], ["--mask_min_size", "5"], ["--register", "--mask_keep_largest", "-1"],
                ["--n4", "--mask_min_size", "-3"], ["--phantom_find_seeds", out, "--phantom_vial_window", "1,2"], find,
                ["--phantom_masks", "--phantom_vial_window", "1,2"], ["--phantom_masks", "--phantom_vial_erode", "2"],
                ["--phantom_masks", "--phantom_vial_size", "1,0"], find + ["--phantom_vial_window", "5"],
                find + ["--phantom_vial_window", "a,b"], find + ["--phantom_vial_window", "9,2"], find + ["--phantom_vial_window", "nan,2"],
                find + ["--phantom_vial_window", "1,2", "--phantom_vial_erode", "33"],
                find + ["--phantom_vial_window", "1,2", "--phantom_vial_erode", "-1"],
                find + ["--phantom_vial_window", "1,2", "--phantom_vial_size", "0,5"],
                find + ["--phantom_vial_window", "1,2", "--phantom_vial_size", "9,5"],
                find + ["--phantom_vial_window", "1,2", "--phantom_vial_size", "9"]):
        with pytest.raises(SystemExit):
            recon.parse_arguments(base + bad)
    # the rules of --phantom_seeds are as they were
    with pytest.raises(SystemExit):
        recon.parse_arguments(base + ["--phantom_seeds", out])
    with pytest.raises(SystemExit):
        recon.parse_arguments(base + ["--phantom_masks", "--phantom_seeds", str(tmp_path / "missing.json")])
    for fn in (recon.process_recon, recon.merge_echoes, recon.register_stacks, recon.correct_stacks, recon.n4_batch):
        assert inspect.signature(fn).parameters["mask_clean"].default is None
    assert recon.cleaned_masks(None, None, None) == {} and recon.cleaned_masks(None, None, {}) == {}


def _host_stage(monkeypatch, recon):
    """recon.t2map with the device calls of the seed finder and of build_mask replaced by their numpy statements."""
    fake = types.SimpleNamespace(
        binary_threshold=lambda vol, lo, hi, device=0: ((vol >= lo) & (vol <= hi)).astype(np.uint8),
        binary_erode=lambda m, element, out=None, device=0: _morph.erode(m, element).astype(np.uint8),
        build_mask=lambda vol, device=0, **kw: _register.build_mask(np.asarray(vol), **kw),
        components=types.SimpleNamespace(seeds=lambda m, c, lo, hi, device=0: _components.seeds(m, c, lo, hi)))
    monkeypatch.setattr(recon, "t2map", fake)
    return fake


def _subjects(tmp_path, subs):
    from fetal_t2mapping_amd import cli

    bids = str(tmp_path / "projects") + "/"
    vol, centres = K.phantom()
    rows = []
    for sub in subs:
        for i, te in enumerate((114, 202)):
            acq = {"prj": "prj-901", "sub": sub, "ses": "ses-01", "run": f"run-{i + 1:02d}", "EchoTime": te / 1000.0,
                   "CoilString": "HeadNeck", "ImageOrientationPatientSTR": "ax"}
            rows.append(acq)
            np.save(cli.get_img_path(bids, acq, cli.recon_dirname).replace(" ", "") + ".npy", (vol * (1.0 if i == 0 else 0.1)).astype(np.float32))
    return bids, pd.DataFrame(rows), centres


def test_find_seeds_writes_what_load_seeds_reads(tmp_path, monkeypatch):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import fake_sitk

    monkeypatch.setitem(sys.modules, "SimpleITK", fake_sitk.install())
    from fetal_t2mapping_amd import recon

    _host_stage(monkeypatch, recon)
    bids, md, centres = _subjects(tmp_path, ["sub-001"])
    out = str(tmp_path / "seeds.json")
    assert recon.process_find_seeds(md, bids, out, window=(500.0, 2000.0), erode=2, size=(10, 0)) == [out]
    seeds = recon.load_seeds(out)
    assert sorted(seeds) == sorted(centres) and seeds == json.load(open(out))
    vol, _ = K.phantom()
    assert seeds == _components.seeds(_morph.erode(vol >= 500, _morph.ball(2)), 1, 10, 0)  # the first echo, in label order
    # without the erosion the specks are components too; the size limits drop them
    recon.process_find_seeds(md, bids, out, window=(500.0, 2000.0), erode=0, size=(1, 0))
    assert len(recon.load_seeds(out)) == 16
    recon.process_find_seeds(md, bids, out, window=(500.0, 2000.0), erode=0, size=(2, 0))
    assert sorted(recon.load_seeds(out)) == sorted(centres)
    with pytest.raises(ValueError, match="0 components"):
        recon.process_find_seeds(md, bids, out, window=(5000.0, 6000.0), erode=2, size=(1, 0))
    # several subjects: a file each
    bids, md, _ = _subjects(tmp_path, ["sub-001", "sub-002"])
    written = recon.process_find_seeds(md, bids, out, window=(500.0, 2000.0), erode=2, size=(10, 0))
    assert written == [str(tmp_path / "seeds_sub-001_ses-01.json"), str(tmp_path / "seeds_sub-002_ses-01.json")]
    assert all(sorted(recon.load_seeds(p)) == sorted(centres) for p in written)


def test_statement_seeds_round_trip(tmp_path):
    from fetal_t2mapping_amd import cli

    vol, centres = K.phantom()
    seeds = _components.seeds(_morph.erode(vol > 0, _morph.ball(2)), 1, 10, 0)
    path = tmp_path / "s.json"
    path.write_text(json.dumps(seeds))
    assert cli.load_seeds(str(path)) == seeds and sorted(seeds) == sorted(centres)


def test_the_masks_the_registration_and_the_n4_get(monkeypatch):
    from fetal_t2mapping_amd import recon

    fake = _host_stage(monkeypatch, recon)
    vol, _ = K.phantom()
    got = recon.cleaned_masks(vol, vol[::-1].copy(), {"keep_largest": 1, "min_size": 0})
    assert sorted(got) == ["fixed_mask", "moving_mask"]
    assert np.array_equal(got["fixed_mask"], _register.build_mask(vol, keep_largest=1)) and got["fixed_mask"].sum() < _register.build_mask(vol).sum()
    assert np.array_equal(got["moving_mask"], _register.build_mask(vol[::-1], keep_largest=1))
    seen = []

    def n4_correct(v, mask, fwhm, device=0):
        seen.append(mask)
        return types.SimpleNamespace(log_field=np.zeros(v.shape, np.float32), iterations=[0])

    fake.bias = types.SimpleNamespace(n4_correct=n4_correct, apply_field=lambda v, f, scale, device=0: v)
    stacks = {o: vol[None] for o in ("ax", "cor", "sag")}
    given = np.ones(vol.shape, np.uint8)
    recon.correct_stacks(stacks, {"ax": given}, [114.0])
    assert seen[0] is given and seen[1] is None and seen[2] is None  # without the flags: the N4 step builds its own
    del seen[:]
    recon.correct_stacks(stacks, {"ax": given}, [114.0], mask_clean={"keep_largest": 0, "min_size": 20})
    assert seen[0] is given and np.array_equal(seen[1], _register.build_mask(vol, min_size=20)) and np.array_equal(seen[1], seen[2])
