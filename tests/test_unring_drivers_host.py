"""--unring in recon.py and --recon_unring in cli.py without a GPU: the flags and their refusals, the driver over
tests/fake_sitk.py with the device stage replaced by its numpy statement (tests/test_unring_gpu.py runs the device's): the
order of the stages, the plane that is filtered, the pixel type, the ``unring`` directory and its file names, and that
nothing changes without the flag."""
import inspect
import os
import sys

import numpy as np
import pytest

import unring_cases as K
from fetal_t2mapping_amd import _unring


def test_recon_and_cli_flags(tmp_path):
    from fetal_t2mapping_amd import cli, recon

    base = ["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo", "--lf"]
    a = recon.parse_arguments(base)
    assert a.unring is False and a.unring_args is None and a.write_unring is False  # off by default
    assert recon.parse_arguments(base + ["--unring"]).unring_args == {"K": 20, "min_w": 1, "max_w": 3} == recon.UNRING_DEFAULTS
    a = recon.parse_arguments(base + ["--unring", "--unring_shifts", "7", "--unring_window", "2,5", "--write_unring"])
    assert a.unring_args == {"K": 7, "min_w": 2, "max_w": 5} and a.write_unring
    assert recon.parse_arguments(base + ["--unring", "--n4"]).n4_args == recon.N4_DEFAULTS  # the two go together
    for bad in (["--unring_shifts", "7"], ["--unring_window", "1,3"], ["--write_unring"], ["--unring_shifts=7"],
                ["--unring", "--unring_shifts", "0"], ["--unring", "--unring_shifts", "33"], ["--unring", "--unring_window", "0,3"],
                ["--unring", "--unring_window", "1,9"], ["--unring", "--unring_window", "3,2"], ["--unring", "--unring_window", "3"],
                ["--unring", "--unring_window", "a,b"]):
        with pytest.raises(SystemExit):
            recon.parse_arguments(base + bad)
    fit = base + ["--gaussian", "--sim", "x"]
    assert "unring" not in cli.parse_arguments(fit + ["--reconstruct"]).reconstruct_args
    assert cli.parse_arguments(fit + ["--reconstruct", "--recon_unring"]).reconstruct_args["unring"] == recon.UNRING_DEFAULTS
    a = cli.parse_arguments(fit + ["--reconstruct", "--recon_unring", "--recon_unring_shifts", "5", "--recon_unring_window", "1,2"])
    assert a.reconstruct_args["unring"] == {"K": 5, "min_w": 1, "max_w": 2}
    for bad in (["--recon_unring"], ["--reconstruct", "--recon_unring_shifts", "5"], ["--reconstruct", "--recon_unring_window", "1,2"],
                ["--reconstruct", "--recon_unring", "--recon_unring_shifts", "40"]):
        with pytest.raises(SystemExit):
            cli.parse_arguments(fit + bad)
    # without the flag the drivers never reach the stage
    for fn in (recon.process_recon, recon.reconstruct_subject):
        assert inspect.signature(fn).parameters["unring"].default is None
    assert inspect.signature(recon.process_recon).parameters["write_unring"].default is False
    assert recon.unring_dirname == "unring"


def _batch():
    rows, batch, run = {}, [], 0
    for te in (114, 255):
        per = {}
        for o in ("ax", "cor", "sag"):
            run += 1
            per[o] = {"prj": "prj-900", "sub": "sub-001", "ses": "ses-01", "run": f"run-{run:02d}", "EchoTime": te / 1000.0,
                      "CoilString": "HeadNeck", "ImageOrientationPatientSTR": o}
        batch.append((te / 1000.0, per, None))
        rows[te] = per
    return rows, batch


def test_driver_unrings_the_acquired_plane_of_every_stack_and_writes_them(tmp_path, monkeypatch):
    import fake_sitk

    fake = fake_sitk.install()
    monkeypatch.setitem(sys.modules, "SimpleITK", fake)
    from fetal_t2mapping_amd import cli, recon

    rows, batch = _batch()
    shapes = {"ax": (3, 12, 16), "cor": (4, 10, 12), "sag": (3, 16, 9)}
    stacks = {o: np.round(K.random_slices(2 * s[0], s[1], s[2], 5 + i)).reshape((2,) + s) for i, (o, s) in enumerate(shapes.items())}
    seen = []

    def statement(block, slice_axis=0, K=20, min_w=1, max_w=3, out=None, info=None, device=0):
        seen.append((block.shape, block.dtype, slice_axis, K, min_w, max_w))
        ny, nx = block.shape[-2:]
        res, skipped = _unring.unring(block.reshape(-1, ny, nx), _unring.Tables(ny, nx, K), min_w, max_w)
        info["skipped"] = skipped
        return res.reshape(block.shape)

    monkeypatch.setattr(recon.t2map.unring, "unring_volume", statement)
    out = recon.unring_batch(stacks, {"K": 3, "min_w": 1, "max_w": 2})
    # every orientation once, the whole (n, Z, Y, X) block, slices along Z: the plane is (Y, X)
    assert seen == [((2,) + shapes[o], np.dtype(np.float32), 0, 3, 1, 2) for o in ("ax", "cor", "sag")]
    for o, s in shapes.items():
        assert out[o].shape == stacks[o].shape and out[o].dtype == np.float32
        want = _unring.unring(stacks[o].reshape(-1, s[1], s[2]).astype(np.float32), _unring.Tables(s[1], s[2], 3), 1, 2)[0]
        assert out[o].tobytes() == want.tobytes()
        assert not np.array_equal(out[o], np.round(out[o]))  # the stacks stop being integers
    geoms = {o: fake.Image(np.zeros(1), (1.0, 1.0, 4.5), (1.0, 2.0, 3.0)) for o in shapes}
    bids = str(tmp_path / "projects") + "/"
    recon.write_stacks(fake, bids, batch, out, geoms, recon.unring_dirname)
    assert len(fake.written) == 6
    for i, te in enumerate((114, 255)):
        for o in shapes:
            path = cli.get_img_path(bids, rows[te][o], "unring")
            assert os.sep + os.path.join("derivatives", "unring", "sub-001", "ses-01", "anat") + os.sep in path
            raw = os.path.basename(cli.get_img_path(bids, rows[te][o], "anat"))
            assert os.path.basename(path) == raw.replace("_T2w.nii.gz", "_T2w_unring.nii.gz") != raw  # the raw stack's name plus the stage
            img = fake.written[path]
            assert img.arr.tobytes() == out[o][i].tobytes() and img.GetSpacing() == (1.0, 1.0, 4.5) and img.GetOrigin() == (1.0, 2.0, 3.0)


def test_unring_runs_before_n4_and_the_pixel_type_is_treated_as_under_n4(tmp_path, monkeypatch):
    """process_recon with the stages replaced by recorders: the order unring, n4, merge; cast as --n4 leaves it; and without
    the flag neither the stage nor the directory is touched."""
    import fake_sitk

    fake = fake_sitk.install()
    monkeypatch.setitem(sys.modules, "SimpleITK", fake)
    from fetal_t2mapping_amd import recon

    rows, batch = _batch()
    stacks = {o: np.full((2, 3, 12, 16), 5.0, np.float32) for o in ("ax", "cor", "sag")}
    calls = []

    class Stop(Exception):
        pass

    monkeypatch.setattr(recon, "echo_groups", lambda md: [("prj-900", "sub-001", "ses-01", None)])
    monkeypatch.setattr(recon, "read_echoes", lambda *a: None)
    monkeypatch.setattr(recon, "batches_of", lambda ready: [batch])
    monkeypatch.setattr(recon, "batch_inputs", lambda sitk, b, cast: (stacks, {o: None for o in stacks}, True))
    monkeypatch.setattr(recon, "unring_batch", lambda s, u, device=0: calls.append(("unring", dict(u))) or {o: v + 1 for o, v in s.items()})
    monkeypatch.setattr(recon, "n4_batch", lambda sitk, bp, b, s, n4, device=0: calls.append(("n4", float(s["ax"][0, 0, 0, 0]))) or s)
    monkeypatch.setattr(recon, "write_stacks", lambda sitk, bp, b, s, g, d: calls.append(("write", d, float(s["ax"][0, 0, 0, 0]))))

    def merge(s, geoms, rows_, **kw):
        calls.append(("merge", float(s["ax"][0, 0, 0, 0]), kw["integer_cast"]))
        raise Stop

    monkeypatch.setattr(recon, "merge_echoes", merge)
    with pytest.raises(Stop):
        recon.process_recon(None, "x/", unring={"K": 3, "min_w": 1, "max_w": 2}, write_unring=True, n4=dict(recon.N4_DEFAULTS))
    assert calls == [("unring", {"K": 3, "min_w": 1, "max_w": 2}), ("write", "unring", 6.0), ("n4", 6.0), ("merge", 6.0, False)]
    calls.clear()
    with pytest.raises(Stop):
        recon.process_recon(None, "x/", unring={"K": 3, "min_w": 1, "max_w": 2}, integer_cast=True)
    assert calls == [("unring", {"K": 3, "min_w": 1, "max_w": 2}), ("merge", 6.0, True)]
    calls.clear()
    with pytest.raises(Stop):
        recon.process_recon(None, "x/")
    assert calls == [("merge", 5.0, True)]  # no flag: the stacks and the pixel type as they were
