"""bench.py --dump-outputs: which voxels a dump holds (host logic) and, on the GPU box, that the dumped maps are the fit
of the bench's seeded volume as a caller of the device entry point receives it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

import bench


def test_dump_index_is_fixed_sorted_and_within_budget():
    assert bench.dump_index(bench.DUMP_MAX_VOXELS) is None  # maps that fit are written whole
    n = 256 ** 3
    idx = bench.dump_index(n)
    assert idx.shape == (bench.DUMP_MAX_VOXELS,) and idx[0] >= 0 and idx[-1] < n
    assert np.all(np.diff(idx) > 0)  # sorted, no voxel twice
    assert np.array_equal(idx, bench.dump_index(n))  # the same set from call to call
    # frozen stream of numpy's RandomState: the sample is the same on every numpy
    assert idx[:4].tolist() == [0, 1, 5, 9] and int(idx.sum() % 1000003) == 764225
    # spread over the whole volume, not a corner of it
    assert np.all(np.histogram(idx, bins=64, range=(0, n))[0] > 0.9 * bench.DUMP_MAX_VOXELS / 64)
    # four float32 maps and their .npy headers stay under 64 MB
    assert len(bench.DUMP_NAMES) * (4 * bench.DUMP_MAX_VOXELS + 128) <= 64_000_000


def test_dump_outputs_writes_the_sampled_rows_as_float32(tmp_path, monkeypatch):
    import torch

    monkeypatch.setattr(bench, "DUMP_MAX_VOXELS", 1000)
    maps4 = torch.arange(4 * 5000, dtype=torch.float32).reshape(4, 5000)
    maps4[3, 7] = float("nan")
    info = bench.dump_outputs(str(tmp_path / "whole"), maps4[:, :1000])
    assert info["voxels_written"] == info["voxels"] == 1000 and info["sample"] is None
    info = bench.dump_outputs(str(tmp_path / "sampled"), maps4)
    assert info["voxels_written"] == 1000 and info["voxels"] == 5000 and info["arrays"] == list(bench.DUMP_NAMES)
    idx = bench.dump_index(5000)
    assert sorted(os.listdir(tmp_path / "sampled")) == sorted(n + ".npy" for n in bench.DUMP_NAMES)
    for j, name in enumerate(bench.DUMP_NAMES):
        whole, part = np.load(tmp_path / "whole" / (name + ".npy")), np.load(tmp_path / "sampled" / (name + ".npy"))
        assert whole.dtype == part.dtype == np.float32 and whole.shape == part.shape == (1000,)
        assert np.array_equal(whole, maps4[j, :1000].numpy(), equal_nan=True)
        assert np.array_equal(part, maps4[j].numpy()[idx], equal_nan=True)


def test_full_is_an_option_that_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and (a.gpus, a.steps, a.warmup) == (1, 4, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    a = bench.parse()
    assert a.full is True and a.cpu_seconds > 0 and not a.no_also  # --full alone runs every secondary measurement
    assert "cpu_baseline" in bench.FULL_ONLY_KEYS and "also" in bench.FULL_ONLY_KEYS and "value" not in bench.FULL_ONLY_KEYS


@pytest.mark.gpu
def test_bench_dump_is_the_fit_of_the_seeded_volume(tmp_path):
    """A plain bench.py run in a process of its own (3 timed steps, a volume larger than a dump holds), then the same seeded volume
    through fit_volume here: the dumped maps are that fit's maps at the dump's voxels, bit for bit."""
    import torch

    import fetal_t2mapping_amd as t2
    from fetal_t2mapping_amd import synth

    shape = (36, 256, 256)
    n = shape[0] * shape[1] * shape[2]
    out = tmp_path / "dump"
    run = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--shape", *map(str, shape), "--dump-outputs", str(out)],
                         capture_output=True, text=True, cwd=str(tmp_path))
    assert run.returncode == 0, run.stderr[-2000:]
    line = json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 3 and line["outputs_dumped"]["voxels"] == n
    # a plain run: the headline fields, nothing of what --full measures or checks besides
    assert line["full"] is False and line["value"] > 0 and line["ms_per_step"] > 0 and line["unit"] == "Mvoxel/s"
    assert not set(line) & set(bench.FULL_ONLY_KEYS) and line["gathered_maps_equal_single_gpu_fit"] is None
    assert line["outputs_dumped"]["voxels_written"] == bench.DUMP_MAX_VOXELS < n
    echoes, mask, te = synth.brain_volume_torch(shape, 8, synth.SEED_BASE + 3, torch.device("cuda", 0))
    maps = t2.fit_volume(echoes.reshape((8,) + shape), mask, te, "gaussian_rician", t2.fit_table("gaussian_rician", True))
    torch.cuda.synchronize()
    idx = bench.dump_index(n)
    inside = mask.cpu().numpy()[idx] != 0
    assert 0.3 < inside.mean() < 0.6
    for name in bench.DUMP_NAMES:
        got = np.load(out / (name + ".npy"))
        assert got.dtype == np.float32 and got.shape == (bench.DUMP_MAX_VOXELS,)
        assert np.array_equal(got, getattr(maps, name).reshape(-1).cpu().numpy()[idx], equal_nan=True), name
        assert np.all(got[~inside] == 0) and np.count_nonzero(got[inside]) > 0.99 * inside.sum()
