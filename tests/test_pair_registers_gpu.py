"""The one-wave-workgroup kernels (last ratio of every correction pair in the lane's registers) against the 256-lane
workgroups (whole ring in LDS): the four maps bit for bit, NaN == NaN.  The large-volume dispatch and the workgroup
shape are read once per process (T2FIT_SMALL_VOLUME, T2FIT_WAVE_WG), so each side runs in a fresh interpreter -- one
per side for all cases, each with its own time limit.  What tools/soak_kernel_variants.py compares, with fixed seeds.

Two of the volumes make waves run with few lanes and refill often, so that a lane's pair registers are taken over by a
new voxel right after a long fit: a voxel count that is no multiple of 64 and a mask that fills less than 1 %."""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPS = ("t2", "k", "sigma", "res")
#        id               shape          n_te  prior  fill
CASES = [("te8_prior",    (20, 64, 64),  8,    True,  0.45),
         ("te8_noprior",  (20, 64, 64),  8,    False, 0.45),
         ("te6_prior",    (20, 64, 64),  6,    True,  0.45),
         ("te6_noprior",  (20, 64, 64),  6,    False, 0.45),
         ("ragged",       (19, 63, 61),  8,    False, 0.45),   # 73017 voxels in the volume (not in the mask): 57 over a multiple of 64
         ("sparse",       (20, 64, 64),  8,    False, 0.008)]  # mask fill below 1 %

_CHILD = """
import sys
import numpy as np
import fetal_t2mapping_amd as t2
from fetal_t2mapping_amd import synth
cases = eval(sys.argv[2])
out = {}
for i, (name, shape, n_te, prior, fill) in enumerate(cases):
    echoes, mask, te = synth.brain_volume(shape, n_te, synth.SEED_BASE + 40 + i, low_field=True, fill=fill)
    m = t2.fit_volume(echoes, mask, te, "gaussian_rician", t2.fit_table("gaussian_rician", True), prior=prior, strict=False)
    for f in ("t2", "k", "sigma", "res"):
        out[name + "/" + f] = np.asarray(getattr(m, f))
    out[name + "/mask"] = mask
np.savez(sys.argv[1], **out)
"""


def _side(tmp, wave_wg):
    path = str(tmp / f"maps_wave_wg{wave_wg}.npz")
    env = dict(os.environ, T2FIT_SMALL_VOLUME="0", T2FIT_WAVE_WG=str(wave_wg), PYTHONPATH=REPO)
    subprocess.run([sys.executable, "-B", "-c", _CHILD, path, repr(CASES)], env=env, check=True, timeout=120)
    return dict(np.load(path))


@pytest.fixture(scope="module")
def sides(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pair_registers")
    return _side(tmp, 1), _side(tmp, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_registers_match_whole_ring(sides, case):
    name, shape, n_te, prior, fill = case
    regs, ring = sides
    mask = regs[name + "/mask"]
    n_fit, n_vox = int(mask.sum()), mask.size
    assert n_fit > 64  # more than one wave's worth of fits
    if name == "ragged":
        assert n_vox % 64 != 0
    if name == "sparse":
        assert n_fit < 0.01 * n_vox
    for f in MAPS:
        a, b = regs[f"{name}/{f}"], ring[f"{name}/{f}"]
        assert a.shape == tuple(shape) and a.dtype == np.float32
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, f, int(np.sum(a.view(np.uint32) != b.view(np.uint32))))
    t2m = regs[name + "/t2"]
    assert np.all(t2m[mask == 0] == 0) and np.count_nonzero(t2m[mask != 0]) > 0.9 * n_fit  # a fit took place
