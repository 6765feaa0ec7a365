"""The one-wave-workgroup L-BFGS-B kernels against a record of the maps they wrote BEFORE the second pass over the
solver round's scalar, branch and ring-addressing work: SHA-256 of t2 / k / sigma / res (and of fun / nit / status where
the extras kernel is asked for) of seven small fits, compared with tests/golden/round2_gpu_parent_digests.json, which
was written by `python tests/test_round2_bits_gpu.py --record` with the library of the commit before that pass.

Unlike the workgroup-shape comparison of test_pair_registers_gpu.py, whose two sides share the solver header, this
holds the kernels to what an earlier build computed.  The volumes are the six of that test (device tensors, so that
the four-map kernel runs) plus one te8_prior fit that asks for fun / nit / status (the extras kernel).  The
large-volume dispatch is read once per process (T2FIT_SMALL_VOLUME), so the fits run in one fresh interpreter."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "round2_gpu_parent_digests.json")
MAPS = ("t2", "k", "sigma", "res")
EXTRAS = ("fun", "nit", "status")
#        id                   shape          n_te  prior  fill   seed index  extras
CASES = [("te8_prior",        (20, 64, 64),  8,    True,  0.45,  0,          False),
         ("te8_noprior",      (20, 64, 64),  8,    False, 0.45,  1,          False),
         ("te6_prior",        (20, 64, 64),  6,    True,  0.45,  2,          False),
         ("te6_noprior",      (20, 64, 64),  6,    False, 0.45,  3,          False),
         ("ragged",           (19, 63, 61),  8,    False, 0.45,  4,          False),  # 57 voxels over a multiple of 64
         ("sparse",           (20, 64, 64),  8,    False, 0.008, 5,          False),  # mask fill below 1 %
         ("te8_prior_extras", (20, 64, 64),  8,    True,  0.45,  0,          True)]

_CHILD = """
import sys
import numpy as np
import torch
import fetal_t2mapping_amd as t2
from fetal_t2mapping_amd import synth
from fetal_t2mapping_amd._gpu_fit import T2Maps
cases = eval(sys.argv[2])
dev = torch.device("cuda", 0)
out = {}
for name, shape, n_te, prior, fill, seed, extras in cases:
    echoes, mask, te = synth.brain_volume(shape, n_te, synth.SEED_BASE + 40 + seed, low_field=True, fill=fill)
    new = lambda dt: torch.zeros(shape, dtype=dt, device=dev)
    maps = T2Maps(new(torch.float32), new(torch.float32), new(torch.float32), new(torch.float32))
    if extras:
        maps.fun, maps.nit, maps.status = new(torch.float32), new(torch.int32), new(torch.uint8)
    m = t2.fit_volume(torch.from_numpy(echoes).to(dev).contiguous(), torch.from_numpy(mask).to(dev).contiguous(), te,
                      "gaussian_rician", t2.fit_table("gaussian_rician", True), prior=prior, out=maps)
    torch.cuda.synchronize()
    for f in ("t2", "k", "sigma", "res") + (("fun", "nit", "status") if extras else ()):
        out[name + "/" + f] = getattr(m, f).cpu().numpy()
    out[name + "/mask"] = mask
np.savez(sys.argv[1], **out)
"""


def _fit_all(path):
    env = dict(os.environ, T2FIT_SMALL_VOLUME="0", PYTHONPATH=REPO)
    subprocess.run([sys.executable, "-B", "-c", _CHILD, path, repr(CASES)], env=env, check=True, timeout=120)
    return dict(np.load(path))


def _digests(maps):
    return {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in sorted(maps.items())
            if not k.endswith("/mask")}


@pytest.fixture(scope="module")
def fitted(tmp_path_factory):
    return _fit_all(str(tmp_path_factory.mktemp("round2_bits") / "maps.npz"))


@pytest.fixture(scope="module")
def gold():
    with open(GOLD) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_maps_match_the_record(fitted, gold, case):
    name, shape, n_te, prior, fill, seed, extras = case
    mask = fitted[name + "/mask"]
    n_fit, n_vox = int(mask.sum()), mask.size
    assert n_fit > 64  # more than one wave's worth of fits
    if name == "ragged":
        assert n_vox % 64 != 0
    if name == "sparse":
        assert n_fit < 0.01 * n_vox
    got = _digests({k: v for k, v in fitted.items() if k.startswith(name + "/")})
    for f in MAPS + (EXTRAS if extras else ()):
        a = fitted[f"{name}/{f}"]
        assert a.shape == tuple(shape)
        assert got[f"{name}/{f}"] == gold[f"{name}/{f}"], (name, f)
    t2m = fitted[name + "/t2"]
    assert np.all(t2m[mask == 0] == 0) and np.count_nonzero(t2m[mask != 0]) > 0.9 * n_fit  # a fit took place
    if extras:
        assert fitted[name + "/nit"][mask != 0].max() > 12  # fits that wrap the ring of ten pairs


if __name__ == "__main__":
    if "--record" in sys.argv:
        import tempfile

        with tempfile.TemporaryDirectory() as tmp:
            d = _digests(_fit_all(os.path.join(tmp, "maps.npz")))
        dst = sys.argv[sys.argv.index("--record") + 1] if len(sys.argv) > sys.argv.index("--record") + 1 else GOLD
        with open(dst, "w") as f:
            json.dump(d, f, indent=1, sort_keys=True)
            f.write("\n")
        print(dst, len(d), "digests")
