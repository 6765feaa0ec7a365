"""The float32 scores of the dictionary fit on the device: what v_mfma_f32_32x32x2_f32 computes from the operands of
DESIGN.md section 8r, read back through the documented accumulator map by the device probe (tests/devprobe, a kernel of its
own: the product kernel is held to the statement by tests/test_dict_gpu.py).

  a. |s32 - s64| <= gamma_K dmax |y|, gamma_K = K u / (1 - K u), u = 2^-24, K the padded echo count: the bound the
     candidate band T of the kernel is built on.  Nothing is fitted to the device here.
  b. the words of the device scores equal tests/dict_cases.py chain32, the emulation of the k-ordered float32 fma chain with
     subnormals kept: the candidate counts of section 8r are computed with that emulation.

Echo counts 2, 5, 6, 17, 32 (one k-step, an odd count with a zero-padded step, the common case, an odd count above 16, the
largest); 96 atoms are three tiles; 64 voxels are two groups; decays with noise 20 (near ties) and the same times 1e-40
(subnormal samples and scores).  A lane-to-row map other than the documented one, or operands the other way round, moves
scores to other (voxel, atom) pairs and fails both."""
import numpy as np
import pytest

import dict_cases as K
from fetal_t2mapping_amd import _dict

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(scope="module")
def probe():
    from devprobe import probe as p

    p.build()
    assert p.device_count() > 0, "no HIP device"
    return p


def operands(n_te, scale):
    atoms = K.atoms_for(96, n_te).atoms
    y = K.decays(n_te, 64, seed=60 + n_te, noise=20.0, scale=scale)
    return atoms, y


@pytest.mark.parametrize("scale", [1.0, 1e-40])
@pytest.mark.parametrize("n_te", [2, 5, 6, 17, 32])
def test_device_scores_keep_the_bound_and_equal_the_fma_chain(probe, n_te, scale):
    atoms, y = operands(n_te, scale)
    k_pad = n_te + n_te % 2
    dh, _, dmax = _dict.normalise(atoms)
    got = probe.dict_scores(_dict.pack(atoms), y)
    assert got.shape == (64, 96) and got.dtype == np.float32 and np.all(np.isfinite(got))
    s64 = _dict.scores(dh, y)
    assert len(np.unique(np.argmax(s64, axis=1))) > 10  # the voxels point at many atoms: rows and columns are told apart
    y64 = y.astype(np.float64)
    norm = np.sqrt(np.sum(y64 * y64, axis=0))
    bound = k_pad * U / (1.0 - k_pad * U) * float(dmax) * norm
    ratio = np.abs(got.astype(np.float64) - s64) / bound[:, None]
    want = K.chain32(dh, y, k_pad)
    off = got.view(np.uint32) != want.view(np.uint32)
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))  # (ulps where the signs agree)
    print(f"n_te {n_te} scale {scale}: largest |s32 - s64| / bound {ratio.max():.4f}; words that differ from chain32 {int(off.sum())} of "
          f"{off.size}, largest distance {int(ulps.max())} ulp; subnormal scores {int(np.sum(np.abs(got) < np.float32(K.SMALLEST_NORMAL)))}")
    assert ratio.max() <= 1.0
    if scale < 1.0:
        # subnormal operands are met (subnormal scores too from 5 echoes up: the count is printed)
        assert np.sum((y != 0) & (np.abs(y) < np.float32(K.SMALLEST_NORMAL))) >= 3
    assert not off.any(), (int(off.sum()), int(ulps.max()))
