"""The replica stream of the parametric bootstrap, restated in numpy: the definition the device kernel
(csrc/t2fit_boot.hip, boot_synth_kernel) is tested against.  Pure numpy, no device.

Philox4x32-10 is the counter-based generator of Salmon, Moraes, Dror and Shaw, "Parallel random numbers: as easy as
1, 2, 3" (SC'11): the four 32-bit words of a block are a function of a 128-bit counter and a 64-bit key alone.  The
bootstrap uses key = (seed low, seed high) and counter = (voxel low, voxel high, echo, replica), so a sample depends on
(seed, voxel, echo, replica) and nothing else.
"""
from __future__ import annotations

import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
_LOW = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32-10.  ``counter``: four array-likes of uint32 (broadcast against each other), ``key``: two.  Returns
    the four uint32 output words as a tuple of arrays of the broadcast shape."""
    c = [np.asarray(x, dtype=np.uint32) for x in np.broadcast_arrays(*[np.asarray(v, dtype=np.uint32) for v in counter])]
    k0, k1 = (np.asarray(v, dtype=np.uint32) for v in key)
    c0, c1, c2, c3 = c
    with np.errstate(over="ignore"):
        for _ in range(10):
            p0 = _M0 * c0.astype(np.uint64)
            p1 = _M1 * c2.astype(np.uint64)
            hi0, lo0 = (p0 >> _S32).astype(np.uint32), (p0 & _LOW).astype(np.uint32)
            hi1, lo1 = (p1 >> _S32).astype(np.uint32), (p1 & _LOW).astype(np.uint32)
            c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
            k0 = (k0 + _W0).astype(np.uint32)
            k1 = (k1 + _W1).astype(np.uint32)
    return c0, c1, c2, c3


def uniforms(w):
    """``((w >> 9) + 0.5) * 2**-23``: an odd multiple of 2**-24 inside (0, 1) -- 24 significant bits, so the value is
    exact in float32 (24 bits of the word plus the half would need 25)."""
    return ((np.asarray(w, np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def normals(voxel, echo, replica, seed):
    """The Box-Muller pair ``(n1, n2)`` of sample (voxel, echo, replica) under ``seed``, float64: words 0 and 1 of the
    block; words 2 and 3 are not used.  ``voxel`` is the flat index in the whole volume (64 bits)."""
    v = np.asarray(voxel, dtype=np.uint64)
    seed = int(seed) & (2 ** 64 - 1)
    w0, w1, _, _ = philox4x32_10(((v & _LOW).astype(np.uint32), (v >> _S32).astype(np.uint32), echo, replica),
                                 (seed & 0xFFFFFFFF, seed >> 32))
    rad = np.sqrt(-2.0 * np.log(uniforms(w0)))
    ang = 2.0 * np.pi * uniforms(w1)
    return rad * np.cos(ang), rad * np.sin(ang)


def replica(t2, k, te_ms, noise_sigma, mask, *, seed, replica, noise="rician", voxel_offset=0):
    """The acquisition :func:`fetal_t2mapping_amd.synth_replica` makes on the device, in float64: ``(nTE,) + shape``.
    ``noise_sigma``: a number or an array shaped like ``t2``.  Voxels outside ``mask`` (when given) are 0."""
    t2 = np.asarray(t2, np.float64)
    k = np.asarray(k, np.float64)
    te = np.asarray(te_ms, np.float64).astype(np.float32).astype(np.float64)  # the kernel holds the echo times in float32
    s = np.broadcast_to(np.asarray(noise_sigma, np.float64), t2.shape)
    v = np.arange(t2.size, dtype=np.uint64).reshape(t2.shape) + np.uint64(voxel_offset)
    out = np.empty((te.size,) + t2.shape)
    for j in range(te.size):
        n1, n2 = normals(v, j, replica, seed)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            clean = k * np.exp(-te[j] / t2)
        out[j] = np.hypot(clean + s * n1, s * n2) if noise == "rician" else clean + s * n1
    if mask is not None:
        out[:, np.asarray(mask) == 0] = 0.0
    return out
