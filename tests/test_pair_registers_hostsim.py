"""The last ratio of every correction pair kept in members of the lane solver (Lbfgsb<.., PAIRS_REG>: registers in the
one-wave-workgroup kernels) against the whole ring in one array (PAIRS_LDS): where a number is kept must not change it,
so x, fun, nit, nfev, status and the per-iteration traces agree bit for bit.  CPU, through tests/hostsim.

The rows are the first rows of the golden fixtures; every set must hold fits that end with fewer than 10 pairs, fits
that drop their oldest pair at least three times and (without the prior) fits that drop the memory and restart --
asserted from the solver's own counters, so that no path of the new storage goes unexercised."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hostsim import sim

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostsim", "pair_registers.cpp")
SO = os.path.join(HERE, "hostsim", "libt2fit_pair_registers.so")
GOLD = os.path.join(HERE, "golden")
N_ROWS = 300
CAP = 128  # iterations traced per row (maxiter of the reference is below it)


@pytest.fixture(scope="module")
def lib():
    deps = [SRC] + [os.path.join(sim.CSRC, f) for f in os.listdir(sim.CSRC) if f.endswith(".h")]
    if not (os.path.exists(SO) and all(os.path.getmtime(SO) >= os.path.getmtime(d) for d in deps)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-o", SO, SRC])
    return C.CDLL(SO)


def run(lib, cfg, rows, home):
    rows = np.ascontiguousarray(rows, np.float32)
    n = len(rows)
    out = np.zeros((n, 14))
    trace = np.zeros((n, CAP, 4))
    lib.hostsim_pairs_fit_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    rc = lib.hostsim_pairs_fit_rows(C.byref(cfg), rows.ctypes.data, n, home, out.ctypes.data, trace.ctypes.data, CAP)
    assert rc == 0, rc
    return out, trace


@pytest.mark.parametrize("n_te", [3, 6, 8])
@pytest.mark.parametrize("prior", [True, False])
@pytest.mark.parametrize("mode", ["gaussian_rician", "rician"])
def test_members_match_ring(lib, mode, prior, n_te):
    d = np.load(os.path.join(GOLD, f"voxels_lf_{mode}_{'prior' if prior else 'noprior'}_te{n_te}.npz"))
    rows = d["y"][:N_ROWS]
    cfg = sim.config(mode, bool(d["low_field"]), d["te"], prior=prior)
    ring, ring_tr = run(lib, cfg, rows, 0)
    regs, regs_tr = run(lib, cfg, rows, 1)
    col_end, n_drop, n_reset, rcs = (regs[:, j].astype(int) for j in (7, 8, 9, 11))
    fitted = rcs == 0
    print(f"{mode} prior={prior} te{n_te}: {fitted.sum()} rows fitted, {np.sum(fitted & (n_drop == 0) & (col_end < 10))} end "
          f"with < 10 pairs, {np.sum(n_drop >= 3)} drop the oldest pair >= 3 times, {np.sum(n_reset > 0)} drop the memory")
    # every path of the storage is in the set
    assert np.sum(fitted & (n_drop == 0) & (col_end < 10) & (col_end > 0)) > 0
    assert np.sum(n_drop >= 3) > 0
    if not prior:
        assert np.sum(n_reset > 0) > 0
    # bit for bit (the records are float64 throughout; NaN == NaN)
    assert np.array_equal(ring.view(np.uint64), regs.view(np.uint64))
    assert np.array_equal(ring_tr.view(np.uint64), regs_tr.view(np.uint64))
    assert np.all(regs[fitted, 10] == np.minimum(regs[fitted, 4], CAP))  # the traces were written: one entry per iteration


def test_store_load_members(lib):
    """store_s / load_s of the member form: what was pushed comes back (as a multiple: s is kept as a direction), right
    after the push and, for the ten newest, after 25 pushes that dropped the oldest pair 15 times."""
    rng = np.random.default_rng(7)
    s = rng.normal(size=(25, 3)) * 10.0 ** rng.integers(-6, 6, size=(25, 1))
    back = np.zeros_like(s)
    held = np.zeros((10, 3))
    lib.hostsim_pairs_roundtrip.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    assert lib.hostsim_pairs_roundtrip(s.ctypes.data, len(s), back.ctypes.data, held.ctypes.data) == 10
    want = s / s[:, :1]  # ratios to the first component, rounded once: within an ulp of the correctly rounded quotient
    assert np.all(back[:, 0] == 1.0) and np.all(held[:, 0] == 1.0)
    np.testing.assert_allclose(back, want, rtol=4e-16, atol=0)
    assert np.array_equal(held, back[-10:])
