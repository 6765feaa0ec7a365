"""The headline lane solver (Lbfgsb<.., NTE, PAIRS_REG>: what the one-wave-workgroup kernels run) against a record of
what it computed BEFORE the second pass over the round's scalar, branch and ring-addressing work: x, fun, nit and
status of four row sets, byte for byte.  CPU, through tests/hostsim (the solver header is shared with the kernels, so
a change of arithmetic shows here without a GPU).

tests/golden/round2_hostsim_parent.npz was written by `python tests/test_round2_bits_hostsim.py --record` with the
headers of the commit before that pass; it is not regenerated with later headers.

The row sets hold fits with more than ten stored pairs (the ring's head is then non-zero and build_b() takes the wrap
of the ring), and -- without the prior -- fits that drop the memory and restart."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from hostsim import sim  # noqa: E402

from fetal_t2mapping_amd import synth  # noqa: E402

SRC = os.path.join(HERE, "hostsim", "pair_registers.cpp")
SO = os.path.join(HERE, "hostsim", "libt2fit_pair_registers.so")
GOLD = os.path.join(HERE, "golden", "round2_hostsim_parent.npz")
N_ROWS = 4096
#       id              shape         n_te  seed offset  prior  fill
SETS = [("te8_prior",   (4, 64, 64),  8,    50,          True,  0.45),
        ("te8_noprior", (4, 64, 64),  8,    50,          False, 0.45),
        ("te6_prior",   (4, 64, 64),  6,    51,          True,  0.45),
        ("sparse",      (20, 64, 64), 8,    52,          False, 0.008)]


def _lib():
    deps = [SRC] + [os.path.join(sim.CSRC, f) for f in os.listdir(sim.CSRC) if f.endswith(".h")]
    if not (os.path.exists(SO) and all(os.path.getmtime(SO) >= os.path.getmtime(d) for d in deps)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-o", SO, SRC])
    return C.CDLL(SO)


def _rows(shape, n_te, seed, fill):
    echoes, mask, te = synth.brain_volume(shape, n_te, synth.SEED_BASE + seed, low_field=True, fill=fill)
    rows = echoes.reshape(n_te, -1).T[mask.reshape(-1) != 0][:N_ROWS]
    return np.ascontiguousarray(rows, np.float32), te


def _fit(lib, name, shape, n_te, seed, prior, fill):
    rows, te = _rows(shape, n_te, seed, fill)
    cfg = sim.config("gaussian_rician", True, te, prior=prior)
    n = len(rows)
    out = np.zeros((n, 14))
    trace = np.zeros((n, 1, 4))
    lib.hostsim_pairs_fit_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    rc = lib.hostsim_pairs_fit_rows(C.byref(cfg), rows.ctypes.data, n, 1, out.ctypes.data, trace.ctypes.data, 1)
    assert rc == 0, rc
    assert np.all(out[:, 11] == 0)  # every row was fitted
    return {"x": np.ascontiguousarray(out[:, 0:3]), "fun": np.ascontiguousarray(out[:, 3]),
            "nit": out[:, 4].astype(np.int32), "status": out[:, 6].astype(np.uint8),
            "n_drop": out[:, 8].astype(np.int32), "n_reset": out[:, 9].astype(np.int32)}


@pytest.fixture(scope="module")
def lib():
    return _lib()


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("case", SETS, ids=[s[0] for s in SETS])
def test_rows_match_the_record(lib, gold, case):
    name = case[0]
    got = _fit(lib, *case)
    n = len(got["nit"])
    assert n == (N_ROWS if name != "sparse" else len(gold[name + "/nit"])) and n > 256
    print(f"{name}: {n} rows, nit median {int(np.median(got['nit']))} max {int(got['nit'].max())}, "
          f"{int(np.sum(got['n_drop'] > 0))} rows dropped an oldest pair, {int(np.sum(got['n_reset'] > 0))} dropped the memory")
    # the ring wraps: more iterations than the ring has slots, and the oldest pair was dropped (head != 0)
    assert got["nit"].max() > 12
    assert np.sum(got["n_drop"] > 0) > 0
    if not case[4]:
        assert np.sum(got["n_reset"] > 0) > 0  # the memory drop is in the set
    for f in ("x", "fun", "nit", "status"):
        a, b = got[f], gold[f"{name}/{f}"]
        assert a.dtype == b.dtype and a.shape == b.shape, (name, f)
        assert a.tobytes() == b.tobytes(), (name, f, int(np.sum(a.view(np.uint8) != b.view(np.uint8))))


if __name__ == "__main__":
    if "--record" in sys.argv:
        rec = {}
        L = _lib()
        for s in SETS:
            r = _fit(L, *s)
            for f in ("x", "fun", "nit", "status"):
                rec[f"{s[0]}/{f}"] = r[f]
            print(s[0], len(r["nit"]), "rows, nit max", int(r["nit"].max()), "drops", int(np.sum(r["n_drop"] > 0)),
                  "resets", int(np.sum(r["n_reset"] > 0)))
        np.savez_compressed(GOLD, **rec)
        print(GOLD, os.path.getsize(GOLD), "bytes")
