"""The branch-free solver logic (dcsrch / dcstep selects, the Cauchy point's breakpoint walk, the begin-iteration tail) may
be restated -- which predicate selects what, as lane masks or as bits of an integer -- but never recomputed: every row of
the least-squares golden fixtures must come out of the host-side lane simulator with the parameters, objective value,
iteration count and status frozen in tests/golden/lane_solver_bits.npz (tests/golden/make_lane_bits.py), bit for bit."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import make_lane_bits  # noqa: E402

FILES = make_lane_bits.names()


@pytest.mark.parametrize("path", FILES, ids=lambda p: os.path.basename(p)[7:-4])
def test_lane_solver_results_are_bit_identical_to_the_frozen_ones(path):
    keep = np.load(os.path.join(GOLDEN, "lane_solver_bits.npz"))
    name = os.path.basename(path)[7:-4]
    o = make_lane_bits.fit(path)
    assert np.array_equal(o["nit"], keep[name + "/nit"])
    assert np.array_equal(o["status"], keep[name + "/status"])
    assert np.array_equal(o["x"].view(np.uint64), keep[name + "/x"])
    assert np.array_equal(o["fun"].view(np.uint64), keep[name + "/fun"])


def test_the_frozen_rows_walk_the_cauchy_breakpoints_and_the_safeguarded_steps():
    """The fixture is only a check of the restated blocks if its rows go through them: fits that end at a bound (a
    breakpoint of the projected path was taken), fits with line searches of several evaluations, and restarts."""
    keep = np.load(os.path.join(GOLDEN, "lane_solver_bits.npz"))
    at_bound = many_evals = 0
    for path in FILES:
        d = np.load(path)
        name = os.path.basename(path)[7:-4]
        x = keep[name + "/x"].view(np.float64)
        nit = keep[name + "/nit"]
        if bool(d["prior"]):
            at_bound += int(np.sum(x[:, 1] == x[:, 1].max()) + np.sum(x[:, 1] == x[:, 1].min()))
        many_evals += int(np.sum(nit >= 10))
    assert at_bound >= 50 and many_evals >= 500, (at_bound, many_evals)
