"""Freeze the lane solver's results on the golden voxel fixtures, bit for bit (tests/test_lane_solver_bits.py).

    python tests/golden/make_lane_bits.py        # writes tests/golden/lane_solver_bits.npz

Run it with the solver headers whose results are to be kept: a restatement of the solver's branch-free logic (which
predicate selects what, in which form) must reproduce every number of this file -- parameters, objective value,
iteration count, status -- on every row of the least-squares fixtures, through the host-side lane simulator.  The
Rician-likelihood fixtures are left out: their objective calls the C library's logf, whose last bit is not ours.
"""
import glob
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from hostsim import sim  # noqa: E402


def fit(path):
    d = np.load(path)
    cfg = sim.config(str(d["mode"]), bool(d["low_field"]), d["te"], prior=bool(d["prior"]), solver="lbfgsb")
    return sim.fit_rows(cfg, d["y"])


def names():
    out = []
    for p in sorted(glob.glob(os.path.join(HERE, "voxels_*.npz"))):
        if str(np.load(p)["mode"]) != "rician":
            out.append(p)
    return out


if __name__ == "__main__":
    keep = {}
    for p in names():
        o = fit(p)
        n = os.path.basename(p)[7:-4]
        keep[n + "/x"] = o["x"].view(np.uint64)
        keep[n + "/fun"] = o["fun"].view(np.uint64)
        keep[n + "/nit"] = o["nit"]
        keep[n + "/status"] = o["status"]
    np.savez_compressed(os.path.join(HERE, "lane_solver_bits.npz"), **keep)
    print(len(keep) // 4, "fixtures,", sum(len(v) for k, v in keep.items() if k.endswith("/nit")), "rows")
