"""The assertions that hold an implementation of the fit (host lane simulator, HIP path) to the reference's own spread in
k, sigma, the objective and the iteration traces: tests/golden/param_floor.npz (make_param_floor.py) is the yardstick,
oracle/noise_model.py defines the statistics.  Shared by test_lane_solver_hostsim.py and test_gpu_parity.py."""
import os

import numpy as np

from conftest import GOLDEN
from oracle.noise_model import exceeds_yardstick, deviation_stats, fun_deviation, rel_deviation, trace_deviation

T2_STABLE_MS = 1e-3  # the stable rule itself: every perturbed run of the reference stays within it


def param_floor():
    return np.load(os.path.join(GOLDEN, "param_floor.npz"))


class StableSetTally:
    """Deviations from the golden rows over the stable sets of the fixtures of ONE model, next to the yardstick's, pooled
    over (row, seed) pairs.  ``frozen``: the frozen-stack rows and yardstick (param_floor.npz frozen/<name>/...)."""

    def __init__(self, frozen=False):
        self.pf = param_floor()
        self.prefix = "frozen/" if frozen else ""
        self.got = {"k": [], "sigma": [], "fun": []}
        self.yard = {"k": [], "sigma": [], "fun": []}
        self.dt = []

    def add(self, name, rows, x, fun, gold_x, gold_fun, y):
        """``rows``: the fixture rows fitted (must be the yardstick's); ``x`` (n, >= n_par), ``fun`` (n,): the
        implementation's float64 results; ``gold_x`` / ``gold_fun`` / ``y``: the fixture's arrays at those rows."""
        key = self.prefix + name
        assert np.array_equal(rows, self.pf[key + "/rows"]), name
        at = slice(None)
        if key + "/k_rel" not in self.pf.files:  # frozen stack, least-squares models: the default stack's perturbed fits ARE
            key = name                           # the frozen stack's (same objective): its per-seed arrays at these rows
            at = np.searchsorted(self.pf[key + "/rows"], rows)
            assert np.array_equal(self.pf[key + "/rows"][at], rows), name
        assert np.all(np.isfinite(fun)) and np.all(np.isfinite(x[:, : gold_x.shape[1]])), name
        self.dt.append(np.abs(x[:, 1] - gold_x[:, 1]))
        self.got["k"].append(rel_deviation(x[:, 0], gold_x[:, 0]))
        self.yard["k"].append(self.pf[key + "/k_rel"][:, at].ravel())
        self.got["fun"].append(fun_deviation(fun, gold_fun, y))
        self.yard["fun"].append(self.pf[key + "/fun_dev"][:, at].ravel())
        if gold_x.shape[1] == 3:
            self.got["sigma"].append(rel_deviation(x[:, 2], gold_x[:, 2]))
            self.yard["sigma"].append(self.pf[key + "/sigma_rel"][:, at].ravel())

    def report(self):
        rep = {"t2_abs_max_ms": float(np.max(np.concatenate(self.dt))),
               "t2_within_stable_rule": float(np.mean(np.concatenate(self.dt) <= T2_STABLE_MS))}
        for what in ("k", "sigma", "fun"):
            if self.got[what]:
                rep[what] = deviation_stats(np.concatenate(self.got[what]))
                rep[what + "_yardstick"] = deviation_stats(np.concatenate(self.yard[what]))
        return rep

    def check(self, label):
        """median / 99th percentile / maximum of k, sigma and fun deviations <= 1.2 x the yardstick's (+ a few float64 ulps);
        T2 within the stable rule (1e-3 ms) of the golden row on >= 99 % of the rows."""
        rep = self.report()
        print("stable_set_parameters " + repr({"set": label, **rep}))
        for what in ("k", "sigma", "fun"):
            if self.got[what]:
                over = exceeds_yardstick(np.concatenate(self.got[what]), np.concatenate(self.yard[what]))
                assert not over, (label, what, over, rep)
        assert rep["t2_within_stable_rule"] >= 0.99, (label, rep)
        return rep


class TraceTally:
    """Per-iteration deviations of traces from the golden ones on the stable traced rows, next to the yardstick's
    (maximum over the 24 seeds per row and iteration)."""

    def __init__(self):
        self.pf = param_floor()
        self.got_f, self.got_s, self.yard_f, self.yard_s = [], [], [], []
        self.n = 0

    def rows(self, name):
        return self.pf[name + "/trace_rows"]

    def add(self, name, d, j, got_f, got_s):
        """Row ``rows(name)[j]`` of fixture ``d``: its trace (f_val and step per iteration; the first step is NaN)."""
        r = int(self.rows(name)[j])
        t = r - int(d["trace_first_row"])
        want_f = d["trace_f"][t][np.isfinite(d["trace_f"][t])]
        want_s = d["trace_step"][t][: len(want_f)]
        assert len(got_f) == len(want_f) == int(d["nit"][r]), (name, r, len(got_f), len(want_f))
        assert np.isnan(got_s[0])
        df, ds = trace_deviation(got_f, got_s, want_f, want_s, d["y"][r])
        defined = want_s[1:] > 0  # (a golden step of exactly 0 has no relative deviation)
        assert np.all(np.isfinite(df)) and np.all(np.isfinite(ds[defined])), (name, r)
        self.got_f.append(df)
        self.got_s.append(ds[defined])
        self.yard_f.append(self.pf[name + "/trace_f_dev"][j][: len(want_f)])
        self.yard_s.append(self.pf[name + "/trace_step_dev"][j][1: len(want_f)][defined])
        self.n += 1

    def check(self, label):
        """median / 90th percentile / maximum over (row, iteration) of the f_val and step deviations <= 1.2 x the yardstick's."""
        qs = (50, 90, 100)
        rep = {"rows": self.n}
        for what, got, yard in (("f_val", self.got_f, self.yard_f), ("step", self.got_s, self.yard_s)):
            got, yard = np.concatenate(got), np.concatenate(yard)
            rep[what] = deviation_stats(got, qs)
            rep[what + "_yardstick"] = deviation_stats(yard, qs)
        print("trace_parameters " + repr({"set": label, **rep}))
        for what, got, yard in (("f_val", self.got_f, self.yard_f), ("step", self.got_s, self.yard_s)):
            over = exceeds_yardstick(np.concatenate(got), np.concatenate(yard), qs)
            assert not over, (label, what, over, rep)
        return rep
