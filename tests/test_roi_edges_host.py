"""The per-label ROI statistics without a device: the numpy statement of tests/roi_cases.py (what the header of
csrc/t2fit_roi.hip fixes: segments in voxel order, the 256-lane sum tree, numpy's two rounds, the radix key of the median)
against a reference written from the definition in exact arithmetic, within bars that are derived in roi_cases.bars; four
mutations of the statement that must fail; the key order.  tests/test_roi_edges_gpu.py holds the device to the statement
bit for bit."""
import numpy as np
import pytest

import roi_cases as K


def _check_statement_against_reference(cases=None, fresh=False):
    """Counts exact, medians bit-equal, means and variances within the derived bars, constant regions with std == 0.0;
    returns the largest |error| / bar of the means and of the variances."""
    worst_mean = worst_var = 0.0
    for c in (K.all_cases() if cases is None else cases):
        if not c.finite:
            continue
        s = K.statement(c.map, c.roi, c.n_labels) if fresh else K.expected(c)
        for i in range(c.n_labels):
            sel = c.map[c.roi == i + 1]
            good = sel[~np.isnan(sel)]
            assert s.count[i] == len(sel) and s.valid[i] == len(good), (c.name, i)
            if len(good) == 0:
                assert np.isnan(s.mean[i]) and np.isnan(s.std[i]) and np.isnan(s.median[i]), (c.name, i)
                continue
            r_mean, r_var, ref = K.ratios(s.mean[i], s.std[i], good)
            assert K.bits_equal([s.median[i]], [ref.median]), (c.name, i, s.median[i], ref.median)
            assert r_mean <= 1.0, (c.name, i, "mean", r_mean)
            assert r_var <= 1.0, (c.name, i, "variance", r_var)
            if np.all(good == good[0]):
                assert s.std[i] == 0.0 and s.mean[i] == float(good[0]), (c.name, i)
            worst_mean, worst_var = max(worst_mean, r_mean), max(worst_var, r_var)
    return worst_mean, worst_var


def test_statement_is_within_the_derived_bars_of_the_from_definition_reference():
    """Every finite case (the sizes 1 .. 257 * 8192 - 5, the parting segments, the ragged trees, the edge values, the
    out-of-range labels).  Largest |error| / bar measured: mean 0.0575 (bar 2 (k + 9) u sum |x| / n), variance 0.107
    (bar 2 (k + 14) u V + delta^2)."""
    worst_mean, worst_var = _check_statement_against_reference()
    print(f"largest |error| / bar: mean {worst_mean:.3g}, variance {worst_var:.3g}")
    assert 0.0 < worst_mean and 0.0 < worst_var  # the bars were exercised by sums that do round


def test_the_cases_are_what_they_claim():
    names = [c.name for c in K.all_cases()]
    assert len(set(names)) == len(names)
    for n in K.SIZES:
        c = K.case(f"size-{n}")
        assert c.shape == (1, 1, n) and c.map.dtype == np.float32 and c.roi.dtype == np.int32 and c.n_labels == 6
        assert K.expected(c).count[5] == 1 and c.roi[n - 1] == 6
    big = K.case(f"size-{257 * K.SPAN - 5}")
    n_units = -(-len(big.roi) // K.SPAN)
    per = -(-n_units // 256)
    assert n_units == 257 and per == 2 and n_units % per == 1 and len(big.roi) % 64 != 0  # the scan's thread 128 takes one unit
    assert len(K.case(f"size-{4 * K.SPAN + 1}").roi) - 4 * K.SPAN == 1  # a second workgroup: one live wave, one voxel
    for c in K.all_cases():
        assert c.n_labels <= 6 or c.name == "labels-256"
    s = K.expected(K.case("size-8191"))
    assert s.valid[3] < s.count[3] and np.array_equal(s.valid[[0, 1, 2, 4]], s.count[[0, 1, 2, 4]])
    for p in range(4):
        s = K.expected(K.case(f"parting-pass-{p}"))
        assert list(s.count[:2]) == [1000, 1001]
    for c in K.label_cases():
        for v in (-1, c.n_labels + 1, K.INT32_MIN, K.INT32_MAX):
            assert np.any(c.roi == v)
        assert K.expected(c).count[c.n_labels - 1] > 0 and np.any((c.roi < 0) | (c.roi > c.n_labels))


def test_edge_values_of_the_statement():
    """Denormals are not flushed (the reference mean is not 0), the zeros keep the sign the total order gives the median,
    and on the non-finite regions the statement says what np.mean / np.std / np.median say."""
    c = K.case("edge-values")
    s = K.expected(c)
    den = c.map[c.roi == 1]
    ref = K.reference(den)
    assert ref.mean != 0 and s.mean[0] != 0.0 and abs(s.mean[0]) < 1.2e-38 and s.std[0] > 0.0
    assert s.mean[1] != 0.0 and np.isfinite(s.std[1]) and s.std[1] > 1e38  # +-max: nothing overflows in float64
    assert s.mean[2] < 0.0 and s.median[2] < 0.0 and np.all(c.map[c.roi == 3] < 0)
    assert s.median[3] == 0.0 and not np.signbit(s.median[3]) and s.count[3] == 3   # [-0.0, 0.0, 0.0]: the middle one is +0.0
    assert s.median[4] == 0.0 and np.signbit(s.median[4]) and s.count[4] == 2       # [-0.0, -0.0]
    assert s.std[3] == 0.0 and s.std[4] == 0.0
    c = K.case("non-finite")
    s = K.expected(c)
    with np.errstate(all="ignore"):
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for i in range(c.n_labels):
                v = c.map[c.roi == i + 1].astype(np.float64)
                assert np.array_equal([s.mean[i], s.std[i], s.median[i]], [np.mean(v), np.std(v), np.median(v)], equal_nan=True), i
    assert s.mean[0] == np.inf and np.isnan(s.std[0]) and np.isfinite(s.median[0])
    assert np.isnan(s.mean[1]) and np.isfinite(s.median[1]) and np.isnan(s.median[2]) and s.median[3] == np.inf


def test_mutations_of_the_statement_fail(monkeypatch):
    """The ragged last row dropped, the 256 partial sums added one after the other, the one-round variance: each must
    fail the reference check on the case whose segments have a ragged last group of 256.  Reversing the values inside
    the segments must change the bits of a mean: that is what lets the device test see a scatter that is not stable."""
    ragged = [c for c in K.all_cases() if c.ragged]
    assert ragged and all(len(seg) % 256 not in (0, len(seg)) for c in ragged for seg in K.expected(c).segments)
    check = lambda: _check_statement_against_reference(ragged, fresh=True)  # noqa: E731
    check()
    rows = K._rows

    with monkeypatch.context() as m:
        m.setattr(K, "_rows", lambda v: rows(v[: len(v) // 256 * 256] if len(v) > 256 else v))
        with pytest.raises(AssertionError, match="mean"):
            check()

    def sequential(sh):
        total = np.float64(0.0)
        for v in sh:
            total = total + v
        return total

    with monkeypatch.context() as m:
        m.setattr(K, "_halve", sequential)
        with pytest.raises(AssertionError, match="mean"):
            check()

    def one_round(x):
        n = np.float64(len(x))
        mean = K.tree_sum(x) / n
        return mean, np.sqrt(np.maximum(K.tree_sum(x * x) / n - mean * mean, 0.0))

    with monkeypatch.context() as m:
        m.setattr(K, "_moments", one_round)
        with pytest.raises(AssertionError, match="variance"):
            check()

    with monkeypatch.context() as m:
        m.setattr(K, "_in_segment", lambda v: v[::-1])
        changed = []
        for c in K.all_cases():
            s, want = K.statement(c.map, c.roi, c.n_labels), K.expected(c)
            assert K.bits_equal(s.median, want.median) and np.array_equal(s.valid, want.valid)  # order-blind
            changed += [(c.name, i) for i in range(c.n_labels) if not K.bits_equal(s.mean[i: i + 1], want.mean[i: i + 1])]
            if len(changed) >= 8 and len({name for name, _ in changed}) >= 3:
                break
        print("reversed segments change the mean's bits in", changed)
        assert len(changed) >= 8 and len({name for name, _ in changed}) >= 3
    check()  # (the patches are gone)


def test_key_order_and_round_trip():
    tiny = np.float32(1e-45)
    edge = np.array([-np.inf, -K.F32_MAX, -1.0, -np.finfo(np.float32).tiny, -tiny, -0.0, 0.0, tiny, np.finfo(np.float32).tiny,
                     1.0, K.F32_MAX, np.inf], np.float32)
    k = K.float_key(edge)
    assert k.dtype == np.uint32 and np.all(k[1:] > k[:-1])
    assert np.array_equal(K.key_float(k).view(np.uint32), edge.view(np.uint32))
    assert k[5] == 0x7FFFFFFF and k[6] == 0x80000000  # the zeros are neighbours
    rng = np.random.default_rng(9)
    bits = np.concatenate([rng.integers(0, 2 ** 32, 4000, dtype=np.uint64).astype(np.uint32), edge.view(np.uint32)])
    assert np.array_equal(K.float_key(K.key_float(bits)), bits)  # key -> float -> key, every pattern (NaNs included)
    f = bits.view(np.float32)
    assert np.array_equal(K.key_float(K.float_key(f)).view(np.uint32), bits)
    fin = np.sort(f[np.isfinite(f) & (f != 0)])  # (np.sort does not tell the two zeros apart; they are held above)
    assert np.all(np.diff(K.float_key(fin).astype(np.int64)) >= 0)
