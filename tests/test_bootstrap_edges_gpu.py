"""The parametric bootstrap where replicas drop out, and its edges (csrc/t2fit_boot.hip).  tests/test_bootstrap_gpu.py pins
the in-library loop on synthetic brains where every replica counts; here the crafted case of tests/boot_cases.py makes the
count differ from voxel to voxel (0..R, known on the CPU), puts exact ties on both T2 bounds, and the reduction is held
against numpy in float64 on the very float32 refits the device reduced.  Then the edges of R, of the mask count, of the
synthesis counters and operands, unaligned and guarded pointers, a caller's stream with the inputs in flight, and the
background level at its small end.  Every test takes a few seconds; nothing is larger than about 700 voxels."""
import ctypes as C
import math
import warnings

import numpy as np
import pytest

import boot_cases as BC

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
EPS = 2.0 ** -52
STATS = ("mean", "bias", "std", "ci_lo", "ci_hi")
PARAMS = ("t2", "k")
GUARD = 64  # words of sentinel on both sides of a guarded payload: (1 + GUARD) * 4 bytes = 4 past a 256-byte boundary
SENTINEL = -0x12345678
EDGE_VOXELS = 131  # the cut of the case the R-edge tests run on


@pytest.fixture(scope="module")
def t2():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X")
    import fetal_t2mapping_amd as t2

    return t2


def _case(n_vox=None):
    """(t2, k, s) of the crafted case: the volume, or its first n_vox voxels as a (1, 1, n_vox) volume (the bootstrap
    numbers voxels from 0, so a leading cut has the samples of the whole)."""
    t2v, k, s, _ = BC.maps()
    if n_vox is None:
        return t2v, k, s
    return tuple(a.reshape(-1)[:n_vox].reshape(1, 1, n_vox).copy() for a in (t2v, k, s))


def _boot(t2, mask=None, R=BC.R, n_vox=None, tensors=False, table=BC.TABLE, **kw):
    import torch

    t2v, k, s = _case(n_vox)
    if tensors:
        t2v, k, s = (torch.from_numpy(a).cuda() for a in (t2v, k, s))
    return t2.bootstrap_volume(None, mask, BC.TE, "gaussian", table, n_replicas=R, seed=BC.SEED, noise_sigma=s, noise="gaussian",
                               solver="loglin", params=PARAMS, maps=t2.T2Maps(t2v, k, None, None), **kw)


def _flat(boot):
    """{(param, stat): flat array} and n_ok of a BootMaps, on the host."""
    host = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else a  # noqa: E731
    out = {}
    for p in PARAMS:
        for name in STATS:
            a = getattr(getattr(boot, p), name)
            if a is not None:
                out[p, name] = host(a).reshape(-1)
    return out, host(boot.n_ok).reshape(-1)


_loops = {}


def _loop(t2, R, n_vox=None, table=BC.TABLE):
    """The loop written with the public pieces: (ok (R, n) bool, {param: (R, n) float32 refits}).  Replica r depends on
    r alone, so the longest loop asked of a cut is computed once and its leading replicas serve the shorter ones."""
    import torch

    which = (n_vox, table is BC.TABLE)
    have = _loops.get(which)
    if have is None or have[0].shape[0] < R:
        t2v, k, s = (torch.from_numpy(a).cuda() for a in _case(n_vox))
        m = torch.ones(t2v.shape, dtype=torch.uint8, device="cuda")
        ok, vals = [], {p: [] for p in PARAMS}
        for r in range(R):
            rep = t2.synth_replica(t2v, k, BC.TE, s, m, seed=BC.SEED, replica=r, noise="gaussian")
            f = t2.fit_volume(rep, m, BC.TE, "gaussian", table, solver="loglin", extras=True)
            ok.append(((f.status == 1) & torch.isfinite(f.t2) & torch.isfinite(f.k)).reshape(-1).cpu().numpy())
            for p in PARAMS:
                vals[p].append(getattr(f, p).reshape(-1).cpu().numpy())
        have = _loops[which] = (np.stack(ok), {p: np.stack(v) for p, v in vals.items()})
    return have[0][:R], {p: v[:R] for p, v in have[1].items()}


def _same(got, want64):
    """got equals float32(want) where want is not finite: NaN where NaN, the same infinity where infinite."""
    return np.array_equal(got.astype(np.float64), want64.astype(np.float32).astype(np.float64), equal_nan=True)


def _check_stats(got, n_ok, ok, x32, centre32, alpha, worst, groups):
    """One parameter's maps against numpy in float64 on the loop's refits.  ``got``: {stat: flat array} (ci_* absent
    without an interval).  Updates ``worst`` (largest error / bar per statistic) and ``groups`` (voxels per group)."""
    n = ok.sum(axis=0)
    assert np.array_equal(n_ok, n)
    interval = "ci_lo" in got
    x = np.where(ok, x32.astype(np.float64), np.nan)
    c = centre32.astype(np.float64)
    shift = np.where(np.isfinite(c), c, 0.0)
    with warnings.catch_warnings(), np.errstate(invalid="ignore", divide="ignore"):
        warnings.simplefilter("ignore")
        mean = np.nanmean(x, axis=0)
        std = np.nanstd(x, axis=0, ddof=1)
        lo, hi = np.nanquantile(x, [alpha / 2.0, 1.0 - alpha / 2.0], axis=0) if interval else (None, None)
        biggest = np.nanmax(np.abs(x), axis=0)
        smallest_v, biggest_v = np.nanmin(x, axis=0), np.nanmax(x, axis=0)
        ssq = np.nansum((x - shift) ** 2, axis=0)

    def ratio(name, sel, want, bar):
        err = np.abs(got[name][sel].astype(np.float64) - want[sel])
        r = err / bar[sel]
        assert np.all(err <= bar[sel]), (name, float(r.max()), int(np.argmax(r)))
        if r.size:
            worst[name] = max(worst.get(name, 0.0), float(r.max()))

    # n = 0: nothing to reduce
    g0 = n == 0
    for name in got:
        assert np.all(np.isnan(got[name][g0])), name
    # n = 1: the value itself, no spread
    g1 = n == 1
    one32 = np.nansum(x[:, g1], axis=0).astype(np.float32)
    assert np.all(np.isnan(got["std"][g1]))
    if interval:
        assert np.array_equal(got["ci_lo"][g1], one32) and np.array_equal(got["ci_hi"][g1], one32)
    # n >= 1: mean and bias; n >= 2: std and the percentiles
    g = n >= 1
    g2 = n >= 2
    tiny = 1e-30
    ratio("mean", g, mean, ULP * np.abs(mean) + tiny)
    fin = g & np.isfinite(c)
    ratio("bias", fin, mean - c, ULP * np.abs(mean - c) + (n + 3) * EPS * (biggest + np.abs(c)) + tiny)
    with np.errstate(invalid="ignore"):
        assert _same(got["bias"][g & ~np.isfinite(c)], (mean - c)[g & ~np.isfinite(c)])
    equal = g2 & (smallest_v == biggest_v)
    spread = g2 & ~equal
    with np.errstate(invalid="ignore", divide="ignore"):
        e = 2.0 * (n + 3) * EPS * ssq / np.maximum(n - 1, 1)
        ratio("std", spread, std, ULP * std + e / (2.0 * std) + tiny)
    assert np.all(got["std"][equal] == 0.0) and np.array_equal(got["mean"][equal], smallest_v[equal].astype(np.float32))
    if interval:
        ratio("ci_lo", g2, lo, ULP * np.abs(lo) + tiny)
        ratio("ci_hi", g2, hi, ULP * np.abs(hi) + tiny)
        assert np.array_equal(got["ci_lo"][equal], got["mean"][equal]) and np.array_equal(got["ci_hi"][equal], got["mean"][equal])
        assert np.all(got["ci_lo"][g] <= got["ci_hi"][g])
    for name, sel in (("n=0", g0), ("n=1", g1), ("n>=2", g2), ("all equal", equal), ("centre not finite", g2 & ~np.isfinite(c))):
        groups[name] = groups.get(name, 0) + int(sel.sum())


# ---- 1. counts ------------------------------------------------------------------------------------------------------
def test_n_ok_equals_the_cpu_prediction_and_the_python_loop(t2):
    _, counted, near, _ = BC.predict()
    want = counted.sum(axis=0)
    _, n_ok = _flat(_boot(t2))
    hist = np.bincount(n_ok, minlength=BC.R + 1)
    print(f"n_ok histogram 0..{BC.R}: {hist.tolist()}; left out of the prediction: {int(near.sum())} of {BC.N} voxels "
          f"({100.0 * near.mean():.2f} %)")
    assert near.mean() <= 0.01 and np.array_equal(n_ok[~near], want[~near])
    assert np.all(hist > 0)  # every count 0..R has run through the reduction
    ok, _ = _loop(t2, BC.R)
    assert np.array_equal(n_ok, ok.sum(axis=0))
    # with a mask: the same counts inside, 0 outside
    mask = BC.masks_with((257,))[0]
    _, masked = _flat(_boot(t2, mask=mask))
    assert np.array_equal(masked, np.where(mask.reshape(-1) != 0, n_ok, 0)) and (mask == 0).sum() > 0


def test_a_converged_refit_that_is_not_finite_does_not_count(t2):
    """Without an upper T2 bound a flat or rising replica converges to T2 = +inf: status CONVERGED, value not finite.
    It must not count, and the statistics are those of the replicas that do."""
    counted, near = BC.predict_open_t2()
    boot = _boot(t2, table=BC.TABLE_OPEN_T2)
    got, n_ok = _flat(boot)
    ok, vals = _loop(t2, BC.R, table=BC.TABLE_OPEN_T2)
    dropped = int((np.isinf(vals["t2"]) & BC.predict()[1]).sum())
    print(f"open T2 bound: {dropped} converged refits of +inf; left out of the prediction: {int(near.sum())} of {BC.N} voxels")
    assert dropped > 1000 and near.mean() <= 0.01
    assert np.array_equal(n_ok[~near], counted.sum(axis=0)[~near]) and np.array_equal(n_ok, ok.sum(axis=0))
    t2v, k, _ = _case()
    for p, centre in (("t2", t2v), ("k", k)):
        worst, groups = {}, {}
        _check_stats({name: got[p, name] for name in STATS}, n_ok, ok, vals[p], centre.reshape(-1), 0.05, worst, groups)
        assert groups["n>=2"] > 0 and np.all(np.isfinite(got[p, "mean"][n_ok >= 1]))


# ---- 2. statistics against numpy in float64 on the loop's refits ----------------------------------------------------------
@pytest.mark.parametrize("alpha", [0.05, 0.5, 0.2, 1e-12, 1.0 - 1e-12])
def test_statistics_equal_numpy_on_the_loops_refits(t2, alpha):
    """alpha = 0.5 makes q (n - 1) an integer for n = 5, 9, 13; 1 - 1e-12 puts q_lo and q_hi either side of t = 0.5;
    1e-12 gives min and max.  Measured on an MI355X: see DESIGN 8b, "Edges"."""
    ok, vals = _loop(t2, BC.R)
    got, n_ok = _flat(_boot(t2, alpha=alpha))
    t2v, k, _ = _case()
    centre = {"t2": t2v.reshape(-1), "k": k.reshape(-1)}
    for p in PARAMS:
        worst, groups = {}, {}
        _check_stats({name: got[p, name] for name in STATS}, n_ok, ok, vals[p], centre[p], alpha, worst, groups)
        print(f"alpha {alpha!r} {p}: worst error / bar " + ", ".join(f"{s} {worst.get(s, 0.0):.3f}" for s in STATS) +
              f"; voxels per group {groups}")
        assert all(groups[name] > 0 for name in ("n=0", "n=1", "n>=2", "all equal")), groups
        if p == "t2":  # the centre of +inf: finite mean and std of the counted refits (include/t2fit.h)
            assert groups["centre not finite"] > 0
            inf_c = np.isposinf(centre[p]) & (n_ok >= 2)
            assert inf_c.sum() >= 5 and np.all(np.isfinite(got[p, "mean"][inf_c])) and np.all(np.isfinite(got[p, "std"][inf_c]))
            assert np.all(np.isneginf(got[p, "bias"][inf_c])) and np.any(got[p, "std"][inf_c] > 0.0)


# ---- 3. R at its edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,interval,alpha", [(2, True, 0.05), (1, False, 0.05), (3, False, 0.05), (256, True, 0.1), (257, True, 0.1)])
def test_replica_counts_at_their_edges(t2, R, interval, alpha):
    """R = 2 is the least an interval takes, R = 1 the least at all; R = 256 is the last launch inside 64 KiB of dynamic
    LDS and R = 257 the first that has to ask for more."""
    ok, vals = _loop(t2, R, EDGE_VOXELS)
    boot = _boot(t2, R=R, n_vox=EDGE_VOXELS, interval=interval, alpha=alpha)
    got, n_ok = _flat(boot)
    t2v, k, _ = _case(EDGE_VOXELS)
    centre = {"t2": t2v.reshape(-1), "k": k.reshape(-1)}
    for p in PARAMS:
        stats = {name: got[p, name] for name in STATS if (p, name) in got}
        assert ("ci_lo" in stats) == interval and (getattr(boot, p).ci_lo is None) == (not interval)
        worst, groups = {}, {}
        _check_stats(stats, n_ok, ok, vals[p], centre[p], alpha, worst, groups)
        print(f"R {R} {p}: worst error / bar {worst}; voxels per group {groups}")
        if R == 1:
            assert np.all(np.isnan(got[p, "std"])) and groups["n=1"] > 0 and groups["n>=2"] == 0
        else:
            assert groups["n>=2"] > 0 and groups["n=0"] > 0


# ---- 4. mask counts ---------------------------------------------------------------------------------------------------
def test_mask_counts_around_the_block_sizes(t2):
    """0, 1, 63, 64, 65, 255, 256, 257 masked voxels: the finalisation works in groups of 64, the accumulation in groups
    of 256.  A sample does not depend on the mask, so each call equals the rows of the full-mask call bit for bit."""
    R = 4
    full, full_n = _flat(_boot(t2, R=R))
    for count, mask in zip((0, 1, 63, 64, 65, 255, 256, 257), BC.masks_with()):
        inside = mask.reshape(-1) != 0
        assert int(inside.sum()) == count
        got, n_ok = _flat(_boot(t2, mask=mask, R=R))
        assert np.array_equal(n_ok, np.where(inside, full_n, 0)), count
        for key, a in got.items():
            assert a[inside].tobytes() == full[key][inside].tobytes(), (count, key)
            assert not a[~inside].any() and a[~inside].tobytes() == bytes(4 * int((~inside).sum())), (count, key)


# ---- 5. determinism on the crafted case -----------------------------------------------------------------------------------
def _raw_boot(lib, cfg, t2_p, k_p, s_p, m_p, n, R, alpha, out_ptr, ctx=None, stream=None, n_ok_p=None):
    """t2fit_bootstrap_dev in interval mode on t2 and k; out_ptr(param index, stat) gives each output pointer."""
    from fetal_t2mapping_amd import _abi

    bm = _abi.T2FitBootMaps()
    for i in range(len(PARAMS)):
        for name in STATS:
            getattr(bm, name)[i] = out_ptr(i, name)
    bm.n_ok = n_ok_p
    rc = lib.t2fit_bootstrap_dev(ctx, C.byref(cfg), t2_p, k_p, None, 0.0, s_p, _abi.BOOT_NOISES["gaussian"], m_p, n, R, BC.SEED,
                                 alpha, 3, C.byref(bm), 0, stream)
    assert rc == _abi.OK, lib.t2fit_last_error().decode()


def test_the_crafted_case_is_deterministic(t2, monkeypatch):
    import torch

    from fetal_t2mapping_amd import _abi
    from fetal_t2mapping_amd._lib import load

    a, a_n = _flat(_boot(t2))
    b, b_n = _flat(_boot(t2))
    monkeypatch.setenv("T2FIT_BOOT_STREAMS", "1")
    c, c_n = _flat(_boot(t2))
    monkeypatch.delenv("T2FIT_BOOT_STREAMS")
    d, d_n = _flat(_boot(t2, tensors=True))
    # through a context's streams, raw
    lib = load()
    cfg = t2.make_config("gaussian", BC.TABLE, BC.TE, solver="loglin")
    dev = [torch.from_numpy(x.reshape(-1)).cuda() for x in _case()]
    m = torch.ones(BC.N, dtype=torch.uint8, device="cuda")
    outs = {(i, name): torch.full((BC.N,), -7.0, dtype=torch.float32, device="cuda") for i in range(2) for name in STATS}
    n_ok = torch.full((BC.N,), -7, dtype=torch.int32, device="cuda")
    ctx = C.c_void_p()
    assert lib.t2fit_create(0, C.byref(ctx)) == _abi.OK
    _raw_boot(lib, cfg, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), m.data_ptr(), BC.N, BC.R, 0.05,
              lambda i, name: outs[i, name].data_ptr(), ctx=ctx, n_ok_p=n_ok.data_ptr())
    assert lib.t2fit_destroy(ctx) == _abi.OK
    e = {(PARAMS[i], name): t.cpu().numpy() for (i, name), t in outs.items()}
    for key, x in a.items():
        for other in (b, c, d, e):
            assert x.tobytes() == other[key].tobytes(), key
    for other in (b_n, c_n, d_n, n_ok.cpu().numpy()):
        assert np.array_equal(a_n, other)


# ---- 6. the counters of the synthesis -------------------------------------------------------------------------------------
def _synth_maps(n, seed=3):
    rng = np.random.default_rng(seed)
    return (rng.uniform(150.0, 400.0, n).astype(np.float32), rng.uniform(500.0, 2000.0, n).astype(np.float32),
            rng.uniform(5.0, 40.0, n).astype(np.float32))


def _units(got, want, s):
    """Largest distance of the samples from their float64 statement in units of 2^-23 (|y| + 6 s)."""
    err = np.abs(got.astype(np.float64) - want)
    unit = ULP * (np.abs(want) + 6.0 * np.asarray(s, np.float64))
    exact = (unit == 0.0) & (err == 0.0)  # a sample of exactly 0 without noise: nothing to be off by
    return float(np.max(np.where(exact, 0.0, err / np.where(unit == 0.0, 1e-300, unit)), initial=0.0))


@pytest.mark.parametrize("noise", ["rician", "gaussian"])
def test_voxel_offset_carries_into_the_high_word_of_the_counter(t2, noise):
    from fetal_t2mapping_amd import _philox

    off = 2 ** 32 - 8
    t2v, k, s = _synth_maps(16)
    kw = dict(seed=1234567890123, replica=3, noise=noise)
    worst = 0.0
    outs = {}
    for n in (16, 15):  # four voxels per lane / one voxel per lane
        got = t2.synth_replica(t2v[:n], k[:n], BC.TE, s[:n], None, voxel_offset=off, **kw).cpu().numpy()
        want = _philox.replica(t2v[:n], k[:n], BC.TE, s[:n], None, voxel_offset=off, **kw)
        worst = max(worst, _units(got, want, s[:n]))
        outs[n] = got
    assert worst <= 4.0
    assert outs[16][:, :15].tobytes() == outs[15].tobytes()
    for n in (8, 7):  # voxels 2^32.. of the straddling call are the first of a call at offset 2^32, on either path
        beyond = t2.synth_replica(t2v[8:8 + n], k[8:8 + n], BC.TE, s[8:8 + n], None, voxel_offset=2 ** 32, **kw).cpu().numpy()
        assert beyond.tobytes() == np.ascontiguousarray(outs[16][:, 8:8 + n]).tobytes()
        low = t2.synth_replica(t2v[8:8 + n], k[8:8 + n], BC.TE, s[8:8 + n], None, voxel_offset=0, **kw).cpu().numpy()
        assert np.all(low != beyond)  # a kernel that dropped the high word would make them equal
    # the largest replica index, and a seed with only its high word set
    far = dict(seed=0xABCD << 32, replica=2 ** 31 - 1, noise=noise)
    for n in (16, 15):
        got = t2.synth_replica(t2v[:n], k[:n], BC.TE, s[:n], None, voxel_offset=off, **far).cpu().numpy()
        worst = max(worst, _units(got, _philox.replica(t2v[:n], k[:n], BC.TE, s[:n], None, voxel_offset=off, **far), s[:n]))
        assert np.all(got != t2.synth_replica(t2v[:n], k[:n], BC.TE, s[:n], None, voxel_offset=off, seed=0, replica=2 ** 31 - 1,
                                              noise=noise).cpu().numpy())
    print(f"synthesis across 2^32 [{noise}]: worst error {worst:.2f} units of 2^-23 (|y| + 6 s)")
    assert worst <= 4.0


# ---- 7. the operands of the synthesis -------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["rician", "gaussian"])
def test_synthesis_operands_at_their_edges(t2, noise):
    """An odd voxel inside a four-voxel group: NaN goes where the statement has NaN, everything else stays within the 4
    units, and the other voxels keep their bits.  k exp(-TE / T2) stays inside [1e-15, 1e15]: the Rician magnitude is
    sqrtf(a^2 + b^2), whose range is not this test's subject."""
    import torch

    from fetal_t2mapping_amd import _abi, _philox
    from fetal_t2mapping_amd._lib import load

    kw = dict(seed=99, replica=5, noise=noise)
    worst = 0.0
    odd_at = 5
    cases = [("t2", 0.0), ("t2", np.inf), ("t2", np.nan), ("t2", -50.0), ("k", 0.0), ("k", np.nan)]
    for te in (BC.TE, [10.0 * (j + 1) for j in range(32)]):  # 2 echoes (1 is refused, below) and the most, 32
        for n in (16, 15):
            for zero_noise in (False, True):
                t2v, k, s = _synth_maps(n)
                if zero_noise:
                    s[:] = 0.0
                plain = t2.synth_replica(t2v, k, te, s, None, **kw).cpu().numpy()
                want = _philox.replica(t2v, k, te, s, None, **kw)
                assert plain.shape == (len(te), n)
                worst = max(worst, _units(plain, want, s))
                for which, value in cases:
                    a, b = t2v.copy(), k.copy()
                    (a if which == "t2" else b)[odd_at] = value
                    got = t2.synth_replica(a, b, te, s, None, **kw).cpu().numpy()
                    want = _philox.replica(a, b, te, s, None, **kw)
                    nan = np.isnan(want)
                    assert np.array_equal(np.isnan(got), nan), (which, value)
                    assert nan[:, odd_at].all() == bool(np.isnan(value)) and not np.delete(nan, odd_at, axis=1).any()
                    worst = max(worst, _units(got[~nan], want[~nan], np.broadcast_to(s, got.shape)[~nan]))
                    others = np.arange(n) != odd_at
                    assert got[:, others].tobytes() == plain[:, others].tobytes(), (which, value)
                    if zero_noise and value == 0.0:
                        assert np.all(got[:, odd_at] == 0.0)  # S = 0 exactly
                    if which == "t2" and value == np.inf and zero_noise:
                        assert np.all(got[:, odd_at] == k[odd_at])  # S = k exactly
    print(f"synthesis operands [{noise}]: worst error {worst:.2f} units of 2^-23 (|y| + 6 s)")
    assert worst <= 4.0
    with pytest.raises(ValueError):  # one echo is no decay: refused like every fit configuration
        t2.synth_replica(t2v, k, [114.0], 20.0, None, **kw)
    # raw only: any non-zero mask byte counts as set, on both paths
    lib = load()
    cfg = t2.make_config("gaussian", BC.TABLE, BC.TE)
    for n in (16, 15):
        t2v, k, s = _synth_maps(n)
        dev = [torch.from_numpy(x).cuda() for x in (t2v, k, s)]
        bytes_ = np.array([1, 2, 255, 0, 0, 255, 2, 1, 0, 0, 0, 0, 2, 2, 255, 255][:n], np.uint8)
        res = []
        for mask in (bytes_, (bytes_ != 0).astype(np.uint8)):
            m = torch.from_numpy(mask).cuda()
            out = torch.full((2, n), -7.0, dtype=torch.float32, device="cuda")
            rc = lib.t2fit_boot_synth_dev(C.byref(cfg), dev[0].data_ptr(), dev[1].data_ptr(), 0.0, dev[2].data_ptr(), m.data_ptr(), n, 0,
                                          99, 5, _abi.BOOT_NOISES[noise], out.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == _abi.OK, lib.t2fit_last_error().decode()
            res.append(out.cpu().numpy())
        assert res[0].tobytes() == res[1].tobytes()
        assert np.all(res[0][:, bytes_ == 0] == 0.0) and np.all(res[0][:, bytes_ != 0] != 0.0)
        want = _philox.replica(t2v, k, BC.TE, s, bytes_, **kw)
        assert _units(res[0], want, s) <= 4.0


# ---- 8. pointers and guards -------------------------------------------------------------------------------------------------
def _guarded(words, n_words=None):
    """An int32 device buffer [1 word | GUARD sentinels | payload | GUARD sentinels], all sentinel but the payload when one
    is given: the payload starts 4 bytes past a 256-byte boundary.  Returns ``(buffer, payload pointer, payload slice)``."""
    import torch

    n = len(words) if words is not None else n_words
    buf = torch.full((1 + GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 256 == 0
    where = slice(1 + GUARD, 1 + GUARD + n)
    if words is not None:
        buf[where] = torch.from_numpy(np.ascontiguousarray(words).view(np.int32).ravel()).cuda()
    ptr = buf.data_ptr() + 4 * (1 + GUARD)
    assert ptr % 256 == 4
    return buf, ptr, where


def _payload(buf, where):
    """The payload of a guarded buffer after a call; everything around it must still be the sentinel."""
    host = buf.cpu().numpy()
    assert np.all(host[:where.start] == SENTINEL) and np.all(host[where.stop:] == SENTINEL), "written outside the output"
    return host[where]


def _odd_mask(mask):
    """A uint8 device copy of the mask that starts 1 byte past a 256-byte boundary: (buffer, pointer)."""
    import torch

    buf = torch.zeros(mask.size + 512, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    buf[257:257 + mask.size] = torch.from_numpy(np.ascontiguousarray(mask).ravel()).cuda()
    return buf, buf.data_ptr() + 257


def test_raw_bootstrap_with_unaligned_inputs_and_guarded_outputs(t2):
    import torch

    from fetal_t2mapping_amd._lib import load

    n, R, alpha = 480, 8, 0.1  # a multiple of 4: bootstrap_volume's aligned buffers take the four-voxel synthesis
    mask = (np.arange(n) % 7 != 3).astype(np.uint8).reshape(1, 1, n)
    want, want_n = _flat(_boot(t2, mask=mask, R=R, n_vox=n, alpha=alpha))
    lib = load()
    cfg = t2.make_config("gaussian", BC.TABLE, BC.TE, solver="loglin")
    ins = [_guarded(a.ravel()) for a in _case(n)]
    assert all(p % 16 == 4 for _, p, _ in ins)
    mbuf, m_p = _odd_mask(mask)
    outs = {(i, name): _guarded(None, n) for i in range(2) for name in STATS}
    nbuf = _guarded(None, n)
    _raw_boot(lib, cfg, ins[0][1], ins[1][1], ins[2][1], m_p, n, R, alpha, lambda i, name: outs[i, name][1], n_ok_p=nbuf[1],
              stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for (i, name), (buf, _, where) in outs.items():
        assert _payload(buf, where).tobytes() == want[PARAMS[i], name].tobytes(), (i, name)
    assert np.array_equal(_payload(nbuf[0], nbuf[2]), want_n)
    assert len(outs) == 10


@pytest.mark.parametrize("noise", ["rician", "gaussian"])
def test_raw_synthesis_with_each_pointer_unaligned_in_turn(t2, noise):
    import torch

    from fetal_t2mapping_amd import _abi
    from fetal_t2mapping_amd._lib import load

    lib = load()
    n = 64
    cfg = t2.make_config("gaussian", BC.TABLE, BC.TE)
    t2v, k, s = _synth_maps(n)
    mask = (np.arange(n) % 5 != 2).astype(np.uint8)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(odd):
        keep = []
        ptrs = []
        for name, a in (("t2", t2v), ("k", k), ("noise", s)):
            if name == odd:
                buf, p, _ = _guarded(a)
            else:
                buf = torch.from_numpy(a).cuda()
                p = buf.data_ptr()
                assert p % 16 == 0
            keep.append(buf)
            ptrs.append(p)
        if odd == "mask":
            mb, m_p = _odd_mask(mask)
        else:
            mb = torch.from_numpy(mask).cuda()
            m_p = mb.data_ptr()
        if odd == "out":
            ob, o_p, where = _guarded(None, 2 * n)
        else:
            ob = torch.full((GUARD + 2 * n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
            o_p, where = ob.data_ptr() + 4 * GUARD, slice(GUARD, GUARD + 2 * n)
            assert o_p % 16 == 0
        rc = lib.t2fit_boot_synth_dev(C.byref(cfg), ptrs[0], ptrs[1], 0.0, ptrs[2], m_p, n, 0, 31, 2, _abi.BOOT_NOISES[noise], o_p, stream)
        assert rc == _abi.OK, lib.t2fit_last_error().decode()
        torch.cuda.synchronize()
        del keep, mb
        return _payload(ob, where).tobytes()

    aligned = call(None)
    want = t2.synth_replica(t2v, k, BC.TE, s, mask, seed=31, replica=2, noise=noise).cpu().numpy()
    assert aligned == want.tobytes()
    for odd in ("t2", "k", "noise", "mask", "out"):
        assert call(odd) == aligned, odd


# ---- 9. a caller's stream with the inputs in flight -------------------------------------------------------------------------
def _busy(stream, ms=250.0):
    """Queue about `ms` of device time on `stream`: the spin kernel where torch has one (its rate measured first), a
    chain of large fills otherwise."""
    import torch

    if hasattr(torch.cuda, "_sleep"):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        probe = 2_000_000
        torch.cuda._sleep(probe)  # (first use: loads the kernel)
        torch.cuda.synchronize()
        start.record()
        torch.cuda._sleep(probe)
        stop.record()
        torch.cuda.synchronize()
        per_ms = probe / max(start.elapsed_time(stop), 1e-3)
        with torch.cuda.stream(stream):
            torch.cuda._sleep(int(min(per_ms * ms, 2 ** 62)))
        return None
    big = torch.empty(1 << 28, dtype=torch.float32, device="cuda")  # 1 GiB: about 0.5 ms a fill
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for i in range(int(ms * 2)):
            big.fill_(float(i))
    return big


def test_bootstrap_waits_for_inputs_still_in_flight_on_the_callers_stream(t2):
    import torch

    from fetal_t2mapping_amd._lib import load

    n, R, alpha = 480, 4, 0.1
    mask = (np.arange(n) % 7 != 3).astype(np.uint8).reshape(1, 1, n)
    want, want_n = _flat(_boot(t2, mask=mask, R=R, n_vox=n, alpha=alpha))
    lib = load()
    cfg = t2.make_config("gaussian", BC.TABLE, BC.TE, solver="loglin")
    src = [torch.from_numpy(a.reshape(-1)).cuda() for a in _case(n)] + [torch.from_numpy(mask.reshape(-1)).cuda()]
    dst = [torch.zeros_like(a) for a in src]
    outs = {(i, name): torch.full((n,), -7.0, dtype=torch.float32, device="cuda") for i in range(2) for name in STATS}
    n_ok = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    keep = _busy(side)
    with torch.cuda.stream(side):
        for d, s_ in zip(dst, src):
            d.copy_(s_, non_blocking=True)
    assert not side.query()  # the premise: the copies that fill the inputs have not run yet
    _raw_boot(lib, cfg, dst[0].data_ptr(), dst[1].data_ptr(), dst[2].data_ptr(), dst[3].data_ptr(), n, R, alpha,
              lambda i, name: outs[i, name].data_ptr(), n_ok_p=n_ok.data_ptr(), stream=C.c_void_p(side.cuda_stream))
    torch.cuda.synchronize()
    del keep
    for (i, name), t in outs.items():
        assert t.cpu().numpy().tobytes() == want[PARAMS[i], name].tobytes(), (i, name)
    assert np.array_equal(n_ok.cpu().numpy(), want_n)


def test_synthesis_and_background_level_follow_the_callers_stream(t2):
    import torch

    from fetal_t2mapping_amd import _abi
    from fetal_t2mapping_amd._lib import load

    lib = load()
    n = 480
    cfg = t2.make_config("gaussian", BC.TABLE, BC.TE)
    mask = (np.arange(n) % 7 != 3).astype(np.uint8)
    t2v, k, s = _synth_maps(n)
    want = t2.synth_replica(t2v, k, BC.TE, s, mask, seed=31, replica=2)
    outside = (mask == 0).astype(np.uint8)  # as a background mask: the level of the voxels the synthesis filled
    want_sigma = t2.estimate_background_sigma(want, torch.from_numpy(outside).cuda())
    assert want_sigma[0] > 100.0 and want_sigma[1] == 2 * int(mask.sum())
    src = [torch.from_numpy(a).cuda() for a in (t2v, k, s, mask, outside)]
    dst = [torch.zeros_like(a) for a in src]
    out = torch.full((2, n), -7.0, dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    keep = _busy(side)
    with torch.cuda.stream(side):
        for d, s_ in zip(dst, src):
            d.copy_(s_, non_blocking=True)
    assert not side.query()
    st = C.c_void_p(side.cuda_stream)
    rc = lib.t2fit_boot_synth_dev(C.byref(cfg), dst[0].data_ptr(), dst[1].data_ptr(), 0.0, dst[2].data_ptr(), dst[3].data_ptr(), n, 0, 31, 2,
                                  _abi.BOOT_NOISES["rician"], out.data_ptr(), st)
    assert rc == _abi.OK, lib.t2fit_last_error().decode()
    with torch.cuda.stream(side):
        read = out.clone()  # a read on that stream, no synchronisation in between
    sigma, count = C.c_double(0.0), C.c_int64(0)
    rc = lib.t2fit_boot_background_dev(out.data_ptr(), _abi.LAYOUT_TE_MAJOR, dst[4].data_ptr(), 2, n, C.byref(sigma), C.byref(count), st)
    assert rc == _abi.OK, lib.t2fit_last_error().decode()
    torch.cuda.synchronize()
    del keep
    assert torch.equal(read, want) and torch.equal(out, want)
    assert (sigma.value, count.value) == want_sigma


# ---- 10. the background level at its small end ------------------------------------------------------------------------------
@pytest.mark.parametrize("n_vox", [1, 255, 257])
@pytest.mark.parametrize("layout", ["te_major", "voxel_major"])
def test_background_level_of_a_single_voxel(t2, n_vox, layout):
    n_te = 32
    rng = np.random.default_rng(n_vox)
    echoes = rng.uniform(1.0, 100.0, (n_te, 1, 1, n_vox)).astype(np.float32)
    mask = np.ones((1, 1, n_vox), np.uint8)
    mask[0, 0, -1] = 0  # one background voxel: the last one (for 257, the first of the launch's second sweep)
    x = [float(v) for v in echoes[:, 0, 0, -1]]
    want = math.sqrt(math.fsum(v * v for v in x) / (2.0 * n_te))
    e = echoes if layout == "te_major" else np.ascontiguousarray(np.moveaxis(echoes, 0, -1))
    sigma, count = t2.estimate_background_sigma(e, mask, layout=layout)
    assert count == n_te and abs(sigma / want - 1.0) <= 1e-12
    assert t2.estimate_background_sigma(e, mask, layout=layout) == (sigma, count)
