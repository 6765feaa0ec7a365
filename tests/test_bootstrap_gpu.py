"""The parametric bootstrap on the device (t2fit_boot_synth_dev / t2fit_boot_background_dev / t2fit_bootstrap_dev,
t2map.synth_replica / estimate_background_sigma / bootstrap_volume, --bootstrap): the replica stream against its numpy
restatement (fetal_t2mapping_amd/_philox.py), the noise statistics, the in-library loop against the same loop written
in Python with the public pieces and numpy's moments and percentiles, determinism, and two physical checks -- the
linear-theory standard error t2_se where that theory holds, and a true Monte-Carlo over independent acquisitions."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def t2():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X")
    import fetal_t2mapping_amd as t2

    return t2


def _truth(shape, seed):
    """Maps to draw replicas from: k 700..3000, T2 40..400 with a pocket of 600..2000, an irregular mask."""
    rng = np.random.default_rng(seed)
    k = rng.uniform(700.0, 3000.0, shape).astype(np.float32)
    t2v = rng.uniform(40.0, 400.0, shape).astype(np.float32)
    t2v[shape[0] // 2, : shape[1] // 3] = rng.uniform(600.0, 2000.0, (shape[1] // 3, shape[2])).astype(np.float32)
    mask = (rng.random(shape) < 0.6).astype(np.uint8)
    mask[0] = 0
    mask[-1, :, ::3] = 1
    return t2v, k, mask


# ---- 4. the replica stream ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["rician", "gaussian"])
def test_synth_replica_equals_the_numpy_restatement(t2, noise):
    import torch

    from fetal_t2mapping_amd import _philox

    shape = (24, 40, 56)
    t2v, k, mask = _truth(shape, 5)
    te = [114.0, 151.5, 188.0, 225.0, 262.5, 299.0]
    sigma = 20.0
    got = t2.synth_replica(t2v, k, te, sigma, mask, seed=1234567890123, replica=3, noise=noise)
    assert got.shape == (6,) + shape and got.dtype == torch.float32 and got.is_cuda
    got = got.cpu().numpy()
    want = _philox.replica(t2v, k, te, sigma, mask, seed=1234567890123, replica=3, noise=noise)
    assert np.all(got[:, mask == 0] == 0.0)
    # measured on an MI355X: the worst sample is 2.04 (rician) / 1.97 (gaussian) of these units off (float32 exp, log,
    # sincospi against float64); a wrong counter layout would show as errors of the order of sigma, 1e6 of these units
    unit = ULP * (np.abs(want) + 6.0 * sigma)
    worst = float(np.max(np.abs(got - want) / unit))
    print(f"synth_replica[{noise}]: worst error {worst:.2f} units of 2^-23 (|sample| + 6 sigma)")
    assert worst <= 4.0
    # a per-voxel noise map, and an unaligned / odd-sized volume through the one-voxel-per-lane kernel
    smap = np.random.default_rng(6).uniform(5.0, 40.0, shape).astype(np.float32)
    got = t2.synth_replica(t2v, k, te, smap, mask, seed=9, replica=0, noise=noise).cpu().numpy()
    want = _philox.replica(t2v, k, te, smap, mask, seed=9, replica=0, noise=noise)
    assert float(np.max(np.abs(got - want) / (ULP * (np.abs(want) + 6.0 * smap)))) <= 4.0
    odd = (3, 5, 7)
    o_t2, o_k, o_mask = _truth(odd, 8)
    got = t2.synth_replica(o_t2, o_k, te, sigma, o_mask, seed=9, replica=1, noise=noise).cpu().numpy()
    want = _philox.replica(o_t2, o_k, te, sigma, o_mask, seed=9, replica=1, noise=noise)
    assert float(np.max(np.abs(got - want) / (ULP * (np.abs(want) + 6.0 * sigma)))) <= 4.0


def test_synth_replica_depends_on_seed_voxel_echo_replica_alone(t2):
    import torch

    shape = (24, 40, 56)
    t2v, k, mask = _truth(shape, 5)
    te = [114.0, 202.0, 299.0]
    kw = dict(seed=77, replica=2)
    a = t2.synth_replica(t2v, k, te, 20.0, mask, **kw)
    assert torch.equal(a, t2.synth_replica(t2v, k, te, 20.0, mask, **kw))
    assert not torch.equal(a, t2.synth_replica(t2v, k, te, 20.0, mask, seed=78, replica=2))
    assert not torch.equal(a, t2.synth_replica(t2v, k, te, 20.0, mask, seed=77, replica=3))
    assert not torch.equal(a, t2.synth_replica(t2v, k, te, 20.0, mask, seed=77 + 2 ** 32, replica=2))
    # not on the mask: the voxels two masks share are equal
    full = t2.synth_replica(t2v, k, te, 20.0, None, **kw)
    m = torch.from_numpy(mask).to(a.device) != 0
    assert torch.equal(a[:, m], full[:, m])
    # not on the partition: a slab with its flat offset is the same rows of the whole volume, bit for bit -- through
    # the four-voxel kernel (offset a multiple of four) and through the one-voxel kernel (a slab of odd size)
    z0, z1 = 7, 15
    slab = t2.synth_replica(t2v[z0:z1], k[z0:z1], te, 20.0, mask[z0:z1], voxel_offset=z0 * 40 * 56, **kw)
    assert torch.equal(slab, a[:, z0:z1])
    flat = lambda x: x.reshape(-1)[1001:2000].reshape(1, 1, -1)  # noqa: E731
    piece = t2.synth_replica(flat(t2v), flat(k), te, 20.0, flat(mask), voxel_offset=1001, **kw)
    assert torch.equal(piece.reshape(3, -1), a.reshape(3, -1)[:, 1001:2000])


# ---- 5. noise statistics ------------------------------------------------------------------------------------------
def test_noise_statistics_and_independence(t2):
    shape = (64, 128, 128)  # 1.05 M voxels
    sigma = 20.0
    te = [114.0, 202.0, 299.0]
    ones = np.ones(shape, np.float32)
    # S = 0: Rayleigh
    zero = t2.synth_replica(ones * 100.0, ones * 0.0, te, sigma, None, seed=3, replica=0).double()
    mean, second = float(zero[0].mean()), float((zero[0] ** 2).mean())
    assert abs(mean / (sigma * np.sqrt(np.pi / 2)) - 1.0) < 0.01 and abs(second / (2 * sigma ** 2) - 1.0) < 0.01
    # S = 50 sigma at every echo (T2 enormous): mean S + sigma^2 / 2S, std sigma
    S = 50.0 * sigma
    big = t2.synth_replica(ones * 1e9, ones * S, te, sigma, None, seed=3, replica=0).double()
    assert abs(float(big[1].mean()) - (S + sigma ** 2 / (2 * S))) < 0.01 * sigma and abs(float(big[1].std()) / sigma - 1.0) < 0.01
    gauss = t2.synth_replica(ones * 1e9, ones * S, te, sigma, None, seed=3, replica=0, noise="gaussian").double()
    assert abs(float(gauss[2].mean()) - S) < 0.01 * sigma and abs(float(gauss[2].std()) / sigma - 1.0) < 0.01
    # kurtosis of a normal: 3
    z = (gauss[0] - S) / sigma
    assert abs(float((z ** 4).mean()) - 3.0) < 0.05
    # independence: between echoes, between neighbouring voxels (x, y, z), between replicas, between seeds
    other = t2.synth_replica(ones * 1e9, ones * S, te, sigma, None, seed=3, replica=1, noise="gaussian").double()
    seed4 = t2.synth_replica(ones * 1e9, ones * S, te, sigma, None, seed=4, replica=0, noise="gaussian").double()

    def rho(a, b):
        a, b = a.reshape(-1) - a.mean(), b.reshape(-1) - b.mean()
        return abs(float((a * b).mean() / (a.std() * b.std())))

    pairs = {"echo 0/1": (gauss[0], gauss[1]), "echo 1/2": (gauss[1], gauss[2]), "x": (gauss[0][:, :, 1:], gauss[0][:, :, :-1]),
             "y": (gauss[0][:, 1:], gauss[0][:, :-1]), "z": (gauss[0][1:], gauss[0][:-1]), "replica": (gauss[0], other[0]),
             "seed": (gauss[0], seed4[0]), "rician echoes": (big[0], big[2])}
    for name, (a, b) in pairs.items():
        assert rho(a, b) < 0.01, name


# ---- 6. the pin: the in-library loop is the composition it claims to be ---------------------------------------------
def _close_f32(got, want64, scale=None, ulps=1.0):
    """|got - float32(want)| within `ulps` float32 ulp of max(|want|, scale)."""
    ref = np.abs(want64) if scale is None else np.maximum(np.abs(want64), scale)
    return np.abs(got.astype(np.float64) - want64) <= ulps * ULP * ref + 1e-30


@pytest.mark.parametrize("fit,solver,precision", [("gaussian", "lbfgsb", "f64"), ("gaussian_rician", "lbfgsb", "f64"),
                                                  ("gaussian", "lm", "f32")])
def test_bootstrap_volume_equals_the_python_loop_and_numpy(t2, fit, solver, precision):
    import torch

    from fetal_t2mapping_amd import synth

    R, sigma, seed = 16, 20.0, 5
    echoes, mask, te = synth.brain_volume((32, 48, 64), 6, seed=synth.SEED_BASE + 1, low_field=True)
    table = t2.fit_table(fit, True)
    e = torch.from_numpy(echoes).cuda()
    m = torch.from_numpy(mask).cuda()
    params = ("t2", "k") if fit == "gaussian" else ("t2", "k", "sigma")
    boot = t2.bootstrap_volume(e, m, te, fit, table, n_replicas=R, seed=seed, noise_sigma=sigma, params=params, solver=solver,
                               precision=precision)
    base = boot.fit
    again = t2.fit_volume(e, m, te, fit, table, solver=solver, precision=precision, extras=True)
    for name in ("t2", "k", "sigma", "res", "status"):  # the fit the replicas are drawn from is the ordinary one
        assert torch.equal(getattr(base, name), getattr(again, name)), name
    stack = {p: [] for p in params}
    ok = []
    for r in range(R):
        rep = t2.synth_replica(base.t2, base.k, te, sigma, m, seed=seed, replica=r)
        f = t2.fit_volume(rep, m, te, fit, table, solver=solver, precision=precision, extras=True)
        good = f.status == 1
        for p in params:
            good = good & torch.isfinite(getattr(f, p))
        ok.append(good.cpu().numpy())
        for p in params:
            stack[p].append(getattr(f, p).double().cpu().numpy())
    ok = np.stack(ok)
    inside = mask != 0
    n_ok = ok.sum(axis=0)
    assert np.array_equal(boot.n_ok.cpu().numpy(), np.where(inside, n_ok, 0))
    assert n_ok[inside].min() >= 0 and np.median(n_ok[inside]) >= R - 2
    sel = inside & (n_ok >= 2)
    assert sel.sum() > 0.9 * inside.sum()
    for p in params:
        x = np.where(ok, np.stack(stack[p]), np.nan)[:, sel]
        centre = getattr(base, p).double().cpu().numpy()[sel]
        s = getattr(boot, p)
        got = {name: getattr(s, name).cpu().numpy() for name in ("mean", "bias", "std", "ci_lo", "ci_hi")}
        for name, a in got.items():
            assert np.all(a[~inside] == 0.0), (p, name)
        mean = np.nanmean(x, axis=0)
        std = np.nanstd(x, axis=0, ddof=1)
        lo, hi = np.nanpercentile(x, [2.5, 97.5], axis=0)
        scale = np.abs(centre)
        assert np.all(_close_f32(got["mean"][sel], mean)), p
        assert np.all(_close_f32(got["ci_lo"][sel], lo)) and np.all(_close_f32(got["ci_hi"][sel], hi)), p
        # bias and std are small differences of values of the parameter's size: one float32 ulp of the statistic where
        # numpy's own float64 rounding noise (1e-13 of the value) is below it, of 1e-6 of the value otherwise
        assert np.all(_close_f32(got["bias"][sel], mean - centre, scale * 1e-6)), p
        assert np.all(_close_f32(got["std"][sel], std, scale * 1e-6)), p
        assert np.all(got["ci_lo"][sel] <= got["ci_hi"][sel]) and np.all(got["std"][sel] >= 0.0)
    # a voxel with fewer than two counted replicas has NaN std; without any, NaN everywhere
    few = inside & (n_ok < 2)
    if few.any():
        assert np.all(np.isnan(boot.t2.std.cpu().numpy()[few]))
    none = inside & (n_ok == 0)
    if none.any():
        assert np.all(np.isnan(boot.t2.mean.cpu().numpy()[none])) and np.all(np.isnan(boot.t2.ci_lo.cpu().numpy()[none]))


def test_bootstrap_volume_with_a_noise_map_equals_the_python_loop(t2):
    """noise_sigma as a per-voxel map, numpy and tensor, with the default params and with maps given (echoes=None):
    the same maps from both, equal to the loop written with synth_replica + fit_volume on that map."""
    import torch

    from fetal_t2mapping_amd import synth

    R, seed = 8, 21
    echoes, mask, te = synth.brain_volume((6, 24, 32), 6, seed=synth.SEED_BASE + 6, low_field=True)
    table = t2.fit_table("gaussian", True)
    smap = np.random.default_rng(7).uniform(10.0, 30.0, mask.shape).astype(np.float32)
    a = t2.bootstrap_volume(echoes, mask, te, "gaussian", table, n_replicas=R, seed=seed, noise_sigma=smap, solver="lm")
    assert a.noise_sigma is None and isinstance(a.boot_std, np.ndarray)
    e, m, sm = torch.from_numpy(echoes).cuda(), torch.from_numpy(mask).cuda(), torch.from_numpy(smap).cuda()
    b = t2.bootstrap_volume(e, m, te, "gaussian", table, n_replicas=R, seed=seed, noise_sigma=sm, solver="lm")
    c = t2.bootstrap_volume(None, mask, te, "gaussian", table, n_replicas=R, seed=seed, noise_sigma=smap, solver="lm", maps=a.fit)
    vals, ok = [], []
    for r in range(R):
        f = t2.fit_volume(t2.synth_replica(b.fit.t2, b.fit.k, te, sm, m, seed=seed, replica=r), m, te, "gaussian", table,
                          solver="lm", extras=True)
        vals.append(f.t2.double().cpu().numpy())
        ok.append(((f.status == 1) & torch.isfinite(f.t2)).cpu().numpy())
    ok = np.stack(ok)
    x = np.where(ok, np.stack(vals), np.nan)
    sel = (mask != 0) & (ok.sum(axis=0) >= 2)
    assert sel.sum() > 0.9 * (mask != 0).sum() and np.array_equal(a.n_ok[sel], ok.sum(axis=0)[sel])
    lo, hi = np.nanpercentile(x[:, sel], [2.5, 97.5], axis=0)
    assert np.all(_close_f32(a.boot_mean[sel], np.nanmean(x[:, sel], axis=0)))
    assert np.all(_close_f32(a.ci_lo[sel], lo)) and np.all(_close_f32(a.ci_hi[sel], hi))
    for name in ("mean", "bias", "std", "ci_lo", "ci_hi"):
        assert getattr(a.t2, name).tobytes() == getattr(b.t2, name).cpu().numpy().tobytes() == getattr(c.t2, name).tobytes(), name
    # a larger noise level gives a larger spread: the map is what the replicas are drawn with
    d = t2.bootstrap_volume(None, mask, te, "gaussian", table, n_replicas=R, seed=seed, noise_sigma=3.0 * smap, solver="lm", maps=a.fit)
    assert np.nanmedian(d.boot_std[sel] / a.boot_std[sel]) > 2.0
    with pytest.raises(ValueError):
        t2.bootstrap_volume(None, mask, te, "gaussian", table, noise_sigma="background", maps=a.fit)
    with pytest.raises(ValueError):
        t2.bootstrap_volume(echoes, mask, te, "gaussian", table, noise_sigma=smap[:, :-1], solver="lm")


# ---- 7. determinism -------------------------------------------------------------------------------------------------
def test_two_calls_are_byte_identical_and_moments_do_not_depend_on_the_interval(t2, monkeypatch):
    from fetal_t2mapping_amd import synth

    echoes, mask, te = synth.brain_volume((12, 40, 48), 6, seed=synth.SEED_BASE + 2, low_field=True)
    table = t2.fit_table("gaussian_rician", True)
    kw = dict(n_replicas=12, seed=99, params=("t2", "sigma"), noise_sigma="background")
    a = t2.bootstrap_volume(echoes, mask, te, "gaussian_rician", table, **kw)
    b = t2.bootstrap_volume(echoes, mask, te, "gaussian_rician", table, **kw)
    c = t2.bootstrap_volume(echoes, mask, te, "gaussian_rician", table, interval=False, **kw)
    monkeypatch.setenv("T2FIT_BOOT_STREAMS", "1")  # synthesis and fit on one stream: the same bits
    d = t2.bootstrap_volume(echoes, mask, te, "gaussian_rician", table, **kw)
    monkeypatch.delenv("T2FIT_BOOT_STREAMS")
    e = t2.bootstrap_volume(echoes, mask, te, "gaussian_rician", table, maps=a.fit, **kw)
    assert isinstance(a.boot_std, np.ndarray) and a.k is None and a.noise_sigma == b.noise_sigma and 15.0 < a.noise_sigma < 25.0
    for p in ("t2", "sigma"):
        for name in ("mean", "bias", "std", "ci_lo", "ci_hi"):
            x = getattr(getattr(a, p), name)
            assert x.dtype == np.float32 and x.shape == mask.shape
            for other in (b, d, e):
                assert x.tobytes() == getattr(getattr(other, p), name).tobytes(), (p, name)
            if name.startswith("ci"):
                assert getattr(getattr(c, p), name) is None
            else:
                assert x.tobytes() == getattr(getattr(c, p), name).tobytes(), (p, name)
    assert a.n_ok.dtype == np.int32 and np.array_equal(a.n_ok, b.n_ok) and np.array_equal(a.n_ok, c.n_ok)
    assert not np.array_equal(a.boot_std, t2.bootstrap_volume(echoes, mask, te, "gaussian_rician", table, maps=a.fit,
                                                              **dict(kw, seed=100)).boot_std)
    # the fitted sigma map as the noise level; refused where there is none
    f = t2.bootstrap_volume(echoes, mask, te, "gaussian_rician", table, maps=a.fit, **dict(kw, noise_sigma="sigma_map"))
    assert f.noise_sigma is None and np.isfinite(f.boot_std[mask != 0]).mean() > 0.9
    with pytest.raises(ValueError):
        t2.bootstrap_volume(echoes, mask, te, "gaussian", t2.fit_table("gaussian", True), noise_sigma="sigma_map")
    with pytest.raises(ValueError):
        t2.bootstrap_volume(echoes, mask, te, "gaussian", t2.fit_table("gaussian", True), params=("sigma",))
    with pytest.raises(ValueError):
        t2.bootstrap_volume(echoes, mask, te, "gaussian_rician", table, n_replicas=600)
    big = t2.bootstrap_volume(echoes[:, :2], mask[:2], te, "gaussian", t2.fit_table("gaussian", True), n_replicas=600,
                              noise_sigma=20.0, interval=False, solver="loglin")
    assert big.n_ok.max() == 600 and big.ci_lo is None


def test_interval_with_hundreds_of_replicas(t2):
    """R = 300 and the largest R = 512 stage 75 and 128 KiB of values per 64 voxels: more than the 64 KiB a launch gets
    without asking.  Closed-form refits keep it quick; the percentiles are numpy's."""
    import torch

    from fetal_t2mapping_amd import synth

    echoes, mask, te = synth.brain_volume((4, 20, 24), 6, seed=synth.SEED_BASE + 5, low_field=True)
    table = t2.fit_table("gaussian", True)
    e, m = torch.from_numpy(echoes).cuda(), torch.from_numpy(mask).cuda()
    for R in (300, 512):
        boot = t2.bootstrap_volume(e, m, te, "gaussian", table, n_replicas=R, seed=8, noise_sigma=20.0, solver="loglin", alpha=0.1)
        vals, ok = [], []
        for r in range(R):
            f = t2.fit_volume(t2.synth_replica(boot.fit.t2, boot.fit.k, te, 20.0, m, seed=8, replica=r), m, te, "gaussian", table,
                              solver="loglin", extras=True)
            vals.append(f.t2.double().cpu().numpy())
            ok.append(((f.status == 1) & torch.isfinite(f.t2)).cpu().numpy())
        ok = np.stack(ok)
        x = np.where(ok, np.stack(vals), np.nan)
        sel = (mask != 0) & (ok.sum(axis=0) >= 2)
        assert sel.sum() > 0.9 * (mask != 0).sum() and np.array_equal(boot.n_ok.cpu().numpy()[sel], ok.sum(axis=0)[sel])
        lo, hi = np.nanpercentile(x[:, sel], [5.0, 95.0], axis=0)
        assert np.all(_close_f32(boot.ci_lo.cpu().numpy()[sel], lo)) and np.all(_close_f32(boot.ci_hi.cpu().numpy()[sel], hi))
        assert np.all(_close_f32(boot.boot_mean.cpu().numpy()[sel], np.nanmean(x[:, sel], axis=0)))


# ---- 8. background noise level --------------------------------------------------------------------------------------
def test_background_sigma_equals_numpy_and_recovers_the_noise_level(t2):
    import torch

    from fetal_t2mapping_amd import synth

    echoes, mask, te = synth.brain_volume((20, 48, 64), 6, seed=synth.SEED_BASE + 3, low_field=True, sigma=20.0)
    bg = echoes[:, mask == 0].astype(np.float64)
    want = np.sqrt(np.sum(bg ** 2) / (2 * bg.size))
    sigma, count = t2.estimate_background_sigma(echoes, mask)
    assert count == bg.size and abs(sigma / want - 1.0) < 1e-12 and abs(sigma / 20.0 - 1.0) < 0.02
    e = torch.from_numpy(echoes).cuda()
    again = [t2.estimate_background_sigma(e, mask) for _ in range(3)]
    assert all(a == (sigma, count) for a in again)  # the same bits
    vm = np.ascontiguousarray(np.moveaxis(echoes, 0, -1))
    assert t2.estimate_background_sigma(vm, mask, layout="voxel_major") == (sigma, count)
    with pytest.raises(ValueError):
        t2.estimate_background_sigma(echoes, np.ones_like(mask))
    with pytest.raises(ValueError):
        t2.estimate_background_sigma(echoes, None)


# ---- 9. physics -----------------------------------------------------------------------------------------------------
def _clean_volume(shape, te, seed, t2_range=(60.0, 300.0), k=1500.0):
    rng = np.random.default_rng(seed)
    t2v = rng.uniform(*t2_range, shape)
    kv = np.full(shape, k)
    return kv, t2v, kv[None] * np.exp(-np.asarray(te)[:, None, None, None] / t2v[None])


def test_boot_std_agrees_with_the_linear_theory_where_it_holds(t2):
    """Converged LM in float64, 2-parameter gaussian model, 8 echoes, sigma = 5 on k = 1500 (SNR 300), T2 60..300 ms,
    far from the bounds: the Gauss-Newton standard error t2_se estimates the same spread the bootstrap measures.
    Measured on an MI355X: median boot_std / t2_se = 1.057.  t2_se carries s from 6 degrees of freedom, and the median
    of sqrt(chi2_6 / 6) is 0.944: a ratio of medians of 1 / 0.944 = 1.059 is what exact agreement looks like."""
    from fetal_t2mapping_amd import synth

    shape = (16, 32, 32)
    te = synth.te_vector(8, True)
    rng = np.random.default_rng(41)
    _, _, clean = _clean_volume(shape, te, 40)
    sigma = 5.0
    echoes = np.hypot(clean + rng.normal(scale=sigma, size=clean.shape), rng.normal(scale=sigma, size=clean.shape)).astype(np.float32)
    mask = np.ones(shape, np.uint8)
    boot = t2.bootstrap_volume(echoes, mask, te, "gaussian", t2.fit_table("gaussian", True), n_replicas=200, seed=1,
                               noise_sigma=sigma, interval=False, solver="lm", precision="f64")
    ratio = boot.boot_std / boot.fit.t2_se
    good = np.isfinite(ratio) & (boot.n_ok == 200)
    assert good.mean() > 0.99
    med = float(np.median(ratio[good]))
    print(f"median boot_std / t2_se = {med:.4f}; median boot_std {np.median(boot.boot_std[good]):.4f} ms")
    assert 0.9 <= med <= 1.1
    assert abs(float(np.median(boot.boot_bias[good]))) < 0.1 * float(np.median(boot.boot_std[good]))


def test_boot_std_agrees_with_a_true_monte_carlo(t2):
    """64 independent noisy acquisitions of one ground truth, fitted: the per-voxel standard deviation of T2 across them
    is what boot_std of any one of them estimates.  Measured on an MI355X: median ratio 1.0073."""
    from fetal_t2mapping_amd import synth

    shape = (8, 24, 32)
    te = synth.te_vector(6, True)
    _, _, clean = _clean_volume(shape, te, 50, t2_range=(60.0, 250.0))
    sigma = 20.0
    mask = np.ones(shape, np.uint8)
    table = t2.fit_table("gaussian", True)
    rng = np.random.default_rng(51)
    fits, boots = [], []
    for a in range(64):
        echoes = np.hypot(clean + rng.normal(scale=sigma, size=clean.shape), rng.normal(scale=sigma, size=clean.shape)).astype(np.float32)
        if a < 16:
            b = t2.bootstrap_volume(echoes, mask, te, "gaussian", table, n_replicas=64, seed=a, noise_sigma=sigma,
                                    interval=False, solver="lm", precision="f64")
            boots.append(b.boot_std)
            fits.append(b.fit.t2)
        else:
            fits.append(t2.fit_volume(echoes, mask, te, "gaussian", table, solver="lm", precision="f64").t2)
    truth = np.std(np.stack(fits).astype(np.float64), axis=0, ddof=1)
    est = np.median(np.stack(boots), axis=0)
    ratio = est / truth
    med = float(np.median(ratio[np.isfinite(ratio)]))
    print(f"median over voxels of median boot_std / Monte-Carlo std = {med:.4f}")
    assert abs(med - 1.0) <= 0.015


# ---- 10. raw ctypes ---------------------------------------------------------------------------------------------------
def test_raw_entry_point_equals_bootstrap_volume_and_refuses_an_oversized_workspace(t2, monkeypatch):
    import torch

    from fetal_t2mapping_amd import _abi, synth
    from fetal_t2mapping_amd._lib import load

    lib = load()
    echoes, mask, te = synth.brain_volume((8, 24, 32), 6, seed=synth.SEED_BASE + 4, low_field=True)
    table = t2.fit_table("gaussian", True)
    want = t2.bootstrap_volume(echoes, mask, te, "gaussian", table, n_replicas=10, seed=4, noise_sigma=20.0, alpha=0.1)
    cfg = t2.make_config("gaussian", table, te)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda().reshape(-1)  # noqa: E731
    t2_d, k_d, m_d = dev(want.fit.t2), dev(want.fit.k), dev(mask)
    n = m_d.numel()
    outs = {name: torch.full((n,), -7.0, dtype=torch.float32, device="cuda") for name in ("mean", "bias", "std", "ci_lo", "ci_hi")}
    n_ok = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    bm = _abi.T2FitBootMaps()
    for name, t in outs.items():
        getattr(bm, name)[0] = t.data_ptr()
    bm.n_ok = n_ok.data_ptr()

    def call(n_vox=n, R=10, ctx=None):  # interval mode, T2 only
        return lib.t2fit_bootstrap_dev(ctx, C.byref(cfg), t2_d.data_ptr(), k_d.data_ptr(), None, 20.0, None, 0, m_d.data_ptr(),
                                       n_vox, R, 4, 0.1, 1, C.byref(bm), 0, None)

    # a workspace beyond what the call may take is refused by arithmetic, before the HIP runtime is touched: nothing is
    # allocated, launched or written.  The sizes are the real ones (every pointer is valid for n voxels): the limit is
    # what is small.  n (8 nTE + 26) + n (4 + 24 + 4 R) bytes = 142 n here.
    monkeypatch.setenv("T2FIT_BOOT_MEM_LIMIT", str(141 * n))
    assert call() == _abi.E_HIP
    msg = lib.t2fit_last_error().decode()
    assert "GiB" in msg and "workspace" in msg and "T2FIT_BOOT_MEM_LIMIT" in msg
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in outs.values()) and bool((n_ok == -7).all())
    monkeypatch.setenv("T2FIT_BOOT_MEM_LIMIT", str(142 * n + 8))
    assert call() == _abi.OK
    monkeypatch.delenv("T2FIT_BOOT_MEM_LIMIT")
    for name, t in outs.items():
        assert t.cpu().numpy().tobytes() == getattr(want.t2, name).tobytes(), name
    assert np.array_equal(n_ok.cpu().numpy().reshape(mask.shape), want.n_ok)
    # through a context's streams: the same bits
    ctx = C.c_void_p()
    assert lib.t2fit_create(0, C.byref(ctx)) == _abi.OK
    for t in outs.values():
        t.fill_(-7.0)
    assert call(ctx=ctx) == _abi.OK and call(ctx=ctx) == _abi.OK
    assert lib.t2fit_destroy(ctx) == _abi.OK
    for name, t in outs.items():
        assert t.cpu().numpy().tobytes() == getattr(want.t2, name).tobytes(), name


# ---- 11. the CLI end to end -------------------------------------------------------------------------------------------
def _tree(tmp_path):
    """A tiny BIDS tree: three echoes of a synthetic brain volume and their masks, with a geometry of their own."""
    import pandas as pd

    from fetal_t2mapping_amd import cli as R
    from fetal_t2mapping_amd import nifti, synth

    shape = (10, 24, 32)
    echoes, mask, te = synth.brain_volume(shape, 3, seed=synth.SEED_BASE, low_field=True)
    root = str(tmp_path)
    bids = os.path.join(root, "projects") + "/"
    os.makedirs(os.path.join(bids, "prj-903"))
    os.makedirs(os.path.join(root, "dicom", "logs"))
    rows = []
    for i, t in enumerate(te):
        acq = {"prj": "prj-903", "sub": "sub-004", "ses": "ses-01", "run": f"run-{i + 1:02d}", "EchoTime": t / 1000.0,
               "CoilString": "HeadNeck"}
        rows.append(acq)
        for arr, dirname in ((echoes[i], R.recon_dirname), (mask, R.mask_dirname)):
            img = nifti.GetImageFromArray(arr)
            img.SetSpacing((1.0, 1.25, 2.0))
            img.SetOrigin((-11.0, 7.5, 3.0))
            nifti.WriteImage(img, R.get_img_path(bids, acq, dirname).replace(" ", ""))
    pd.DataFrame(rows).to_csv(os.path.join(root, "dicom", "logs", "log.csv"), index=False)
    out_dir = os.path.join(bids, "prj-903", "derivatives", R.t2map_dirname, "sub-004", "ses-01", "anat")
    return root, out_dir, echoes, mask, te


def test_cli_writes_the_bootstrap_maps(t2, tmp_path, monkeypatch, capsys):
    import sys

    from fetal_t2mapping_amd import cli as R
    from fetal_t2mapping_amd import nifti

    monkeypatch.setitem(sys.modules, "SimpleITK", None)
    stem = "sub-004_ses-01_recon_1mm_sim-b1_"
    fit = "gaussian_rician"
    map_files = sorted(stem + f"{m}map_ada-{fit}.nii.gz" for m in ("t2", "k", "sigma", "res"))
    boot_files = [stem + f"{tag}map_ada-{fit}.nii.gz" for tag in R.BOOT_TAGS]
    root0, out0, _, _, te = _tree(tmp_path / "plain")
    base = ["--csv", "log.csv", "--in_vivo", "--" + fit, "--lf", "--sim", "b1", "--TEs"] + [str(int(t)) for t in te]
    R.main(["--path", root0] + base)
    plain_log = capsys.readouterr().out
    assert sorted(os.listdir(out0)) == map_files and "ootstrap" not in plain_log
    root, out_dir, echoes, mask, _ = _tree(tmp_path / "boot")
    R.main(["--path", root] + base + ["--bootstrap", "12", "--bootstrap_seed", "3", "--bootstrap_alpha", "0.2"])
    log = capsys.readouterr().out
    assert sorted(os.listdir(out_dir)) == sorted(map_files + boot_files)
    line = [ln for ln in log.splitlines() if ln.startswith("Bootstrap: noise level")]
    assert len(line) == 1 and "12 replicas" in line[0] and "replicas/sec" in line[0] and "background" in line[0]
    read = lambda name: nifti.ReadImage(os.path.join(out_dir, name))  # noqa: E731
    t2_img = read(stem + f"t2map_ada-{fit}.nii.gz")
    for m in ("t2", "k", "sigma", "res"):  # the maps do not depend on the flag
        a = nifti.ReadImage(os.path.join(out0, stem + f"{m}map_ada-{fit}.nii.gz")).arr
        assert np.array_equal(a, read(stem + f"{m}map_ada-{fit}.nii.gz").arr, equal_nan=True)
    want = t2.bootstrap_volume(echoes, mask, te, fit, t2.fit_table(fit, True), n_replicas=12, seed=3, alpha=0.2)
    assert np.array_equal(want.fit.t2, t2_img.arr)
    for name, arr in zip(boot_files, (want.boot_std, want.boot_bias, want.ci_lo, want.ci_hi, want.n_ok)):
        img = read(name)
        assert img.GetSpacing() == t2_img.GetSpacing() == (1.0, 1.25, 2.0) and img.GetOrigin() == t2_img.GetOrigin()
        assert img.GetDirection() == t2_img.GetDirection() and img.arr.shape == mask.shape
        assert img.arr.dtype == arr.dtype and np.array_equal(img.arr, arr, equal_nan=True), name
