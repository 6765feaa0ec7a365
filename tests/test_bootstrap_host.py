"""Host side of the parametric bootstrap (no device): the numpy restatement of the replica stream against the published
known-answer vectors of Philox4x32-10, the ABI of the built library (version still 5, the three additive entry points,
every argument check refused with a message before HIP is touched), and the --bootstrap flags and file names of the
CLI.  tests/test_bootstrap_gpu.py runs the kernels."""
import ctypes as C
import os

import numpy as np
import pytest


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_philox4x32_10_known_answers():
    """The three vectors of the generator's published test file (Random123 kat_vectors, philox4x32 10)."""
    from fetal_t2mapping_amd import philox4x32_10

    ones = 0xFFFFFFFF
    assert _hex(philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(philox4x32_10((ones,) * 4, (ones, ones))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"
    # vectorised over counters: element i equals the scalar call
    c0 = np.array([0, ones, 0x243F6A88], np.uint32)
    w = philox4x32_10((c0, 0, 0, 0), (0, 0))
    assert w[0].shape == (3,) and w[0].dtype == np.uint32 and _hex(x[0] for x in w) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(x[1] for x in w) == _hex(philox4x32_10((ones, 0, 0, 0), (0, 0)))


def test_uniforms_are_exact_float32_inside_the_open_interval_and_normals_are_standard():
    from fetal_t2mapping_amd import _philox

    w = np.array([0, 1, 511, 512, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], np.uint32)
    u = _philox.uniforms(w)
    assert np.all(u > 0.0) and np.all(u < 1.0) and np.array_equal(u.astype(np.float32).astype(np.float64), u)
    assert u[0] == 2.0 ** -24 and u[-1] == 1.0 - 2.0 ** -24 and u[2] == u[0] and u[3] == 3 * 2.0 ** -24
    n1, n2 = _philox.normals(np.arange(400000), 3, 5, seed=7)
    for n in (n1, n2):
        assert abs(n.mean()) < 0.01 and abs(n.std() - 1.0) < 0.01 and np.abs(n).max() <= 5.78
    assert abs(np.corrcoef(n1, n2)[0, 1]) < 0.01
    # a sample is a function of (seed, voxel, echo, replica): any one of them changes it, the call shape does not
    a = _philox.normals(np.array([12345]), 3, 5, seed=7)[0][0]
    assert a == n1[12345]
    assert len({a, _philox.normals(12345, 4, 5, 7)[0].item(), _philox.normals(12345, 3, 6, 7)[0].item(),
                _philox.normals(12345, 3, 5, 8)[0].item(), _philox.normals(12345 + 2 ** 32, 3, 5, 7)[0].item(),
                _philox.normals(12345, 3, 5, 7 + 2 ** 32)[0].item()}) == 6
    r = _philox.replica(np.full((2, 3), 100.0), np.full((2, 3), 1000.0), [100.0, 200.0], 0.0, np.array([[1, 1, 0]] * 2),
                        seed=0, replica=0)
    assert r.shape == (2, 2, 3) and np.all(r[:, :, 2] == 0) and np.allclose(r[1, :, :2], 1000.0 * np.exp(-2.0))
    slab = _philox.replica(np.full((1, 3), 100.0), np.full((1, 3), 1000.0), [100.0, 200.0], 20.0, None, seed=0, replica=1,
                           voxel_offset=3)
    whole = _philox.replica(np.full((2, 3), 100.0), np.full((2, 3), 1000.0), [100.0, 200.0], 20.0, None, seed=0, replica=1)
    assert np.array_equal(slab[:, 0], whole[:, 1])


def test_built_library_keeps_abi_5_and_refuses_bad_bootstrap_arguments_without_a_device(monkeypatch):
    from fetal_t2mapping_amd import _abi, build

    assert _abi.ABI_VERSION == 5
    names = [s[0] for s in _abi.SYMBOLS]
    header = open(os.path.join(os.path.dirname(build.PKG), "include", "t2fit.h")).read()
    assert "#define T2FIT_ABI_VERSION 5" in header
    for sym in ("t2fit_boot_background_dev", "t2fit_boot_synth_dev", "t2fit_bootstrap_dev"):
        assert sym in names and sym + "(" in header
    assert any(src.endswith("t2fit_boot.hip") for src in build.SOURCES)
    import torch  # noqa: F401  (one HIP runtime per process: see _lib.load)

    lib = _abi.bind(C.CDLL(build.build()))
    assert lib.t2fit_abi_version() == 5
    cfg = _abi.T2FitConfig()
    assert lib.t2fit_config_default(C.byref(cfg), _abi.MODEL_GAUSSIAN_RICIAN, 1) == 0
    cfg2 = _abi.T2FitConfig()
    assert lib.t2fit_config_default(C.byref(cfg2), _abi.MODEL_GAUSSIAN, 1) == 0
    normed = _abi.T2FitConfig()
    assert lib.t2fit_config_default(C.byref(normed), _abi.MODEL_GAUSSIAN, 1) == 0
    normed.norm = 1
    p = 4096  # never dereferenced: every call below is refused first
    sig, cnt = C.c_double(), C.c_int64()

    def background(e=p, layout=0, mask=p, n_te=3, n_vox=64, s=C.byref(sig), c=C.byref(cnt)):
        return lib.t2fit_boot_background_dev(e, layout, mask, n_te, n_vox, s, c, None)

    def synth(c=cfg, t2=p, k=p, s=10.0, smap=None, n_vox=64, off=0, rep=0, kind=0, out=p):
        return lib.t2fit_boot_synth_dev(C.byref(c) if c is not None else None, t2, k, s, smap, None, n_vox, off, 1, rep, kind, out, None)

    def maps(ci=True, n_ok=p):
        m = _abi.T2FitBootMaps()
        for i in range(3):
            m.mean[i] = m.bias[i] = m.std[i] = p
            if ci:
                m.ci_lo[i] = m.ci_hi[i] = p
        m.n_ok = n_ok
        return m

    def boot(c=cfg, t2=p, k=p, sg=p, s=10.0, smap=None, kind=0, mask=p, n_vox=64, R=8, alpha=0.05, which=1, out=maps(), flags=0):
        return lib.t2fit_bootstrap_dev(None, C.byref(c) if c is not None else None, t2, k, sg, s, smap, kind, mask, n_vox, R, 3,
                                       alpha, which, C.byref(out) if out is not None else None, flags, None)

    cases = {
        "NULL": [lambda: background(e=None), lambda: background(mask=None), lambda: background(s=None), lambda: background(c=None),
                 lambda: synth(t2=None), lambda: synth(k=None), lambda: synth(out=None), lambda: boot(t2=None),
                 lambda: boot(k=None), lambda: boot(mask=None), lambda: boot(out=None), lambda: boot(c=None), lambda: synth(c=None),
                 lambda: boot(c=cfg, sg=None, which=4)],
        "layout": [lambda: background(layout=2)],
        "n_te": [lambda: background(n_te=0), lambda: background(n_te=33)],
        "n_vox": [lambda: background(n_vox=0), lambda: synth(n_vox=0), lambda: synth(n_vox=1 << 32), lambda: boot(n_vox=-1)],
        "norm": [lambda: synth(c=normed), lambda: boot(c=normed)],
        "noise_kind": [lambda: synth(kind=2), lambda: boot(kind=-1)],
        "noise_scalar": [lambda: synth(s=-1.0), lambda: synth(s=float("nan")), lambda: boot(s=float("inf"))],
        "negative": [lambda: synth(rep=-1), lambda: synth(off=-1)],
        "which_params": [lambda: boot(which=0), lambda: boot(which=8)],
        "no sigma": [lambda: boot(c=cfg2, which=4), lambda: boot(c=cfg2, which=5)],
        "flags": [lambda: boot(flags=1), lambda: boot(flags=2)],
        "n_replicas": [lambda: boot(R=0)],
        "at least 2 replicas": [lambda: boot(R=1)],
        "at most 512 replicas": [lambda: boot(R=513)],
        "alpha": [lambda: boot(alpha=0.0), lambda: boot(alpha=1.0), lambda: boot(alpha=float("nan"))],
    }
    for word, calls in cases.items():
        for i, call in enumerate(calls):
            assert call() == _abi.E_INVALID, (word, i)
            assert word in lib.t2fit_last_error().decode(), (word, i, lib.t2fit_last_error().decode())
    # the workspace check is arithmetic and comes before the HIP runtime: 64 voxels, 3 echoes, moments only need
    # 64 (8 * 3 + 26) + 8 + 64 * 28 = 5 000 bytes at most.  Only where there is no device (nothing can then be launched
    # on the pointers above, whatever the check does).
    if lib.t2fit_device_count() == 0:
        monkeypatch.setenv("T2FIT_BOOT_MEM_LIMIT", "4999")
        assert boot(R=1, out=maps(ci=False)) == _abi.E_HIP
        msg = lib.t2fit_last_error().decode()
        assert "workspace" in msg and "T2FIT_BOOT_MEM_LIMIT" in msg and "GiB" in msg
        monkeypatch.setenv("T2FIT_BOOT_MEM_LIMIT", "5000")
        assert boot(R=1, out=maps(ci=False)) == _abi.E_HIP  # passes the limit; then there is no device
        assert "T2FIT_BOOT_MEM_LIMIT" not in lib.t2fit_last_error().decode()
        # moments only: one replica and more than 512 pass the argument checks
        assert boot(R=600, out=maps(ci=False)) == _abi.E_HIP and "replicas" not in lib.t2fit_last_error().decode()


def test_cli_bootstrap_flags_refusals_and_file_names(tmp_path):
    from fetal_t2mapping_amd import cli as R

    base = ["--path", "x", "--csv", "a.csv", "--in_vivo", "--gaussian_rician", "--lf", "--sim", "7"]
    args = R.parse_arguments(base)
    assert args.bootstrap == 0 and args.bootstrap_seed == 0 and args.bootstrap_alpha == 0.05 and args.bootstrap_noise == "background"
    args = R.parse_arguments(base + ["--bootstrap", "64", "--bootstrap_seed", "11", "--bootstrap_alpha", "0.1",
                                     "--bootstrap_noise", "sigma_map"])
    assert (args.bootstrap, args.bootstrap_seed, args.bootstrap_alpha, args.bootstrap_noise) == (64, 11, 0.1, "sigma_map")
    assert R.parse_arguments(base + ["--bootstrap", "16", "--bootstrap_noise", "12.5"]).bootstrap_noise == 12.5
    assert R.parse_bootstrap_noise("background") == "background" and R.parse_bootstrap_noise("3") == 3.0
    for bad in ("rayleigh", "-1", "0", "nan", "inf"):
        with pytest.raises(ValueError):
            R.parse_bootstrap_noise(bad)
    gauss = ["--path", "x", "--csv", "a.csv", "--in_vivo", "--gaussian", "--hf", "--sim", "7"]
    fast = ["--path", "x", "--csv", "a.csv", "--in_vitro_fast", "--gaussian", "--hf", "--sim", "7"]
    for argv in (base + ["--bootstrap", "16", "--norm"], fast + ["--bootstrap", "16"], gauss + ["--bootstrap", "16", "--bootstrap_noise", "sigma_map"],
                 base + ["--bootstrap", "1"], base + ["--bootstrap", "513"], base + ["--bootstrap", "16", "--bootstrap_alpha", "1.0"],
                 base + ["--bootstrap", "16", "--bootstrap_noise", "loud"]):
        with pytest.raises(SystemExit):
            R.parse_arguments(argv)
    # without --bootstrap its companions are not looked at
    assert R.parse_arguments(base + ["--norm", "--bootstrap_noise", "loud"]).bootstrap == 0
    bids = str(tmp_path / "projects") + "/"
    assert R.BOOT_TAGS == ("T2std", "T2bias", "T2cilo", "T2cihi", "T2nok")
    for acq, fit in (({"prj": "prj-004", "sub": "sub-002", "ses": "ses-01", "run": "run-03", "EchoTime": 0.114, "CoilString": "HeadNeck"}, "gaussian_rician"),
                     ({"prj": "prj-002", "sub": "sub-010", "ses": "ses-02", "run": "run-01", "EchoTime": 0.115, "CoilString": "Body"}, "gaussian")):
        t2 = R.get_img_path(bids, acq, R.t2map_dirname).replace("t2map.nii.gz", f"sim-7_t2map_ada-{fit}.nii.gz")
        got = [R.boot_map_path(bids, acq, R.t2map_dirname, "7", fit, tag) for tag in R.BOOT_TAGS]
        assert got == [t2.replace("_t2map_", f"_{tag}map_") for tag in R.BOOT_TAGS] and len(set(got)) == 5
        assert os.path.relpath(got[0], bids) == (f"{acq['prj']}/derivatives/recon_1mm_t2map/{acq['sub']}/{acq['ses']}/anat/"
                                                 f"{acq['sub']}_{acq['ses']}_recon_1mm_sim-7_T2stdmap_ada-{fit}.nii.gz")


def test_crafted_bootstrap_case_has_every_count_ties_on_both_bounds_and_few_samples_near_zero():
    """tests/boot_cases.py by its float64 statement alone (no device, no library): what the device tests rely on."""
    import boot_cases as BC

    t2, k, s, names = BC.maps()
    assert t2.shape == BC.SHAPE and BC.N == 651 and BC.N % 4 and BC.N % 64
    y, counted, near, t2_fit = BC.predict()
    assert y.shape == (BC.R, 2, BC.N) and BC.R == 16
    n = counted.sum(axis=0)
    hist = np.bincount(n, minlength=BC.R + 1)
    print("count histogram 0..R:", hist.tolist())
    assert hist.size == BC.R + 1 and np.all(hist > 0)  # every count 0..R occurs
    upper = int(np.sum(np.sum(t2_fit == BC.T2_BOUNDS[1], axis=0) >= 2))
    lower = int(np.sum(np.sum(t2_fit == BC.T2_BOUNDS[0], axis=0) >= 2))
    print(f"voxels with two or more counted refits on the T2 bound: upper {upper}, lower {lower}")
    assert upper >= 50 and lower >= 10
    flat = names.reshape(-1)
    same = flat == "k1500_s0"  # the s = 0 class: every replica is the clean signal, and counts
    assert same.sum() >= 10 and np.all(s.reshape(-1)[same] == 0.0) and np.all(n[same] == BC.R)
    assert np.all(y[:, :, same] == y[:1, :, same]) and np.all(y[:, :, same] > 0.0)
    for name in ("zero_s0", "t2_nan", "k_nan", "k_inf"):  # never count
        assert (flat == name).sum() >= 3 and np.all(n[flat == name] == 0), name
    for name in ("t2_inf_k60", "t2_inf_k2000", "t2_zero", "steep"):
        assert (flat == name).sum() >= 3, name
    assert np.all(n[flat == "t2_inf_k60"] >= 2) and np.all(n[flat == "steep"] == BC.R)
    print(f"voxels with a sample within {BC.NEAR} s of zero: {int(near.sum())} of {BC.N}")
    assert near.mean() <= 0.01
    # voxels whose counted T2 refits are all equal while the shifted sums the kernel keeps round to a positive variance:
    # only the min / max it keeps as well make their std exactly 0
    x = np.where(counted, t2_fit, np.nan)
    rounds_up = [int(i) for i in np.flatnonzero((n >= 2) & np.isfinite(t2.reshape(-1)))
                 if np.nanmin(x[:, i]) == np.nanmax(x[:, i])
                 and BC.shifted_variance_of_equal(np.nanmax(x[:, i]), t2.reshape(-1)[i], int(n[i])) > 0.0]
    print(f"voxels of equal refits whose shifted variance rounds above 0: {rounds_up}")
    assert len(rounds_up) >= 3
    # the masks of the mask-count tests: exact counts, both ends of the volume set in some and clear in others
    counts = (0, 1, 63, 64, 65, 255, 256, 257)
    masks = BC.masks_with(counts)
    assert [int(m.sum()) for m in masks] == list(counts)
    for end in (0, -1):
        ends = {int(m.reshape(-1)[end]) for m in masks[1:]}
        assert ends == {0, 1}
