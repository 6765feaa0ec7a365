"""The vector-valued (joint) TV denoiser without a device: the numpy statement (fetal_t2mapping_amd/_tv.py,
tv_joint_problem) against the voxel-by-voxel reference of tests/tvj_cases.py, mutations the reference must notice, the
identities of the model (C = 1 is the scalar problem, equal channels are the scalar problem at weight w / sqrt(C), a channel
of zeros changes nothing), the argument checks of the two entry points, the flags, the benefit on a multi-echo phantom and
the joint prox of the super-resolution statement.  tests/test_tvj_gpu.py holds the device to the statement."""
import ctypes as C

import numpy as np
import pytest

import tvj_cases as K

from fetal_t2mapping_amd import _tv

REF_IDS = [f"C{c}-" + "x".join(map(str, sp)) for c, sp in K.REF_CASES]


@pytest.mark.parametrize("chans,sp", K.REF_CASES, ids=REF_IDS)
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_statement_is_bit_equal_to_the_voxel_by_voxel_reference(chans, sp, precision):
    """`out` bit for bit after REF_ITERS iterations; E within 1e-13 (the reference sums exactly, the statement pairwise)."""
    assert K.statement_matches_reference(chans, sp, precision)
    assert max(sp_ for _, sp_ in K.REF_CASES if len(sp_) == 2) == (4, 5) and (3, (3, 4, 5)) in K.REF_CASES


@pytest.mark.parametrize("name", sorted(K.MUTATIONS))
def test_a_mutated_statement_fails(name):
    """Each wrong variant misses the reference on at least one case with C = 3, and the unmutated statement is back after."""
    with K.mutated(name):
        missed = [(c, sp, p) for c, sp in K.REF_CASES for p in ("f32", "f64") if not K.statement_matches_reference(c, sp, p)]
    print(name, "noticed on", missed)
    assert missed and all(c > 1 for c, _, _ in missed)  # with one channel the three variants are the statement itself
    assert all(K.statement_matches_reference(c, sp, p) for c, sp in K.REF_CASES for p in ("f32", "f64"))


@pytest.mark.parametrize("dims", [2, 3])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_one_channel_is_the_scalar_problem(dims, precision):
    """Bytes, n_iter and E of tv_problem, with the stop rule active (the problems stop well before the limit)."""
    a = K.field((1, 4, 20, 23), seed=3)
    f = a[0, 0] if dims == 2 else a[0]
    for weight in (10.0, 40.0):
        h0, h1 = [], []
        want, want_n, want_e = _tv.tv_problem(f, weight, 2e-4, 200, K.DTYPE[precision], history=h0)
        got, n, e = _tv.tv_joint_problem(f[None], weight, 2e-4, 200, K.DTYPE[precision], history=h1)
        assert 1 < want_n < 199 and n == want_n and e == want_e and h0 == h1
        assert got.shape == (1,) + f.shape and got[0].tobytes() == want.tobytes()
    out, n_iter, energy = _tv.denoise_tv_joint(a, 25.0, 2e-4, 200, dims, precision)
    want = _tv.denoise_tv(a, 25.0, 2e-4, 200, dims, precision)
    assert out.tobytes() == want[0].tobytes() and np.array_equal(n_iter, want[1]) and np.array_equal(energy, want[2])


# the largest |joint - scalar at w / sqrt(C)| / max |f| over the cases of the test below, measured on the statement
EQUAL_CHANNELS_MEASURED = {"f32": 2.25e-7, "f64": 3.36e-16}


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_equal_channels_are_the_scalar_problem_at_weight_over_sqrt_c(precision):
    """C copies of one image: S = C sq, so nrm = sqrt(C) |g| and the update is the scalar one at weight w / sqrt(C): an
    identity of the model, not of the rounding (sqrt(C) is rounded, S is summed).  Measured on the statement over exactly
    these cases (C in 2, 3, 6; 24 x 31 and 5 x 9 x 12; 10 and 50 iterations; weight 40): the largest difference relative to
    max |f| is 2.25e-7 in float32 and 3.36e-16 in float64 (EQUAL_CHANNELS_MEASURED).  The bar is ten times that."""
    worst = 0.0
    for chans in (2, 3, 6):
        for dims, shape in ((2, (1, 1, 24, 31)), (3, (1, 5, 9, 12))):
            f = K.field(shape, seed=77)[0]
            f = f[0] if dims == 2 else f
            for iters in (10, 50):
                joint = _tv.tv_joint_problem(np.stack([f] * chans), 40.0, 0.0, iters, K.DTYPE[precision])[0]
                one = _tv.tv_problem(f, 40.0 / np.sqrt(chans), 0.0, iters, K.DTYPE[precision])[0]
                assert all(joint[c].tobytes() == joint[0].tobytes() for c in range(chans))
                worst = max(worst, float(np.max(np.abs(joint[0].astype(np.float64) - one)) / np.max(np.abs(f))))
                twice = _tv.tv_problem(f, 40.0, 0.0, iters, K.DTYPE[precision])[0]  # (the unscaled weight is far away)
                assert float(np.max(np.abs(joint[0].astype(np.float64) - twice)) / np.max(np.abs(f))) > 1e-3
    print(f"{precision}: largest relative difference {worst:.3g}, measured {EQUAL_CHANNELS_MEASURED[precision]:.3g}")
    assert worst <= 10.0 * EQUAL_CHANNELS_MEASURED[precision]


@pytest.mark.parametrize("dims", [2, 3])
def test_a_channel_of_zeros_changes_no_other_channel(dims):
    """sq = 0 of the zero channel is added to S exactly (in any position), and its own output stays 0."""
    a = K.field((3, 3, 9, 11), seed=8)
    f = a[:, 0] if dims == 2 else a
    want = _tv.tv_joint_problem(f, 25.0, 0.0, 12, np.float32)[0]
    for at in (0, 1, 3):
        wider = np.insert(f, at, 0.0, axis=0)
        got = _tv.tv_joint_problem(wider, 25.0, 0.0, 12, np.float32)[0]
        assert np.all(got[at] == 0.0) and np.delete(got, at, axis=0).tobytes() == want.tobytes(), at


def test_stack_call_is_the_problems_one_by_one():
    a = K.field((3, 4, 10, 13), seed=12)
    out, n_iter, energy = _tv.denoise_tv_joint(a, 20.0, 2e-4, 200, 2, "f32")
    assert out.dtype == np.float32 and out.shape == a.shape and n_iter.shape == (4,) and len(set(n_iter.tolist())) >= 1
    for z in range(4):
        o, n, e = _tv.tv_joint_problem(a[:, z], 20.0, 2e-4, 200, np.float32)
        assert out[:, z].tobytes() == o.tobytes() and n_iter[z] == n and energy[z] == e
    out3, n3, e3 = _tv.denoise_tv_joint(a, 20.0, 0.0, 9, 3, "f64")
    o, n, e = _tv.tv_joint_problem(a, 20.0, 0.0, 9, np.float64)
    assert out3.tobytes() == o.astype(np.float32).tobytes() and n3.tolist() == [8] and e3[0] == e
    with pytest.raises(ValueError):
        _tv.denoise_tv_joint(a[0], 20.0)
    with pytest.raises(ValueError):
        _tv.tv_joint_problem(a[0, 0], 20.0)


def test_entry_points_refuse_bad_arguments_without_a_device_and_the_workspace_arithmetic():
    import os

    from fetal_t2mapping_amd import _abi, build

    names = [s[0] for s in _abi.SYMBOLS]
    header = open(os.path.join(os.path.dirname(build.PKG), "include", "t2fit.h")).read()
    assert _abi.ABI_VERSION == 5 and "#define T2FIT_ABI_VERSION 5" in header
    assert _abi.TVJ_SYMBOLS == ("t2fit_tv_joint_workspace_bytes", "t2fit_tv_joint_denoise_dev")
    for sym in _abi.TVJ_SYMBOLS:
        assert sym in names and sym + "(" in header and sym in _abi.LOOKED_UP
    assert f"#define T2FIT_TV_JOINT_MAX_CHAN {_abi.TV_JOINT_MAX_CHAN}" in header
    assert _abi.TV_JOINT_MAX_CHAN == K.MAX_CHAN >= 16
    import torch  # noqa: F401  (one HIP runtime per process: see _lib.load)

    lib = _abi.bind(C.CDLL(build.build()))
    par = _abi.T2FitTvParams()
    assert lib.t2fit_tv_params_default(C.byref(par)) == _abi.OK

    up = lambda v: (v + 255) // 256 * 256  # noqa: E731
    cdiv = lambda a, b: (a + b - 1) // b  # noqa: E731

    def want_bytes(dims, elem, n_chan, nz, ny, nx):
        problems = nz if dims == 2 else 1
        tiles = problems * (cdiv(ny, 32) * cdiv(nx, 64) if dims == 2 else cdiv(nz, 4) * cdiv(ny, 8) * cdiv(nx, 64))
        return 2 * up(dims * n_chan * nz * ny * nx * elem) + up(16 * tiles) + up(32 * problems)

    need, scalar = C.c_size_t(), C.c_size_t()
    for dims in (2, 3):
        for prec, elem in ((_abi.PREC_F32, 4), (_abi.PREC_F64, 8)):
            for size in ((8, 256, 256, 256), (6, 180, 256, 256), (1, 1, 1, 1), (3, 5, 33, 65), (K.MAX_CHAN, 16, 17, 1)):
                par.dims, par.precision = dims, prec
                assert lib.t2fit_tv_joint_workspace_bytes(C.byref(par), *size, C.byref(need)) == _abi.OK
                assert need.value == want_bytes(dims, elem, *size), (dims, prec, size)
                assert lib.t2fit_tv_workspace_bytes(C.byref(par), *size, C.byref(scalar)) == _abi.OK
                assert need.value <= scalar.value and (size[0] > 1 or need.value == scalar.value)
    assert lib.t2fit_tv_params_default(C.byref(par)) == _abi.OK
    assert lib.t2fit_tv_joint_workspace_bytes(C.byref(par), 1, 4, 4, 4, None) == _abi.E_INVALID

    p = 4096  # never dereferenced: every call below is refused first
    ok_size = (2, 3, 8, 8)
    assert lib.t2fit_tv_joint_workspace_bytes(C.byref(par), *ok_size, C.byref(need)) == _abi.OK

    def refused(fragment, par=par, src=p, dst=p, size=ok_size, ws=p, ws_bytes=None):
        rc = lib.t2fit_tv_joint_denoise_dev(C.byref(par) if par is not None else None, src, dst, *size, ws,
                                            need.value if ws_bytes is None else ws_bytes, None, None, None)
        msg = lib.t2fit_last_error().decode()
        assert rc == _abi.E_INVALID and fragment in msg and "t2fit_tv_joint_denoise_dev" in msg, (fragment, rc, msg)

    refused("NULL", src=None)
    refused("NULL", dst=None)
    refused("NULL", ws=None)
    refused("params is NULL", par=None)
    refused("workspace too small", ws_bytes=need.value - 1)
    refused("not aligned to 256", ws=p + 64)
    refused("not aligned to 4", src=p + 2)
    refused("not aligned to 4", dst=p + 1)
    for size in ((0, 3, 8, 8), (-2, 3, 8, 8), (2, 0, 8, 8), (2, 3, -1, 8), (2, 3, 8, 0)):
        refused(">= 1", size=size)
    refused("T2FIT_TV_JOINT_MAX_CHAN", size=(K.MAX_CHAN + 1, 3, 8, 8))
    refused("T2FIT_TV_JOINT_MAX_CHAN", size=(2 ** 31 - 1, 1, 1, 1))
    refused("2^40", size=(K.MAX_CHAN, 2 ** 31 - 1, 2 ** 10, 2))
    refused("2^40", size=(16, 2 ** 20, 2 ** 20, 1))
    refused("tiles", size=(K.MAX_CHAN, 2 ** 25, 1, 1))
    for size in ((K.MAX_CHAN + 1, 3, 8, 8), (0, 3, 8, 8), (2, 3, 8, 0)):
        assert lib.t2fit_tv_joint_workspace_bytes(C.byref(par), *size, C.byref(need)) == _abi.E_INVALID
    assert lib.t2fit_tv_joint_workspace_bytes(C.byref(par), *ok_size, C.byref(need)) == _abi.OK

    def with_(**kw):
        q = _abi.T2FitTvParams()
        lib.t2fit_tv_params_default(C.byref(q))
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    for kw, fragment in (({"weight": 0.0}, "weight"), ({"weight": -1.0}, "weight"), ({"weight": float("nan")}, "weight"),
                         ({"weight": float("inf")}, "weight"), ({"eps": -1e-9}, "eps"), ({"eps": float("nan")}, "eps"),
                         ({"max_iter": 0}, "max_iter"), ({"dims": 1}, "dims"), ({"dims": 4}, "dims"),
                         ({"precision": 2}, "precision"), ({"flags": 1}, "flags")):
        refused(fragment, par=with_(**kw))
        assert lib.t2fit_tv_joint_workspace_bytes(C.byref(with_(**kw)), 1, 4, 4, 4, C.byref(need)) == _abi.E_INVALID


def test_flags(capsys):
    from fetal_t2mapping_amd import cli as R
    from fetal_t2mapping_amd import recon

    base = ["--path", "/x", "--csv", "a.csv", "--in_vivo", "--gaussian", "--lf", "--sim", "1"]
    old = {"weight": ("abs", 0.1), "dims": 2, "eps": 2e-4, "max_iter": 200}
    assert R.parse_arguments(base + ["--denoise", "tv"]).denoise_args == old
    assert R.parse_arguments(base + ["--denoise", "tv_joint"]).denoise_args == {**old, "joint": True}
    a = R.parse_arguments(base + ["--denoise", "tv_joint", "--denoise_weight", "2.4sigma", "--denoise_dims", "3",
                                  "--denoise_eps", "0", "--denoise_iter", "50"])
    assert a.denoise_args == {"weight": ("sigma", 2.4), "dims": 3, "eps": 0.0, "max_iter": 50, "joint": True}
    for extra, word in ((["--denoise", "nlm"], "invalid choice"), (["--denoise", "tv_joint", "--bootstrap", "10"], "--bootstrap"),
                        (["--recon_sr_tv", "joint"], "--recon_method sr"),
                        (["--reconstruct", "--recon_sr_tv", "joint"], "--recon_method sr"),
                        (["--reconstruct", "--recon_method", "sr", "--recon_sr_tv", "both"], "invalid choice")):
        with pytest.raises(SystemExit):
            R.parse_arguments(base + extra)
        assert word in capsys.readouterr().err, extra
    plain = R.parse_arguments(base + ["--reconstruct", "--recon_method", "sr"]).reconstruct_args["sr"]
    assert "tv" not in plain
    given = R.parse_arguments(base + ["--reconstruct", "--recon_method", "sr", "--recon_sr_tv", "channel"]).reconstruct_args["sr"]
    assert given == plain
    joint = R.parse_arguments(base + ["--reconstruct", "--recon_method", "sr", "--recon_sr_tv", "joint"]).reconstruct_args["sr"]
    assert joint == {**plain, "tv": "joint"}
    with pytest.raises(SystemExit):
        R.parse_arguments(base + ["--help"])
    assert "sqrt(nTE)" in " ".join(capsys.readouterr().out.split()) and "sqrt(nTE)" in " ".join(R.__doc__.split())
    assert "sr_tv" in recon.SR_FLAGS
    import inspect

    assert inspect.signature(R.denoise_subject).parameters["joint"].default is False


def test_recon_flags(capsys):
    from fetal_t2mapping_amd import recon

    src = open(recon.__file__).read()
    assert '"channel", "joint"' in src
    import argparse

    p = argparse.ArgumentParser()
    recon.add_sr_arguments(p, "")
    for argv, want in ((["--recon_method", "sr"], None), (["--recon_method", "sr", "--sr_tv", "channel"], None),
                       (["--recon_method", "sr", "--sr_tv", "joint"], "joint")):
        out = recon.sr_arguments(p, p.parse_args(argv), "", argv)
        assert out.get("tv") == want, argv
    with pytest.raises(SystemExit):
        recon.sr_arguments(p, p.parse_args(["--sr_tv", "joint"]), "", ["--sr_tv", "joint"])
    assert "--recon_method sr" in capsys.readouterr().err


def test_joint_tv_fits_t2_better_than_per_echo_tv_on_the_phantom():
    """The 64 x 64 multi-echo phantom of tvj_cases (6 echoes, Rician sigma 25, seed 0), 100 iterations at eps 0 on the
    float32 statement, T2 from an unweighted log-linear fit: the best joint T2 RMSE over the weights {0.5, 1, 2, 3} sigma
    is strictly below the best per-echo one.  Measured: none 24.50; per-echo 13.11 / 12.83 / 16.14 / 19.61; joint 16.95 /
    12.47 / 10.73 / 11.40 ms."""
    none, per, joint = K.benefit_tables()
    print(f"T2 RMSE (ms): none {none:.2f}; per-echo {per}; joint {joint}")
    assert tuple(per) == tuple(joint) == (0.5, 1.0, 2.0, 3.0)
    assert min(per.values()) < none and min(joint.values()) < min(per.values())


def test_super_resolution_statement_with_the_joint_prox():
    """tv='joint' with one echo is tv='channel'; with three echoes of the vial phantom (side 16 instead of 48, so that the
    host loop runs in seconds) it returns finite output of the right shape that differs from 'channel'."""
    from test_recon_gpu import _phantom_stacks

    from fetal_t2mapping_amd import _sr

    stacks, geoms = _phantom_stacks(n_te=3, side=16, thick=4.0)[:2]
    kw = dict(weight=20.0, n_iter=2, prox_iter=5)
    one = {o: v[:1] for o, v in stacks.items()}
    a, _ = _sr.reconstruct_sr(one, geoms, **kw)
    b, _ = _sr.reconstruct_sr(one, geoms, tv="joint", **kw)
    assert a.shape == (1, 16, 16, 16) and a.tobytes() == b.tobytes()
    chan, hi = _sr.reconstruct_sr(stacks, geoms, **kw)
    same, _ = _sr.reconstruct_sr(stacks, geoms, tv="channel", **kw)
    joint, hj = _sr.reconstruct_sr(stacks, geoms, tv="joint", **kw)
    assert same.tobytes() == chan.tobytes()
    assert joint.shape == chan.shape == (3, 16, 16, 16) and joint.dtype == np.float32 and np.isfinite(joint).all()
    assert hi.shape == hj.shape and not np.array_equal(joint, chan)
    assert np.array_equal(chan[0], a[0])  # per echo, the echoes do not see each other; jointly they do
    assert not np.array_equal(joint[0], a[0])
    j64, _ = _sr.reconstruct_sr(stacks, geoms, tv="joint", out_dtype=np.float64, **kw)
    assert j64.dtype == np.float64 and float(np.max(np.abs(j64 - joint))) < 1e-2
    with pytest.raises(ValueError, match="tv must be"):
        _sr.reconstruct_sr(stacks, geoms, tv="both", **kw)
