"""The super-resolution operator, its adjoint and the proximal-gradient loop as fetal_t2mapping_amd/_sr.py states them,
without a device: adjointness to a derived bound, a dense matrix written pair by pair, the aligned box case against the
phantom's block means, the candidate boxes by brute force, the edge cases of the loop, every refusal (Python and C ABI:
the library checks its arguments before it touches HIP), the command-line flags and the recovery of the phantom."""
import ctypes as C
import os

import numpy as np
import pytest

import sr_cases as K
from fetal_t2mapping_amd import _resample as R
from fetal_t2mapping_amd import _sr as S


@pytest.mark.parametrize("profile", K.PROFILE_NAMES)
@pytest.mark.parametrize("name", sorted(K.DIRECTIONS))
def test_forward_and_adjoint_are_adjoint_to_the_rounding_bound(name, profile):
    """<A x, r> and <x, A^T r> are two groupings of the same terms t = w x r / N over the pairs that count: each grouping is
    off the exact sum by less than n_terms 2^-53 sum |t| (every term passes through fewer than n_terms roundings), so the
    two differ by less than n_terms 2^-52 sum |t|."""
    c = K.small_case(name)
    rng = np.random.default_rng(41)
    x = rng.normal(size=c.hr.shape)
    r = rng.normal(size=c.stack.shape)
    ax, n = S.forward(x, c.B, c.stack.shape, profile, c.rel, mask=c.mask, out_dtype=np.float64)
    atr = S.adjoint([r], [n], [c.B], profile, c.rel, c.hr.shape, masks=[c.mask], out_dtype=np.float64)
    counts = (n > 0) & (c.mask != 0)
    assert counts.sum() > 100 and np.any(c.mask == 0) and c.rel != 1.0 and np.all(ax[~counts] == 0.0)
    w = K.weights_by_broadcast(c.B, c.hr.shape, c.stack.shape, profile, c.rel)[counts.ravel()]
    terms = np.abs(w * x.ravel()[None, :] * (r[counts] / n[counts])[:, None])
    n_terms = int(np.count_nonzero(w))
    bound = n_terms * 2.0 ** -52 * float(terms.sum())
    lhs, rhs = float(np.sum(ax * r)), float(np.sum(x * atr))
    print(f"{name} {profile}: |lhs - rhs| = {abs(lhs - rhs):.3e}, bound {bound:.3e}, {n_terms} terms")
    assert n_terms > 1000 and abs(lhs - rhs) <= bound


@pytest.mark.parametrize("name,profile", [("ax", "box"), ("sag_oblique", "bspline3"), ("cor_oblique", "box"), ("cor", "bspline3")])
def test_statement_equals_a_dense_matrix_written_pair_by_pair(name, profile):
    c = K.Case(name, (7, 6, 5), (5, 4, 2), (1.0, 1.1, 2.5), 3.5, K.rigid(0.5), seed=42)
    hr, lr = c.hr.shape, c.stack.shape
    W, N = K.dense_matrix(c.B, hr, lr, profile, c.rel)
    n_h, n_l = W.shape[1], W.shape[0]
    assert np.count_nonzero(W) > 4 * n_l and np.any(N > 0)
    # every entry: x = the unit vectors gives w / N per pair, the weights alone give N
    units = np.eye(n_h).reshape((n_h,) + hr)
    got, n = S.forward(units, c.B, lr, profile, c.rel, out_dtype=np.float64)
    assert np.array_equal(n.ravel(), N)
    counts = N > 0
    want = np.where(counts[:, None], W / np.where(counts, N, 1.0)[:, None], 0.0)
    assert np.array_equal(got.reshape(n_h, n_l).T, want)
    assert np.array_equal(S.forward(None, c.B, lr, profile, c.rel, hr_shape=hr)[1].ravel(), N)
    # rows sum to 1 where N > 0: the sum of w x over a constant 1 is the very sum that made N
    ones = S.forward(np.ones(hr), c.B, lr, profile, c.rel, out_dtype=np.float64)[0].ravel()
    assert np.all(ones[counts] == 1.0) and np.all(ones[~counts] == 0.0)
    # both directions on random data, masked, in the order the definition fixes
    rng = np.random.default_rng(43)
    x, r = rng.normal(size=n_h), rng.normal(size=n_l)
    cm = counts & (c.mask.ravel() != 0)
    f = S.forward(x.reshape(hr), c.B, lr, profile, c.rel, mask=c.mask, out_dtype=np.float64)[0]
    assert np.array_equal(f.ravel(), K.dense_forward(W, N, x, cm))
    a = S.adjoint([r.reshape(lr)], [n], [c.B], profile, c.rel, hr, masks=[c.mask], out_dtype=np.float64)
    assert np.array_equal(a.ravel(), K.dense_adjoint(W, N, r, cm))
    # the transposed unit vectors: the adjoint holds the very same w / N
    back = S.adjoint([np.eye(n_l).reshape((n_l,) + lr)], [n], [c.B], profile, c.rel, hr, out_dtype=np.float64)
    assert np.array_equal(back.reshape(n_l, n_h), want)


def test_aligned_box_operator_reproduces_the_phantom_block_means():
    """Thickness 4 on the truth's own 1 mm grid: A_s is the mean over the four voxels of a slice, and the half-open edge
    gives every voxel to exactly one slice of every stack."""
    stacks, geoms, truth, grid, _, _ = K.phantom()
    n_te, side = truth.shape[0], truth.shape[-1]
    n_sl = side // 4
    clean = {"ax": truth.reshape(n_te, n_sl, 4, side, side).mean(2),
             "cor": truth.reshape(n_te, side, n_sl, 4, side).mean(3).transpose(0, 2, 1, 3),
             "sag": truth.reshape(n_te, side, side, n_sl, 4).mean(4).transpose(0, 3, 1, 2)}
    for o in ("ax", "cor", "sag"):
        B = R.index_affine(grid, geoms[o])
        got, n = S.forward(truth, B, geoms[o].shape, "box", 1.0, out_dtype=np.float64)
        assert np.all(n == 4.0), o
        assert np.allclose(got, clean[o], rtol=4 * 2.0 ** -52, atol=0.0), o
        owners = S.adjoint([n], [n], [B], "box", 1.0, grid.shape, out_dtype=np.float64)  # sum_j w N / N: the slices that claim v
        assert np.all(owners == 1.0), o


def _brute_force_box_check(B, hr_shape, lr_shape, profile, rel, box):
    binv, radius = box
    w = K.weights_by_broadcast(B, hr_shape, lr_shape, profile, rel)
    jx, jy, jz = (np.broadcast_to(g, lr_shape).ravel() for g in S._grid((0, 0, 0), lr_shape))
    k = [np.floor(S._coord(binv, a, jx, jy, jz) + 0.5) for a in range(3)]
    vx, vy, vz = (np.broadcast_to(g, hr_shape).ravel() for g in S._grid((0, 0, 0), hr_shape))
    far = ((np.abs(vx[None, :] - k[0][:, None]) > radius[0]) | (np.abs(vy[None, :] - k[1][:, None]) > radius[1])
           | (np.abs(vz[None, :] - k[2][:, None]) > radius[2]))
    return int(np.count_nonzero(w)), int(np.count_nonzero((w > 0) & far))


@pytest.fixture(scope="module")
def lib():
    from fetal_t2mapping_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        from fetal_t2mapping_amd import build

        build.build()
    return _lib.load()


def _err(lib):
    return lib.t2fit_last_error().decode()


def _plan_host(lib, B, half):
    binv, radius = (C.c_double * 12)(), (C.c_int32 * 3)()
    rc = lib.t2fit_sr_plan_host((C.c_double * 12)(*np.asarray(B, np.float64).ravel()), (C.c_double * 3)(*half), binv, radius)
    return rc, np.array(binv).reshape(3, 4), tuple(radius)


def test_plan_box_covers_the_support_on_random_affines_by_brute_force(lib):
    rng = np.random.default_rng(44)
    hr_shape, lr_shape = (9, 8, 7), (6, 5, 4)
    total = 0
    for trial in range(24):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        lin = q @ np.diag(rng.uniform(0.2, 1.3, size=3)) if trial % 3 else np.diag(rng.uniform(0.2, 1.3, size=3))[:, rng.permutation(3)]
        B = np.empty((3, 4))
        B[:, :3] = lin
        B[:, 3] = np.array(lr_shape[::-1]) / 2.0 - lin @ (np.array(hr_shape[::-1]) / 2.0) + rng.uniform(-1, 1, size=3)
        for profile in K.PROFILE_NAMES:
            rel = float(rng.uniform(0.6, 2.5))
            _, hw = S.profile_params(profile, rel)
            box = S.plan_box(B, (1.0, 1.0, hw))
            assert np.allclose(box[0][:, :3] @ B[:, :3], np.eye(3), atol=1e-12) and min(box[1]) >= 2
            pairs, outside = _brute_force_box_check(B, hr_shape, lr_shape, profile, rel, box)
            assert outside == 0, (trial, profile)
            total += pairs
            rc, binv, radius = _plan_host(lib, B, (1.0, 1.0, hw))  # the library's host arithmetic is the same arithmetic
            assert rc == 0 and radius == box[1] and np.array_equal(binv, box[0])
            # the result does not depend on the box: a wider one gives the same bits
            x = rng.normal(size=hr_shape)
            wide = (box[0], tuple(r + 2 for r in box[1]))
            a = S.forward(x, B, lr_shape, profile, rel, out_dtype=np.float64)
            b = S.forward(x, B, lr_shape, profile, rel, out_dtype=np.float64, box=wide)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert total > 20000


def _tiny_problem(n_te=2, seed=45):
    """Three 12 x 12 x 4 stacks of 1 x 1 x 3 mm around one centre."""
    rng = np.random.default_rng(seed)
    geoms = {o: K.centred_stack(K.DIRECTIONS[o], (12, 12, 4), (1.0, 1.0, 3.0), (0.0, 0.0, 0.0)) for o in ("ax", "cor", "sag")}
    stacks = {o: rng.normal(500, 100, size=(n_te,) + geoms[o].shape).astype(np.float32) for o in geoms}
    return stacks, geoms


def test_weight_zero_one_iteration_is_one_back_projection_step():
    stacks, geoms = _tiny_problem()
    got, hi, info = S.reconstruct_sr(stacks, geoms, weight=0.0, n_iter=1, return_info=True)
    order, hi2, B, rels = S.sr_plan(geoms)
    x0 = R.reconstruct(stacks, geoms)[0]
    r = [S.forward(x0, B[s], stacks[o].shape[-3:], "box", rels[s], y=stacks[o])[0] for s, o in enumerate(order)]
    want = S.adjoint(r, info["N"], B, "box", rels, hi.shape, x=x0, tau=info["tau"])
    assert hi.GetSize() == hi2.GetSize() and got.dtype == np.float32 and np.array_equal(got, want)
    assert info["tau"] == 1.0 / sum(float(m) for m in info["column_max"]) and not np.array_equal(got, x0)
    assert np.array_equal(S.reconstruct_sr(stacks, geoms, weight=0.0, n_iter=0)[0], x0)  # x_0 is the averaged merge


def test_a_stack_wholly_outside_the_grid_changes_nothing():
    stacks, geoms = _tiny_problem()
    x0 = R.reconstruct(stacks, geoms)[0]
    far = K.centred_stack(K.DIRECTIONS["cor_oblique"], (12, 12, 4), (1.0, 1.0, 3.0), (900.0, -700.0, 40.0))
    more_s, more_g = dict(stacks, far=stacks["cor"] + 7.0), dict(geoms, far=far)
    kw = dict(weight=2.0, n_iter=2, prox_iter=3, x0=x0, return_info=True)
    a, _, ia = S.reconstruct_sr(stacks, geoms, **kw)
    b, _, ib = S.reconstruct_sr(more_s, more_g, **kw)
    assert len(ib["N"]) == 4 and np.all(ib["N"][3] == 0.0) and ib["column_max"][3] == 0.0 and ib["tau"] == ia["tau"]
    assert np.array_equal(a, b)
    # one stack alone is accepted too (the merge needs three); its default x_0 is its own linear resample
    one, g1 = S.reconstruct_sr({"cor": stacks["cor"]}, {"cor": geoms["cor"]}, fixed="cor", weight=0.0, n_iter=0)
    assert np.array_equal(one, R.resample(stacks["cor"], R.index_affine(g1, geoms["cor"]), g1.shape))


def test_python_refusals():
    stacks, geoms = _tiny_problem(1)
    B = R.index_affine(R.isotropic_geometry(geoms["ax"]), geoms["ax"])
    x = np.zeros(R.isotropic_geometry(geoms["ax"]).shape, np.float32)
    for bad in ({"profile": "gauss"}, {"rel_thickness": 0.0}, {"rel_thickness": -1.0}, {"rel_thickness": np.nan}):
        with pytest.raises(ValueError):
            S.forward(x, B, geoms["ax"].shape, **bad)
    with pytest.raises(ValueError, match="singular"):
        S.plan_box(np.zeros((3, 4)), (1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="finite"):
        S.plan_box(np.full((3, 4), np.nan), (1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="half-widths"):
        S.plan_box(np.eye(3, 4), (1.0, 1.0, 0.0))
    with pytest.raises(ValueError, match="between 1 and 6"):
        S.adjoint([], [], [], "box", 1.0, x.shape)
    with pytest.raises(ValueError, match="between 1 and 6"):
        S.sr_plan({str(i): geoms["ax"] for i in range(7)}, fixed="0")
    for bad in ({"fixed": "cor2"}, {"weight": -1.0}, {"weight": np.inf}, {"n_iter": -1}, {"prox_iter": 0}, {"thickness": 0.0},
                {"thickness": {"cor": -2.0}}, {"profile": "sinc"}, {"transforms": {"ax": np.eye(4)}}, {"x0": np.zeros((3, 2, 2, 2))}):
        with pytest.raises(ValueError):
            S.reconstruct_sr(stacks, geoms, **bad)
    with pytest.raises(ValueError, match="number of echoes"):
        S.reconstruct_sr(dict(stacks, cor=np.concatenate([stacks["cor"]] * 2)), geoms)
    far = K.centred_stack(K.DIRECTIONS["ax"], (12, 12, 4), (1.0, 1.0, 3.0), (900.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="nothing to reconstruct"):
        S.reconstruct_sr({"ax": stacks["ax"], "b": stacks["ax"]}, {"ax": geoms["ax"], "b": far}, stack_masks={"ax": np.zeros((4, 12, 12))})


def test_library_exports_the_symbols_and_refuses_bad_arguments_without_a_device(lib):
    from fetal_t2mapping_amd import _abi

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "t2fit.h")).read()
    for name in _abi.SR_SYMBOLS:
        assert hasattr(lib, name) and name in header and name in _abi.LOOKED_UP
    assert lib.t2fit_abi_version() == 5 and "#define T2FIT_SR_MAX_STACKS 6" in header
    assert (_abi.SR_PROFILE_BOX, _abi.SR_PROFILE_BSPLINE3, _abi.SR_MAX_STACKS) == (S.BOX, S.BSPLINE3, S.MAX_STACKS) == (0, 1, 6)
    eye = np.eye(3, 4)
    nan = eye.copy()
    nan[1, 2] = np.nan
    D = lambda a: (C.c_double * np.size(a))(*np.ravel(a))
    # the plan
    for B, half, text in ((nan, (1, 1, 1), "non-finite"), (np.zeros((3, 4)), (1, 1, 1), "singular"), (eye, (1, 0, 1), "half-widths"),
                          (eye, (1, 1, np.inf), "half-widths"), (eye * 1e-9, (1, 1, 1), "singular")):
        assert _plan_host(lib, B, half)[0] == _abi.E_INVALID and text in _err(lib), (text, _err(lib))
    assert lib.t2fit_sr_plan_host(None, D((1, 1, 1)), D(eye), (C.c_int32 * 3)()) == _abi.E_INVALID and "NULL" in _err(lib)
    # the workspace: up(4 n_vol |H|) + sum_s up(8 |L_s|) + up(4 n_vol |L_s|)
    up = lambda v: (v + 255) // 256 * 256
    lo = (C.c_int32 * 6)(3, 8, 9, 5, 19, 21)
    need = C.c_size_t(0)
    assert lib.t2fit_sr_workspace_bytes(2, lo, 10, 9, 11, 3, C.byref(need)) == 0
    assert need.value == up(4 * 3 * 990) + up(8 * 216) + up(4 * 3 * 216) + up(8 * 1995) + up(4 * 3 * 1995)
    for args, text in (((0, lo, 10, 9, 11, 3), "n_stacks"), ((7, lo, 10, 9, 11, 3), "n_stacks"), ((2, lo, 0, 9, 11, 3), ">= 1"),
                       ((2, lo, 10, 9, 11, 0), ">= 1"), ((2, (C.c_int32 * 6)(3, 8, 9, 5, -1, 21), 10, 9, 11, 3), ">= 1"),
                       ((2, None, 10, 9, 11, 3), "NULL")):
        assert lib.t2fit_sr_workspace_bytes(*args, C.byref(need)) == _abi.E_INVALID and text in _err(lib), text
    assert lib.t2fit_sr_workspace_bytes(2, lo, 10, 9, 11, 3, None) == _abi.E_INVALID
    # forward: the pointers are never dereferenced, every call is refused first
    rad = (C.c_int32 * 3)(2, 2, 3)

    def fwd(x=0x1000, h=(10, 9, 11), n_vol=2, B=eye, Binv=eye, radius=rad, profile=0, thick=1.2, y=0x2000, mask=0x3000, lsz=(3, 8, 9),
            out=0x4000, N=0x5000):
        return lib.t2fit_sr_forward_dev(x, *h, n_vol, None if B is None else D(B), None if Binv is None else D(Binv), radius, profile,
                                        thick, y, mask, *lsz, out, N, None)

    for kw, text in (({"B": None}, "NULL"), ({"Binv": None}, "NULL"), ({"radius": None}, "NULL"), ({"out": None, "x": None, "y": None, "N": None}, "both NULL"),
                     ({"x": None}, "go together"), ({"out": None}, "go together"), ({"x": None, "out": None}, "y_dev needs"),
                     ({"h": (10, 0, 11)}, ">= 1"), ({"lsz": (3, 8, -2)}, ">= 1"), ({"n_vol": 0}, ">= 1"), ({"B": nan}, "non-finite"),
                     ({"Binv": nan}, "non-finite"), ({"radius": (C.c_int32 * 3)(2, 0, 3)}, "radius"), ({"profile": 2}, "unknown profile"),
                     ({"profile": -1}, "unknown profile"), ({"thick": 0.0}, "thickness"), ({"thick": -1.0}, "thickness"),
                     ({"thick": np.nan}, "thickness"), ({"thick": np.inf}, "thickness"), ({"x": 0x1002}, "aligned"),
                     ({"y": 0x2001}, "aligned"), ({"out": 0x4002}, "aligned"), ({"N": 0x5004}, "aligned"), ({"out": 0x1000}, "must not be x_dev")):
        assert fwd(**kw) == _abi.E_INVALID, kw
        assert text in _err(lib), (kw, _err(lib))
    # adjoint
    P = lambda *v: (C.c_void_p * len(v))(*v)

    def adj(n_s=2, r=P(0x1000, 0x2000), N=P(0x3000, 0x4000), mask=None, lo=lo, B=np.concatenate([eye, eye]), profile=(0, 1),
            thick=(1.0, 1.5), x=0x6000, tau=0.5, out=0x7000, h=(10, 9, 11), n_vol=3):
        return lib.t2fit_sr_adjoint_dev(n_s, r, N, mask, lo, None if B is None else D(B), (C.c_int32 * 2)(*profile), D(thick), x, tau, out,
                                        *h, n_vol, None)

    for kw, text in (({"r": None}, "NULL"), ({"N": None}, "NULL"), ({"lo": None}, "NULL"), ({"B": None}, "NULL"), ({"out": None}, "NULL"),
                     ({"n_s": 0}, "n_stacks"), ({"n_s": 7}, "n_stacks"), ({"h": (10, 9, 0)}, ">= 1"), ({"n_vol": 0}, ">= 1"),
                     ({"tau": np.nan}, "tau"), ({"tau": np.inf}, "tau"), ({"x": 0x6001}, "aligned"), ({"out": 0x7002}, "aligned"),
                     ({"r": P(0x1000, None)}, "pointer is NULL"), ({"N": P(None, 0x4000)}, "pointer is NULL"),
                     ({"r": P(0x1001, 0x2000)}, "aligned"), ({"N": P(0x3000, 0x4004)}, "aligned"), ({"r": P(0x1000, 0x7000)}, "is out_dev"),
                     ({"lo": (C.c_int32 * 6)(3, 8, 9, 0, 19, 21)}, ">= 1"), ({"B": np.concatenate([eye, nan])}, "non-finite"),
                     ({"profile": (0, 5)}, "unknown profile"), ({"thick": (1.0, 0.0)}, "thickness"), ({"thick": (np.nan, 1.0)}, "thickness")):
        assert adj(**kw) == _abi.E_INVALID, kw
        assert text in _err(lib), (kw, _err(lib))


def test_command_line_flags_parse_and_are_refused_where_they_have_no_effect(tmp_path, capsys, monkeypatch):
    import pandas as pd

    from fetal_t2mapping_amd import cli, recon

    base = ["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo", "--lf"]
    args = recon.parse_arguments(base)
    assert args.recon_method == "average" and args.sr_args is None
    args = recon.parse_arguments(base + ["--recon_method", "sr"])
    assert args.sr_args == {"weight": S.DEFAULT_WEIGHT, "n_iter": S.DEFAULT_N_ITER, "profile": "box", "thickness": None}
    args = recon.parse_arguments(base + ["--recon_method", "sr", "--sr_weight", "3.5", "--sr_iter", "4", "--sr_profile", "bspline3",
                                         "--sr_thickness", "4.5"])
    assert args.sr_args == {"weight": 3.5, "n_iter": 4, "profile": "bspline3", "thickness": 4.5}
    for bad in (["--sr_weight", "3"], ["--sr_iter", "2"], ["--sr_profile", "box"], ["--sr_thickness", "4"],
                ["--recon_method", "sr", "--sr_weight", "-1"], ["--recon_method", "sr", "--sr_iter", "-2"],
                ["--recon_method", "sr", "--sr_thickness", "0"], ["--recon_method", "sr", "--sr_profile", "gauss"],
                ["--recon_method", "median"]):
        with pytest.raises(SystemExit):
            recon.parse_arguments(base + bad)
    fit = base + ["--gaussian", "--sim", "s"]
    assert cli.parse_arguments(fit + ["--reconstruct"]).reconstruct_args == {"fixed": "ax", "res": 1.0, "transforms_dir": None}
    args = cli.parse_arguments(fit + ["--reconstruct", "--recon_method", "sr", "--recon_sr_iter", "2"])
    assert args.reconstruct_args["sr"] == {"weight": S.DEFAULT_WEIGHT, "n_iter": 2, "profile": "box", "thickness": None}
    for bad in (["--recon_method", "sr"], ["--reconstruct", "--recon_sr_weight", "2"], ["--reconstruct", "--recon_method", "sr", "--recon_sr_weight", "nan"]):
        with pytest.raises(SystemExit):
            cli.parse_arguments(fit + bad)
    capsys.readouterr()
    # sr is a --reconstruct: the same refusal on a volume that several ranks share
    monkeypatch.setattr(cli, "_dist_env", lambda: (0, 2, 0))  # two ranks, one subject
    md = pd.DataFrame([{"prj": "prj-1", "sub": "sub-1", "ses": "ses-1", "run": "run-01", "EchoTime": 0.114}])
    with pytest.raises(ValueError, match="--reconstruct is not run on a volume that is shared by several ranks"):
        cli.process_t2maps(md, str(tmp_path), [114], None, {}, False, True, True, False, False, "s", reconstruct=args.reconstruct_args)


def test_super_resolution_is_closer_to_the_truth_than_the_averaged_merge_on_the_phantom():
    stacks, geoms, truth, grid, _, _ = K.phantom()
    x, hi, info = K.phantom_statement(S.DEFAULT_N_ITER, S.DEFAULT_PROX_ITER)
    merged, hi_m = R.reconstruct(stacks, geoms)
    assert hi.GetOrigin() == hi_m.GetOrigin() and x.shape == merged.shape and x.dtype == np.float32
    sr, avg = K.interior_rmse(x, truth, grid, hi.GetOrigin()), K.interior_rmse(merged, truth, grid, hi.GetOrigin())
    print(f"interior RMSE: super-resolution {sr:.3f}, averaged merge {avg:.3f}, tau {info['tau']}")
    assert sr < avg
