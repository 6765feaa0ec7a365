"""The super-resolution operator with a rigid pose per slice as fetal_t2mapping_amd/_sr.py states it (forward_slices,
adjoint_slices, reconstruct_sr(slice_transforms=...)), without a device: a dense matrix written pair by pair with an affine
per slice, equal slice affines against the stack-wise statement bit for bit, adjointness to the derived bound, the
accumulation order by slice index, the refusals of the table call (the library checks its arguments without a device) and
of the Python layer, the files of slice transforms, the command-line flags and the recovery of a phantom that moved
between slices."""
import ctypes as C
import os

import numpy as np
import pytest

import sr_cases as K
import sr_slice_cases as L
from fetal_t2mapping_amd import _resample as R
from fetal_t2mapping_amd import _sr as S


@pytest.mark.parametrize("name,profile", [("ax", "box"), ("sag_oblique", "bspline3"), ("cor_oblique", "box"), ("cor", "bspline3")])
def test_statement_equals_a_dense_matrix_with_an_affine_per_slice(name, profile):
    c, Bs = L.moved_case(name)
    hr, lr = c.hr.shape, c.stack.shape
    assert hr == (10, 9, 11) and lr == (3, 8, 9) and not np.array_equal(Bs[0], Bs[1])
    W, N = L.dense_matrix_slices(Bs, hr, lr, profile, c.rel)
    n_h, n_l = W.shape[1], W.shape[0]
    assert np.count_nonzero(W) > 4 * n_l and np.count_nonzero(N > 0) > n_l // 2
    n = S.forward_slices(None, Bs, lr, profile, c.rel, hr_shape=hr)[1]
    assert n.dtype == np.float64 and np.array_equal(n.ravel(), N)
    rng = np.random.default_rng(71)
    x, r = rng.normal(size=n_h), rng.normal(size=n_l)
    for mask in (None, c.mask):
        cm = (N > 0) if mask is None else (N > 0) & (mask.ravel() != 0)
        f, n2 = S.forward_slices(x.reshape(hr), Bs, lr, profile, c.rel, mask=mask, out_dtype=np.float64)
        assert np.array_equal(n2.ravel(), N) and np.array_equal(f.ravel(), K.dense_forward(W, N, x, cm))
        a = S.adjoint_slices([r.reshape(lr)], [n], [Bs], profile, c.rel, hr, masks=None if mask is None else [mask], out_dtype=np.float64)
        assert np.array_equal(a.ravel(), K.dense_adjoint(W, N, r, cm))
    # every entry both ways: the unit vectors give w / N per pair
    counts = N > 0
    want = np.where(counts[:, None], W / np.where(counts, N, 1.0)[:, None], 0.0)
    got = S.forward_slices(np.eye(n_h).reshape((n_h,) + hr), Bs, lr, profile, c.rel, out_dtype=np.float64)[0]
    assert np.array_equal(got.reshape(n_h, n_l).T, want)
    back = S.adjoint_slices([np.eye(n_l).reshape((n_l,) + lr)], [n], [Bs], profile, c.rel, hr, out_dtype=np.float64)
    assert np.array_equal(back.reshape(n_l, n_h), want)
    # a box of samples and a box of voxels give the bits of the whole
    part = S.forward_slices(x.reshape(hr), Bs, lr, profile, c.rel, mask=c.mask, start=(2, 1, 1), shape=(2, 5, 4), out_dtype=np.float64)
    whole = S.forward_slices(x.reshape(hr), Bs, lr, profile, c.rel, mask=c.mask, out_dtype=np.float64)
    assert np.array_equal(part[0], whole[0][1:3, 1:6, 2:6]) and np.array_equal(part[1], whole[1][1:3, 1:6, 2:6])
    a = S.adjoint_slices([r.reshape(lr)], [n], [Bs], profile, c.rel, hr, x=x.reshape(hr), tau=0.3, out_dtype=np.float64)
    b = S.adjoint_slices([r.reshape(lr)], [n], [Bs], profile, c.rel, hr, x=x.reshape(hr), tau=0.3, start=(3, 2, 1), shape=(4, 5, 6),
                         out_dtype=np.float64)
    assert np.array_equal(b, a[1:5, 2:7, 3:9])


@pytest.mark.parametrize("profile", K.PROFILE_NAMES)
@pytest.mark.parametrize("name", ["ax", "cor_oblique", "sag"])
def test_equal_slice_affines_reproduce_the_stack_wise_statement_bit_for_bit(name, profile):
    c = K.small_case(name)
    hr, lr = c.hr.shape, c.stack.shape
    Bs = np.repeat(c.B[None], lr[0], axis=0)
    rng = np.random.default_rng(72)
    x = rng.normal(500, 200, size=(2,) + hr).astype(np.float32)
    y = rng.normal(500, 200, size=(2,) + lr).astype(np.float32)
    assert np.any(c.mask == 0)
    want, wn = S.forward(x, c.B, lr, profile, c.rel, y=y, mask=c.mask)
    got, gn = S.forward_slices(x, Bs, lr, profile, c.rel, y=y, mask=c.mask)
    assert np.array_equal(gn, wn) and np.array_equal(got, want) and np.any(want != 0)
    a = S.adjoint([want], [wn], [c.B], profile, c.rel, hr, masks=[c.mask], x=x, tau=0.3)
    b = S.adjoint_slices([want], [wn], [Bs], profile, c.rel, hr, masks=[c.mask], x=x, tau=0.3)
    assert np.array_equal(a, b) and not np.array_equal(a, x)
    assert np.array_equal(S.adjoint([want], [wn], [c.B], profile, c.rel, hr), S.adjoint_slices([want], [wn], [Bs], profile, c.rel, hr))


@pytest.mark.parametrize("profile", K.PROFILE_NAMES)
@pytest.mark.parametrize("name", sorted(K.DIRECTIONS))
def test_forward_and_adjoint_are_adjoint_to_the_rounding_bound(name, profile):
    """The bound of test_sr_host: <A x, r> and <x, A^T r> are two groupings of the same terms t = w x r / N over the pairs
    that count, each off the exact sum by less than n_terms 2^-53 sum |t|, so they differ by less than n_terms 2^-52 sum |t|."""
    c, Bs = L.moved_case(name)
    hr, lr = c.hr.shape, c.stack.shape
    rng = np.random.default_rng(73)
    x, r = rng.normal(size=hr), rng.normal(size=lr)
    ax, n = S.forward_slices(x, Bs, lr, profile, c.rel, mask=c.mask, out_dtype=np.float64)
    atr = S.adjoint_slices([r], [n], [Bs], profile, c.rel, hr, masks=[c.mask], out_dtype=np.float64)
    counts = (n > 0) & (c.mask != 0)
    w = np.concatenate([K.weights_by_broadcast(Bs[k], hr, lr, profile, c.rel).reshape(lr + (-1,))[k].reshape(lr[1] * lr[2], -1)
                        for k in range(lr[0])])[counts.ravel()]
    terms = np.abs(w * x.ravel()[None, :] * (r[counts] / n[counts])[:, None])
    n_terms = int(np.count_nonzero(w))
    bound = n_terms * 2.0 ** -52 * float(terms.sum())
    lhs, rhs = float(np.sum(ax * r)), float(np.sum(x * atr))
    print(f"{name} {profile}: |lhs - rhs| = {abs(lhs - rhs):.3e}, bound {bound:.3e}, {n_terms} terms")
    assert counts.sum() > 100 and n_terms > 1000 and abs(lhs - rhs) <= bound


@pytest.mark.parametrize("profile", K.PROFILE_NAMES)
def test_the_adjoint_accumulates_by_slice_index_not_by_position(profile):
    """Slices 0 and 2 swap places in space and slice 1 takes the very pose of (the moved) slice 0's neighbour, so two slices
    lie in one pose: the accumulator still runs in ascending index, which is the order of the dense rows."""
    c = K.small_case("ax_oblique")
    hr, lr = c.hr.shape, c.stack.shape
    normal = np.asarray(K.DIRECTIONS["ax_oblique"])[:, 2] * 3.0  # one slice spacing along the stack's normal
    shift = lambda n: np.block([[np.eye(3), (n * normal)[:, None]], [np.zeros((1, 3)), np.ones((1, 1))]])
    # slice k images the voxels whose u_z is near k: u_z - 2 puts slice 0 where slice 2 was, u_z + 2 the reverse
    t = np.stack([shift(-2.0) @ K.rigid(), K.rigid(), shift(2.0) @ K.rigid()])
    Bs = S.slice_affines(c.hr, c.stack, t)
    assert np.allclose(Bs[0][2, 3] + 2.0, Bs[1][2, 3]) and np.allclose(Bs[2][2, 3] - 2.0, Bs[1][2, 3])
    same = np.stack([K.rigid(), shift(1.0) @ K.rigid(), K.rigid()])  # slice 1 images what slice 0 images
    for poses in (Bs, S.slice_affines(c.hr, c.stack, same)):
        W, N = L.dense_matrix_slices(poses, hr, lr, profile, c.rel)
        rows = W.reshape(lr + (-1,))
        shared = np.count_nonzero((rows[0].sum(0) > 0) & (rows[1].sum(0) + rows[2].sum(0) > 0))
        assert shared > 50  # voxels that take terms from several slices: their order matters
        rng = np.random.default_rng(74)
        r = rng.normal(size=lr)
        n = S.forward_slices(None, poses, lr, profile, c.rel, hr_shape=hr)[1]
        got = S.adjoint_slices([r], [n], [poses], profile, c.rel, hr, out_dtype=np.float64)
        assert np.array_equal(n.ravel(), N) and np.array_equal(got.ravel(), K.dense_adjoint(W, N, r.ravel(), N > 0))
    # in space slice 2 now comes first: summing in that order gives other bits somewhere, so the test can tell the two orders
    W, N = L.dense_matrix_slices(Bs, hr, lr, profile, c.rel)
    r = np.random.default_rng(74).normal(size=lr).ravel()
    by_index = K.dense_adjoint(W, N, r, N > 0)
    flip = np.arange(len(N)).reshape(lr)[::-1].ravel()
    by_position = K.dense_adjoint(W[flip], N[flip], r[flip], (N > 0)[flip])
    assert not np.array_equal(by_index, by_position) and np.allclose(by_index, by_position, rtol=1e-12, atol=1e-12)


def test_compose_slice_transforms_turns_every_slice_about_its_own_centre():
    c = K.small_case("cor_oblique")
    p = L.motion(3, 6.0, 1.5, 75)
    t = S.compose_slice_transforms(K.rigid(), p, c.stack)
    assert t.shape == (3, 4, 4)
    m, o = R._index_to_point(c.stack)
    for k in range(3):
        centre = o + m @ np.array([4.0, 3.5, float(k)])
        motion = t[k] @ np.linalg.inv(K.rigid())
        assert np.allclose(motion[:3, :3] @ motion[:3, :3].T, np.eye(3), atol=1e-14)
        assert np.allclose(motion[:3, :3] @ centre + motion[:3, 3], centre + p[k, 3:], atol=1e-12)  # the centre only translates
    zero = S.compose_slice_transforms(None, np.zeros((3, 6)), c.stack)
    assert np.array_equal(zero, np.repeat(np.eye(4)[None], 3, axis=0))
    assert np.array_equal(S.slice_affines(c.hr, c.stack, zero)[1], R.index_affine(c.hr, c.stack, np.eye(4)))


def _tiny_problem(n_te=2, seed=76):
    rng = np.random.default_rng(seed)
    geoms = {o: K.centred_stack(K.DIRECTIONS[o], (12, 12, 4), (1.0, 1.0, 3.0), (0.0, 0.0, 0.0)) for o in ("ax", "cor", "sag")}
    stacks = {o: rng.normal(500, 100, size=(n_te,) + geoms[o].shape).astype(np.float32) for o in geoms}
    return stacks, geoms


def test_reconstruct_sr_with_slice_transforms_runs_on_the_slice_operators():
    stacks, geoms = _tiny_problem()
    t = {"cor": K.rigid(0.5)}
    kw = dict(weight=2.0, n_iter=2, prox_iter=3, transforms=t, return_info=True)
    plain, hi, pinfo = S.reconstruct_sr(stacks, geoms, **kw)
    # every slice at its stack's transform (the fixed stack: the identity): the bits of the stack-wise loop
    same = {"ax": np.repeat(np.eye(4)[None], 4, axis=0), "cor": np.repeat(t["cor"][None], 4, axis=0)}
    got, hi2, info = S.reconstruct_sr(stacks, geoms, slice_transforms=same, **kw)
    assert hi2.GetSize() == hi.GetSize() and info["tau"] == pinfo["tau"] and np.array_equal(got, plain)
    assert np.array_equal(S.reconstruct_sr(stacks, geoms, slice_transforms={}, **kw)[0], plain)
    # poses of their own: one step by hand from the merge
    poses = {"ax": S.compose_slice_transforms(None, L.motion(4, 3.0, 1.0, 77), geoms["ax"]),
             "sag": S.compose_slice_transforms(None, L.motion(4, 3.0, 1.0, 78), geoms["sag"])}
    got, hi, info = S.reconstruct_sr(stacks, geoms, weight=0.0, n_iter=1, transforms=t, slice_transforms=poses, return_info=True)
    order, _, B, rels = S.sr_plan(geoms, transforms=t)
    Bs = [S.slice_affines(hi, geoms["ax"], poses["ax"]), np.repeat(B[1][None], 4, axis=0), S.slice_affines(hi, geoms["sag"], poses["sag"])]
    assert order == ["ax", "cor", "sag"]
    x0 = R.reconstruct(stacks, geoms, transforms=t)[0]
    r = [S.forward_slices(x0, Bs[s], stacks[o].shape[-3:], "box", rels[s], y=stacks[o])[0] for s, o in enumerate(order)]
    for s in range(3):
        assert np.array_equal(info["N"][s], S.forward_slices(None, Bs[s], stacks[order[s]].shape[-3:], "box", rels[s], hr_shape=hi.shape)[1])
    want = S.adjoint_slices(r, info["N"], Bs, "box", rels, hi.shape, x=x0, tau=info["tau"])
    assert np.array_equal(got, want) and not np.array_equal(got, x0) and info["tau"] != pinfo["tau"]


def test_python_refusals():
    stacks, geoms = _tiny_problem(1)
    hi = R.isotropic_geometry(geoms["ax"])
    good = np.repeat(np.eye(4)[None], 4, axis=0)
    nan = good.copy()
    nan[2, 1, 3] = np.nan
    for bad in (good[:3], good[:, :3], np.eye(4), nan):
        with pytest.raises(ValueError):
            S.slice_affines(hi, geoms["ax"], bad)
    for bad in ({"ax": good[:3]}, {"cor": nan}, {"cor2": good}, {"ax": np.eye(4)}):
        with pytest.raises(ValueError):
            S.reconstruct_sr(stacks, geoms, slice_transforms=bad)
    with pytest.raises(ValueError, match="unknown|given per stack"):
        S.reconstruct_sr(stacks, geoms, slice_transforms={"oblique": good})
    for bad in (np.zeros((3, 6)), np.zeros((4, 5)), np.full((4, 6), np.inf)):
        with pytest.raises(ValueError):
            S.compose_slice_transforms(None, bad, geoms["ax"])
    with pytest.raises(ValueError):
        S.compose_slice_transforms(np.eye(3), np.zeros((4, 6)), geoms["ax"])
    B = np.repeat(R.index_affine(hi, geoms["ax"])[None], 4, axis=0)
    x = np.zeros(hi.shape, np.float32)
    for bad in (B[:3], B[0]):
        with pytest.raises(ValueError):
            S.forward_slices(x, bad, geoms["ax"].shape)
        with pytest.raises(ValueError):
            S.adjoint_slices([stacks["ax"][0]], [np.ones(geoms["ax"].shape)], [bad], "box", 1.0, hi.shape)
    with pytest.raises(ValueError, match="between 1 and 6"):
        S.adjoint_slices([], [], [], "box", 1.0, hi.shape)
    with pytest.raises(ValueError, match="singular"):
        S.forward_slices(x, np.zeros((4, 3, 4)), geoms["ax"].shape)


@pytest.fixture(scope="module")
def lib():
    from fetal_t2mapping_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        from fetal_t2mapping_amd import build

        build.build()
    return _lib.load()


def _err(lib):
    return lib.t2fit_last_error().decode()


def test_library_packs_the_table_and_refuses_bad_arguments_without_a_device(lib):
    from fetal_t2mapping_amd import _abi

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "t2fit.h")).read()
    for name in _abi.SR_SLICE_SYMBOLS:
        assert hasattr(lib, name) and name + "(" in header and name in _abi.LOOKED_UP and name not in _abi.SR_SYMBOLS
    assert lib.t2fit_abi_version() == 5 and "#define T2FIT_SR_SLICE_RECORD_BYTES 208" in header and _abi.SR_SLICE_RECORD_BYTES == 208
    D = lambda a: (C.c_double * np.size(a))(*np.ravel(a))
    _, Bs = L.moved_case("sag_oblique")
    need = C.c_size_t(0)
    assert lib.t2fit_sr_slice_table_bytes(3, C.byref(need)) == 0 and need.value == 3 * 208
    assert lib.t2fit_sr_slice_table_bytes(0, C.byref(need)) == _abi.E_INVALID and ">= 1" in _err(lib)
    assert lib.t2fit_sr_slice_table_bytes(3, None) == _abi.E_INVALID and "NULL" in _err(lib)
    # the layout: B, Binv and the radii of t2fit_sr_plan_host per slice, a zero pad word; nothing beyond the table is written
    for profile, rel in (("box", 4.0 / 3.0), ("bspline3", 1.7)):
        raw = np.full(3 * 208 + 16, 0xAB, np.uint8)
        rc = lib.t2fit_sr_slice_table_host(3, D(Bs), _abi.SR_PROFILES[profile], rel, raw.ctypes.data_as(C.c_void_p), 3 * 208)
        assert rc == 0, _err(lib)
        assert np.all(raw[3 * 208:] == 0xAB)
        for k in range(3):
            rec = raw[208 * k:208 * (k + 1)]
            binv, radius = S.plan_box(Bs[k], (1.0, 1.0, S.profile_params(profile, rel)[1]))
            assert np.array_equal(rec[:96].view(np.float64).reshape(3, 4), Bs[k])
            assert np.array_equal(rec[96:192].view(np.float64).reshape(3, 4), binv)
            assert tuple(rec[192:208].view(np.int32)) == radius + (0,)
    # refusals; a bad slice leaves the table untouched
    nan, singular, tiny = Bs.copy(), Bs.copy(), Bs.copy()
    nan[2, 1, 2] = np.inf
    singular[1] = 0.0
    tiny[0] = Bs[0] * 1e-9
    raw = np.full(3 * 208, 0xAB, np.uint8)
    table = raw.ctypes.data_as(C.c_void_p)

    def pack(lz=3, B=Bs, profile=0, thick=1.2, table=table, nbytes=3 * 208):
        return lib.t2fit_sr_slice_table_host(lz, None if B is None else D(B), profile, thick, table, nbytes)

    for kw, text in (({"B": None}, "NULL"), ({"table": None}, "NULL"), ({"lz": 0}, ">= 1"), ({"nbytes": 3 * 208 - 1}, "smaller"),
                     ({"profile": 2}, "unknown profile"), ({"thick": 0.0}, "thickness"), ({"thick": np.nan}, "thickness"),
                     ({"B": nan}, "slice 2: B has a non-finite"), ({"B": singular}, "slice 1: B is singular"),
                     ({"B": tiny}, "slice 0: B is singular")):
        assert pack(**kw) == _abi.E_INVALID, kw
        assert text in _err(lib), (kw, _err(lib))
        assert np.all(raw == 0xAB), kw
    # forward: the pointers are never dereferenced, every call is refused first
    def fwd(x=0x1000, h=(10, 9, 11), n_vol=2, table=0x8000, profile=0, thick=1.2, y=0x2000, mask=0x3000, lsz=(3, 8, 9), out=0x4000,
            N=0x5000):
        return lib.t2fit_sr_slice_forward_dev(x, *h, n_vol, table, profile, thick, y, mask, *lsz, out, N, None)

    for kw, text in (({"table": None}, "table_dev is NULL"), ({"table": 0x8004}, "aligned to 8"),
                     ({"out": None, "x": None, "y": None, "N": None}, "both NULL"), ({"x": None}, "go together"),
                     ({"out": None}, "go together"), ({"x": None, "out": None}, "y_dev needs"), ({"h": (10, 0, 11)}, ">= 1"),
                     ({"lsz": (3, 8, -2)}, ">= 1"), ({"n_vol": 0}, ">= 1"), ({"profile": 2}, "unknown profile"),
                     ({"thick": 0.0}, "thickness"), ({"thick": np.inf}, "thickness"), ({"x": 0x1002}, "aligned"),
                     ({"y": 0x2001}, "aligned"), ({"out": 0x4002}, "aligned"), ({"N": 0x5004}, "aligned"), ({"out": 0x1000}, "must not be x_dev")):
        assert fwd(**kw) == _abi.E_INVALID, kw
        assert text in _err(lib), (kw, _err(lib))
    # adjoint
    P = lambda *v: (C.c_void_p * len(v))(*v)
    lo = (C.c_int32 * 6)(3, 8, 9, 5, 19, 21)

    def adj(n_s=2, r=P(0x1000, 0x2000), N=P(0x3000, 0x4000), mask=None, tables=P(0x8000, 0x9000), lo=lo, profile=(0, 1), thick=(1.0, 1.5),
            x=0x6000, tau=0.5, out=0x7000, h=(10, 9, 11), n_vol=3):
        return lib.t2fit_sr_slice_adjoint_dev(n_s, r, N, mask, tables, lo, (C.c_int32 * 2)(*profile), D(thick), x, tau, out, *h, n_vol, None)

    for kw, text in (({"r": None}, "NULL"), ({"N": None}, "NULL"), ({"tables": None}, "NULL"), ({"lo": None}, "NULL"), ({"out": None}, "NULL"),
                     ({"tables": P(0x8000, None)}, "slice table pointer is NULL"), ({"tables": P(0x8002, 0x9000)}, "aligned to 8"),
                     ({"n_s": 0}, "n_stacks"), ({"n_s": 7}, "n_stacks"), ({"h": (10, 9, 0)}, ">= 1"), ({"n_vol": 0}, ">= 1"),
                     ({"tau": np.nan}, "tau"), ({"x": 0x6001}, "aligned"), ({"out": 0x7002}, "aligned"),
                     ({"r": P(0x1000, None)}, "pointer is NULL"), ({"N": P(None, 0x4000)}, "pointer is NULL"),
                     ({"r": P(0x1001, 0x2000)}, "aligned"), ({"N": P(0x3000, 0x4004)}, "aligned"), ({"r": P(0x1000, 0x7000)}, "is out_dev"),
                     ({"lo": (C.c_int32 * 6)(3, 8, 9, 0, 19, 21)}, ">= 1"), ({"profile": (0, 5)}, "unknown profile"),
                     ({"thick": (1.0, 0.0)}, "thickness")):
        assert adj(**kw) == _abi.E_INVALID, kw
        assert text in _err(lib), (kw, _err(lib))


def test_slice_transform_files_round_trip_bit_for_bit_and_name_a_bad_file(tmp_path):
    from fetal_t2mapping_amd import recon

    _, geoms = _tiny_problem(1)
    acq = {"sub": "sub-001", "ses": "ses-01", "EchoTime": 0.114}
    rng = np.random.default_rng(79)
    poses = {o: S.compose_slice_transforms(K.rigid(), rng.normal(0, 0.05, size=(4, 6)) * np.pi, geoms[o]) for o in ("ax", "sag")}
    paths = recon.save_slice_transforms(str(tmp_path), acq, poses)
    assert sorted(os.path.basename(p) for p in paths) == ["sub-001_ses-01_te-114_ax_slices.txt", "sub-001_ses-01_te-114_sag_slices.txt"]
    assert len(open(paths[0]).read().splitlines()) == 4 and len(open(paths[0]).readline().split()) == 16
    back = recon.load_slice_transforms(str(tmp_path), acq, geoms)
    assert sorted(back) == ["ax", "sag"] and all(np.array_equal(back[o], poses[o]) and back[o].shape == (4, 4, 4) for o in back)
    assert recon.load_slice_transforms(None, acq, geoms) == {}
    # the echo's own file goes before the file of the (sub, ses), as with load_transforms
    other = dict(acq, EchoTime=0.202)
    assert recon.load_slice_transforms(str(tmp_path), other, geoms) == {}
    os.rename(paths[1], os.path.join(str(tmp_path), "sub-001_ses-01_sag_slices.txt"))
    assert sorted(recon.load_slice_transforms(str(tmp_path), other, geoms)) == ["sag"]
    assert sorted(recon.load_slice_transforms(str(tmp_path), acq, geoms)) == ["ax", "sag"]
    # a file whose row count is not the stack's slice count
    np.savetxt(paths[0], poses["ax"][:3].reshape(3, 16), fmt="%.17g")
    with pytest.raises(ValueError, match=r"te-114_ax_slices\.txt: 3 rows, but stack 'ax' has 4 slices"):
        recon.load_slice_transforms(str(tmp_path), acq, geoms)
    np.savetxt(paths[0], poses["ax"].reshape(4, 16)[:, :12], fmt="%.17g")
    with pytest.raises(ValueError, match=r"te-114_ax_slices\.txt: expected rows of 16"):
        recon.load_slice_transforms(str(tmp_path), acq, geoms)
    with pytest.raises(ValueError):
        recon.save_slice_transforms(str(tmp_path), acq, {"ax": np.eye(4)})


def test_command_line_flags_parse_and_are_refused_without_the_sr_method(tmp_path):
    from fetal_t2mapping_amd import cli, recon

    base = ["--path", str(tmp_path), "--csv", "x.csv", "--in_vivo", "--lf"]
    args = recon.parse_arguments(base + ["--recon_method", "sr", "--sr_slice_transforms", "poses"])
    assert args.sr_args == {"weight": S.DEFAULT_WEIGHT, "n_iter": S.DEFAULT_N_ITER, "profile": "box", "thickness": None,
                            "slice_transforms_dir": "poses"}
    assert "slice_transforms_dir" not in recon.parse_arguments(base + ["--recon_method", "sr"]).sr_args
    for bad in (["--sr_slice_transforms", "poses"], ["--recon_method", "average", "--sr_slice_transforms=poses"]):
        with pytest.raises(SystemExit):
            recon.parse_arguments(base + bad)
    fit = base + ["--gaussian", "--sim", "s"]
    args = cli.parse_arguments(fit + ["--reconstruct", "--recon_method", "sr", "--recon_sr_slice_transforms", "poses"])
    assert args.reconstruct_args["sr"]["slice_transforms_dir"] == "poses"
    for bad in (["--reconstruct", "--recon_sr_slice_transforms", "poses"], ["--recon_sr_slice_transforms", "poses"]):
        with pytest.raises(SystemExit):
            cli.parse_arguments(fit + bad)


RECOVERY_RATIO = 0.765  # measured with the statement: see the docstring below


def test_the_slice_poses_recover_a_phantom_that_moved_between_slices():
    """``sr_cases.phantom()``'s truth (48^3, its first echo), acquired through the operator itself with a rigid pose per
    slice about the slice's centre, components uniform in +-4 degrees / +-2 mm (seed 64), Rician noise of sigma 15; 8
    iterations with the defaults.  Measured with this statement, interior RMSE against the truth: averaged merge 246.19,
    reconstruct_sr without the poses 247.38, with the true poses 188.32, ratio 188.32 / 246.19 = 0.765.  The bound is that
    ratio + 0.05 for another noise draw."""
    stacks, geoms, truth, grid, poses = L.moved_phantom()
    aware, hi, info = L.moved_statement(S.DEFAULT_N_ITER, S.DEFAULT_PROX_ITER, True)
    plain, _, pinfo = L.moved_statement(S.DEFAULT_N_ITER, S.DEFAULT_PROX_ITER, False)
    merged, hi_m = R.reconstruct(stacks, geoms)
    assert hi.GetOrigin() == hi_m.GetOrigin() and aware.shape == merged.shape == (1, 48, 48, 48) and aware.dtype == np.float32
    rmse = {k: K.interior_rmse(v, truth, grid, hi.GetOrigin()) for k, v in (("aware", aware), ("plain", plain), ("merge", merged))}
    ratio = rmse["aware"] / min(rmse["merge"], rmse["plain"])
    print(f"interior RMSE: merge {rmse['merge']:.3f}, without the poses {rmse['plain']:.3f}, with them {rmse['aware']:.3f}, "
          f"ratio {ratio:.4f}, tau {info['tau']} / {pinfo['tau']}")
    assert rmse["aware"] < rmse["merge"] and rmse["aware"] < rmse["plain"]
    assert ratio <= RECOVERY_RATIO + 0.05
