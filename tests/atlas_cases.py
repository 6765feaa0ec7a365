"""Inputs shared by tests/test_atlas_host.py and tests/test_atlas_gpu.py: seeded, built once per process.  The named
cases of the 43 sums come from register_cases; here are the bin volumes laid over them, the cross-contrast recovery pair
and the blob labels of the stage."""
import ctypes as C
import functools
import os

import numpy as np

import register_cases as K
from fetal_t2mapping_amd import _register as G
from fetal_t2mapping_amd import _resample as R

SUMS_CASES = ("prime", "bricks", "empty_bricks", "outside", "nothing", "fixed_1x1x1", "fixed_9x6x65", "fixed_8x4x64", "half_rim",
              "integer", "tail257")
N_BINS = (1, 7, 64)


@functools.lru_cache(maxsize=None)
def bins_of(name, n_bins):
    """The bin volume of a named case's fixed volume (normal, mean 400, deviation 120) over 220 .. 580: the tails beyond
    1.5 deviations clamp into bins 0 and n_bins - 1, which are then the fullest."""
    return G.bin_volume(K.case(name)[0], 220.0, n_bins / 360.0, n_bins)


@functools.lru_cache(maxsize=None)
def layout_case(kind):
    """``(bins, moving, A, fixed mask, moving mask)`` on the "bricks" volumes with 64 bins laid out by position:
    'brick': every brick of 64 x 4 x 8 holds one bin, a different one from brick to brick; 'lanes': every lane of a wave
    holds another bin (bin = x mod 64), so all 64 are present in every wave."""
    fixed, moving, a, fmask, mmask = K.case("bricks")
    iz, iy, ix = np.meshgrid(*(np.arange(n) for n in fixed.shape), indexing="ij")
    if kind == "brick":
        nbz, nby, nbx = G.brick_counts(fixed.shape)
        bins = (((iz // G.BZ) * nby + iy // G.BY) * nbx + ix // G.BX) * 5 % 64
    else:
        bins = ix % 64
    return bins.astype(np.uint8), moving, a, fmask, mmask


@functools.lru_cache(maxsize=None)
def statement(name, n_bins):
    """``(binned, lut, sums_lut)`` of the numpy statement for a named case (or a layout case at 64 bins)."""
    if name in ("brick", "lanes"):
        bins, moving, a, fmask, mmask = layout_case(name)
    else:
        _, moving, a, fmask, mmask = K.case(name)
        bins = bins_of(name, n_bins)
    binned = G.binned_sums(bins, moving, a, n_bins, fmask, mmask)
    lut = G.lut_from_binned(binned)
    return binned, lut, G.registration_sums_lut(bins, lut, moving, a, fmask, mmask)


# ---- the cross-contrast recovery pair --------------------------------------------------------------------------------
STRETCH = np.array([[1.06, 0.03, -0.02], [0.0, 0.95, 0.025], [0.0, 0.0, 1.04]])
RECOVERY_TRUE = K.rigid((4.0, 3.0, -5.0), (2.5, -1.5, 2.0))
RECOVERY_TRUE[:3, :3] = RECOVERY_TRUE[:3, :3] @ STRETCH
START_TRE = 7.34  # mm, of the identity


def remap(f):
    """A T1-like remapping of the phantom's intensities: not monotonic, zero in the background."""
    f = np.asarray(f, np.float64)
    return ((900.0 - 700.0 * np.abs(f / f.max() - 0.45) / 0.55) * (f > 20)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def recovery_pair():
    """``(fixed, moving, geometry, fixed mask, moving mask)``: register_cases.recovery_pair's fixed volume and its
    remapped copy resampled through RECOVERY_TRUE (so that remap(fixed)(x) = moving(T x))."""
    fixed, _, g, _, _ = K.recovery_pair()
    moving = R.resample(remap(fixed), R.index_affine(g, g, np.linalg.inv(RECOVERY_TRUE)), g.shape)
    return fixed, moving, g, G.build_mask(fixed, threshold=20), G.build_mask(moving, threshold=20)


@functools.lru_cache(maxsize=None)
def recovered(metric, dof, bins=32):
    """The statement's registration of the recovery pair, once per process."""
    fixed, moving, g, fmask, mmask = recovery_pair()
    return G.register_affine(fixed, moving, g, g, metric=metric, bins=bins, dof=dof, fixed_mask=fmask, moving_mask=mmask)


def tre(found):
    fixed, _, g, fmask, _ = recovery_pair()
    return G.target_registration_error(found, RECOVERY_TRUE, fmask, g)


@functools.lru_cache(maxsize=None)
def gradient_case():
    """The recovery volumes with a fixed mask that is a box 6 voxels inside and a moving mask of all ones (no voxel
    enters or leaves the counted set under a small change of the transform)."""
    fixed, moving, g, _, _ = recovery_pair()
    box = np.zeros(fixed.shape, np.uint8)
    box[6:-6, 6:-6, 6:-6] = 1
    return fixed, moving, g, box, np.ones(moving.shape, np.uint8)


GRADIENT_P0 = np.array([0.02, -0.01, 0.03, 0.5, -0.3, 0.4, 0.01, -0.02, 0.01, 0.01, 0.0, -0.01])


# ---- the refusals of the raw ABI ---------------------------------------------------------------------------------------
def check_refusals(lib, src, bins, lut, fmask, moving, mmask, binned, sums, ws, ws43, fshape, mshape, a, n_bins, stream):
    """Every refusal include/t2fit.h lists for the four symbols, each T2FIT_E_INVALID with its message and before any
    launch -- so the pointers may be made up (the host test) or real (the device test, which then checks that no
    output byte changed).  ``ws`` / ``ws43``: 256-aligned workspaces of exactly the needed sizes."""
    need, need43, scratch = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    assert lib.t2fit_register_binned_workspace_bytes(*fshape, n_bins, C.byref(need)) == 0
    assert lib.t2fit_register_workspace_bytes(*fshape, C.byref(need43)) == 0
    A = (C.c_double * 12)(*np.asarray(a, np.float64).ravel())
    inf = (C.c_double * 12)(*np.asarray(a, np.float64).ravel())
    inf[5] = np.inf
    n_vox = int(np.prod(fshape))

    def refused(rc, word):
        err = lib.t2fit_last_error().decode()
        assert rc == -1 and word in err, (rc, word, err)

    def bin_dev(src=src, n=n_vox, lo=0.0, scale=1.0, nb=n_bins, out=bins):
        return lib.t2fit_register_bin_dev(src, n, lo, scale, nb, out, stream)

    def binned_dev(bins=bins, fmask=fmask, fs=fshape, moving=moving, mmask=mmask, ms=mshape, A=A, nb=n_bins, binned=binned, lut=lut,
                   ws=ws, nbytes=need.value):
        return lib.t2fit_register_binned_sums_dev(bins, fmask, *fs, moving, mmask, *ms, A, nb, binned, lut, ws, nbytes, stream)

    def lut_dev(bins=bins, lut=lut, nb=n_bins, fmask=fmask, fs=fshape, moving=moving, mmask=mmask, ms=mshape, A=A, sums=sums, ws=ws43,
                nbytes=need43.value):
        return lib.t2fit_register_sums_lut_dev(bins, lut, nb, fmask, *fs, moving, mmask, *ms, A, sums, ws, nbytes, stream)

    for nb in (0, -1, 65):
        refused(bin_dev(nb=nb), "n_bins")
        refused(lib.t2fit_register_binned_workspace_bytes(*fshape, nb, C.byref(scratch)), "n_bins")
        refused(binned_dev(nb=nb), "n_bins")
        refused(lut_dev(nb=nb), "n_bins")
    for kw, word in (({"src": None}, "NULL"), ({"out": None}, "NULL"), ({"n": 0}, "n_vox"), ({"lo": np.nan}, "not finite"),
                     ({"lo": -np.inf}, "not finite"), ({"scale": np.inf}, "not finite"), ({"scale": np.nan}, "not finite"),
                     ({"src": src + 2}, "aligned to 4")):
        refused(bin_dev(**kw), word)
    refused(lib.t2fit_register_binned_workspace_bytes(*fshape, n_bins, None), "NULL")
    refused(lib.t2fit_register_binned_workspace_bytes(fshape[0], 0, fshape[2], n_bins, C.byref(scratch)), ">= 1")
    shared = (({"bins": None}, "NULL"), ({"fmask": None}, "NULL"), ({"moving": None}, "NULL"), ({"mmask": None}, "NULL"),
              ({"A": None}, "NULL"), ({"ws": None}, "NULL"), ({"fs": (fshape[0], 0, fshape[2])}, "fixed sizes"),
              ({"ms": (mshape[0], mshape[1], -1)}, "moving sizes"), ({"A": inf}, "non-finite"), ({"moving": moving + 2}, "aligned to 4"))
    for kw, word in shared + (({"binned": None}, "NULL"), ({"binned": binned + 4}, "aligned to 8"), ({"lut": lut + 4}, "aligned to 8"),
                              ({"ws": ws + 128}, "aligned to 256"), ({"nbytes": need.value - 1}, "workspace too small")):
        refused(binned_dev(**kw), word)
    for kw, word in shared + (({"lut": None}, "NULL"), ({"sums": None}, "NULL"), ({"sums": sums + 4}, "aligned to 8"),
                              ({"lut": lut + 4}, "aligned to 8"), ({"ws": ws43 + 128}, "aligned to 256"),
                              ({"nbytes": need43.value - 1}, "workspace too small")):
        refused(lut_dev(**kw), word)


# ---- the stage: a painted atlas ------------------------------------------------------------------------------------------
BLOBS = (((-8.0, -6.0, -5.0), 5.0, 3), ((7.0, 5.0, 1.0), 6.0, 11), ((0.0, -7.0, 8.0), 7.0, 48))  # centre [mm], radius, label


@functools.lru_cache(maxsize=None)
def atlas_case():
    """``(subject, template, geometry, subject mask, {name: labels on the template grid}, truth on the subject grid)``:
    the recovery pair as a T2w subject and a T1 template, two atlases of three balls painted on the template's grid, and
    the same balls carried onto the subject's grid through RECOVERY_TRUE itself."""
    fixed, moving, g, fmask, _ = recovery_pair()
    m, o = R._index_to_point(g)
    iz, iy, ix = np.meshgrid(*(np.arange(n) for n in g.shape), indexing="ij")
    pts = np.stack([ix, iy, iz], -1).astype(np.float64) @ m.T + o
    lab = np.zeros(g.shape, np.int32)
    for centre, radius, value in BLOBS:
        lab[np.sum((pts - np.array(centre)) ** 2, -1) <= radius * radius] = value
    atlases = {"ho": lab, "jhu": np.where(lab == 11, 0, lab * 2).astype(np.int32)}
    a = R.index_affine(g, g, RECOVERY_TRUE)
    truth = {n: R.resample(v, a, g.shape, interp="nearest", default=0) for n, v in atlases.items()}
    return fixed, moving, g, fmask, atlases, truth


@functools.lru_cache(maxsize=None)
def atlas_statement():
    from fetal_t2mapping_amd import _atlas

    subject, template, g, mask, atlases, _ = atlas_case()
    return _atlas.atlas_labels(subject, g, template, g, atlases, mask=mask)


def dice(a, b, value):
    a, b = np.asarray(a) == value, np.asarray(b) == value
    return 2.0 * np.count_nonzero(a & b) / (np.count_nonzero(a) + np.count_nonzero(b))


# ---- recon.py --atlas_labels over fake_sitk ----------------------------------------------------------------------------
def write_atlas_subject(tmp_path):
    """A one-subject tree for recon.py --atlas_labels over fake_sitk (which reads ``path + '.npy'``): two echoes'
    recon_1mm volumes, the first echo's mask, a template and two atlases.  Returns ``(bids, metadata, template path,
    atlas specs)``."""
    import pandas as pd

    from fetal_t2mapping_amd import cli

    subject, template, _, mask, atlases, _ = atlas_case()
    bids = str(tmp_path / "projects") + "/"
    rows = []
    for i, te in enumerate((114, 228)):
        acq = {"prj": "prj-901", "sub": "sub-001", "ses": "ses-01", "run": f"run-{i + 1:02d}", "EchoTime": te / 1000.0,
               "CoilString": "HeadNeck", "ImageOrientationPatientSTR": "ax"}
        rows.append(acq)
        np.save(cli.get_img_path(bids, acq, cli.recon_dirname).replace(" ", "") + ".npy", subject * (1.0 - 0.3 * i))
    np.save(cli.get_img_path(bids, rows[0], cli.mask_dirname).replace(" ", "") + ".npy", mask)
    specs = []
    for name, arr in [("mni152", template)] + sorted(atlases.items()):
        path = str(tmp_path / f"{name}.nii.gz")
        np.save(path + ".npy", arr)
        open(path, "w").close()  # (the flags are checked against the file system)
        specs.append((name, path))
    return bids, pd.DataFrame(rows), specs[0][1], specs[1:]


def check_atlas_files(fake, bids, md, cli):
    """What recon.py --atlas_labels wrote, and that cli.py's label reader finds every atlas under its --roi_stats name."""
    anat = os.path.join(bids, "prj-901", "derivatives", "{0}", "sub-001", "ses-01", "anat", "sub-001_ses-01_te-114_{0}.nii.gz")
    subject, _, _, mask, atlases, _ = atlas_case()
    for d in ("recon_1mm_bet", "recon_1mm_mni152", "recon_1mm_ho", "recon_1mm_jhu"):
        assert anat.format(d) in fake.written, sorted(fake.written)
    bet = fake.written[anat.format("recon_1mm_bet")]
    assert np.array_equal(bet.arr, np.where(mask != 0, subject, 0)) and bet.GetSpacing() == (1.0, 1.0, 1.5)  # the subject's grid
    t = np.loadtxt(anat.format("recon_1mm_mni152").replace(".nii.gz", ".txt"))
    assert t.shape == (4, 4) and np.array_equal(t[3], [0, 0, 0, 1]) and np.all(np.isfinite(t))
    acqs = [acq for _, acq in md.iterrows()]
    for name in ("ho", "jhu"):
        assert cli.parse_roi_spec(name) == (name, None)
        path = anat.format("recon_1mm_" + name)
        np.save(path + ".npy", fake.written[path].arr)
        open(path, "w").close()
        got = cli._read_label_image(fake, bids, acqs, cli.recon_dirname + "_" + name)
        assert got is not None and got.dtype == np.int32 and np.array_equal(got, fake.written[path].arr)
        assert set(np.unique(got)) <= set(np.unique(atlases[name])) and np.count_nonzero(got) > 500
    return t
