"""The Python seam as a whole: ``t2map`` is a facade over one binding module per stage (``_gpu_fit``, ``_gpu_roi``,
``_gpu_boot``, ``_gpu_tv``, ``_gpu_resample``, ``_gpu_morph``) and one marshalling module (``_gpu``).  Host tests: the
public surface, the symbol groups, the marshalling on CPU tensors and arrays, the map-field table.  GPU tests: the
``out=`` check of ``fill_holes``, the stack-shape check of ``fit_voxels_trace``, the label chunks of ``roi_erode`` and
the two entries of ``fit_volume``."""
import ctypes as C

import numpy as np
import pytest

# the public callables and classes of t2map at the commit before the split: a dropped re-export fails the test
PUBLIC = ["BootMaps", "BootStats", "RoiStats", "T2Maps", "binary_close", "binary_dilate", "binary_erode", "binary_open",
          "binary_threshold", "bootstrap_volume", "build_mask", "compute_residuals", "denoise_tv", "dense_labels",
          "estimate_background_sigma", "fill_holes", "fit_table", "fit_volume", "fit_voxel", "fit_voxels", "fit_voxels_trace",
          "label_stats", "make_config", "mask_from_labels", "phantom_labels", "phantom_mask", "reconstruct_stacks", "relabel",
          "resample_volume", "roi_erode", "roi_frame", "roi_stats", "roi_table", "seed_labels", "set_fit_params",
          "stack_mask_flatten", "synth_replica", "synthseg_to_feta", "tv_params", "union_mask_dev"]


def test_public_surface_of_the_facade():
    import fetal_t2mapping_amd as pkg
    from fetal_t2mapping_amd import t2map

    for name in pkg.__all__:
        assert getattr(pkg, name) is not None
        if name != "philox4x32_10":  # the one name of the package that t2map never had
            assert getattr(t2map, name) is getattr(pkg, name), name
    own = ("fetal_t2mapping_amd.t2map", "fetal_t2mapping_amd._gpu")  # defined by the facade or a module behind it
    public = sorted(n for n, v in vars(t2map).items()
                    if not n.startswith("_") and callable(v) and getattr(v, "__module__", "").startswith(own))
    assert public == sorted(PUBLIC)
    assert t2map.ROI_MAX_LABELS == 256 and t2map.RECON_FORMS == ("chain", "fused")


def test_additive_symbols_are_the_four_named_groups():
    from fetal_t2mapping_amd import _abi

    assert _abi.ADDITIVE == _abi.BOOT_SYMBOLS + _abi.TV_SYMBOLS + _abi.RECON_SYMBOLS + _abi.MORPH_SYMBOLS
    assert len(set(_abi.ADDITIVE)) == len(_abi.ADDITIVE) == 15
    declared = {name for name, _, _ in _abi.SYMBOLS}
    assert set(_abi.ADDITIVE) <= declared
    for group, word in ((_abi.BOOT_SYMBOLS, "boot"), (_abi.TV_SYMBOLS, "_tv_")):
        assert all(word in name for name in group)


def test_marshalling_on_cpu_tensors_and_arrays():
    import torch

    from fetal_t2mapping_amd import _gpu

    assert _gpu.is_tensor(torch.zeros(2)) and _gpu.is_tensor(torch.nn.Parameter(torch.zeros(2)))
    for a in (np.zeros(2), [1, 2], 3.0, None, "torch"):
        assert not _gpu.is_tensor(a)
    # integer labels: float and bool are refused, int64 ids above 2^31 survive, narrow dtypes become int32
    for bad in (np.zeros((2, 2, 2), np.float32), np.zeros(3, bool), torch.zeros(3), torch.zeros(3, dtype=torch.bool)):
        with pytest.raises(ValueError, match="integer dtype"):
            _gpu.int_labels(bad)
    big = np.array([[0, 2**31 + 5, -7, 2**40]], np.int64)
    for src in (big, torch.from_numpy(big)):
        t = _gpu.int_labels(src, torch.device("cpu"))
        assert t.dtype == torch.int64 and t.shape == (1, 4) and t.tolist() == big.tolist()
    assert _gpu.int_labels(np.array([3, 2**32 - 1], np.uint32)).tolist() == [3, 2**32 - 1]
    for dt in (np.int8, np.uint8, np.int16, np.uint16, np.int32):
        assert _gpu.int_labels(np.array([1, 2], dt)).dtype == torch.int32
    # flat / mask / volume on the host device
    cpu = torch.device("cpu")
    f = _gpu.flat(np.arange(6, dtype=np.float64).reshape(2, 3), cpu, 6)
    assert f.dtype == torch.float32 and f.shape == (6,) and f.is_contiguous()
    assert _gpu.flat(torch.arange(6).reshape(2, 3).t(), cpu).tolist() == [0.0, 3.0, 1.0, 4.0, 2.0, 5.0]
    assert _gpu.flat([1.9, -1.9], cpu, dtype="int32").tolist() == [1, -1]
    with pytest.raises(ValueError, match="k has 6 elements, the volume has 5"):
        _gpu.flat(np.zeros(6), cpu, 5, "k")
    assert _gpu.mask_u8(None, cpu, 3).tolist() == [1, 1, 1]
    assert _gpu.mask_u8(np.array([[0.0, 0.5], [-2.0, 0.0]]), cpu, 4).tolist() == [0, 1, 1, 0]
    assert _gpu.mask_u8(torch.tensor([0, 7, 255], dtype=torch.uint8), cpu, 3).tolist() == [0, 1, 1]
    with pytest.raises(ValueError, match="mask shape"):
        _gpu.mask_u8(np.ones(4), cpu, 3)
    v = _gpu.volume(np.full((1, 2, 2), 3.5), torch.uint8, cpu, "mask")
    assert v.dtype == torch.uint8 and v.tolist() == [[[1, 1], [1, 1]]]
    with pytest.raises(ValueError, match="mask must be 3-D"):
        _gpu.volume(np.zeros((2, 2)), torch.uint8, cpu, "mask")


def test_check_out_refuses_what_the_library_would_overrun():
    import torch

    from fetal_t2mapping_amd import _gpu

    cpu = torch.device("cpu")
    _gpu.check_out(torch.zeros((3, 5, 7), dtype=torch.uint8), torch.uint8, (3, 5, 7), cpu)
    _gpu.check_out(torch.zeros((3, 35), dtype=torch.int32), "int32", 105, cpu)
    _gpu.check_out(np.zeros((3, 5, 7), np.float32), "float32", 105, None)
    _gpu.check_out(np.zeros((3, 5, 7), np.uint8), torch.uint8, (3, 5, 7), None)
    frozen = np.zeros((3, 5, 7), np.float32)
    frozen.setflags(write=False)
    bad = [(torch.zeros((3, 5, 7)), torch.uint8, (3, 5, 7), cpu),                             # dtype
           (torch.zeros((3, 5, 6), dtype=torch.uint8), torch.uint8, (3, 5, 7), cpu),          # shape
           (torch.zeros((5, 21), dtype=torch.uint8), torch.uint8, (3, 5, 7), cpu),            # same count, other shape
           (torch.zeros((3, 5, 7), dtype=torch.uint8), torch.uint8, 104, cpu),                # count
           (torch.zeros((3, 5, 14), dtype=torch.uint8)[:, :, ::2], torch.uint8, (3, 5, 7), cpu),  # not contiguous
           (torch.zeros((3, 5, 7), dtype=torch.uint8), torch.uint8, (3, 5, 7), torch.device("meta")),  # other device
           (np.zeros((3, 5, 7), np.uint8), torch.uint8, (3, 5, 7), cpu),                      # an array where a tensor goes
           (torch.zeros((3, 5, 7)), "float32", 105, None),                                    # a tensor at the host entry
           (np.zeros((3, 5, 7), np.float64), "float32", 105, None),                           # dtype
           (np.zeros(106, np.float32), "float32", 105, None),                                 # count
           (np.zeros((105, 2), np.float32)[:, 0], "float32", 105, None),                      # not contiguous
           (frozen, "float32", 105, None),                                                    # read-only
           (None, "float32", 105, None)]
    for out, dtype, size, dev in bad:
        with pytest.raises(ValueError, match="out.t2 must be a"):
            _gpu.check_out(out, dtype, size, dev, "out.t2")


def test_map_field_table_mirrors_the_abi_struct():
    from fetal_t2mapping_amd import _abi
    from fetal_t2mapping_amd._gpu_fit import MAP_FIELDS

    assert [name for name, _, _ in MAP_FIELDS] == [name for name, _ in _abi.T2FitMaps._fields_]
    assert all(ctype is C.c_void_p for _, ctype in _abi.T2FitMaps._fields_)
    assert {name: dtype for name, dtype, _ in MAP_FIELDS} == {
        "t2": "float32", "k": "float32", "sigma": "float32", "res": "float32", "r2": "float32", "fun": "float32",
        "nit": "int32", "status": "uint8", "t2_se": "float32"}
    assert [name for name, _, required in MAP_FIELDS if required] == ["t2", "k", "sigma", "res"]


# ---------------------------------------------------------------------------------------------------------------------
# on the device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def t2():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the gpu-marked tests need an MI355X")
    import fetal_t2mapping_amd as t2

    return t2


@pytest.mark.gpu
def test_fill_holes_refuses_a_bad_out_before_it_writes(t2):
    """fill_holes(out=...) hands out.data_ptr() to the library, which writes one byte per voxel of the mask: a tensor of
    another dtype, shape or layout is refused as the other morphology calls refuse it, and nothing has been touched."""
    import torch

    rng = np.random.default_rng(11)
    a = rng.random((3, 5, 7)) < 0.5
    a[1, 1:4, 1:6] = True
    a[1, 2, 2:5] = False  # a hole that only the per-plane fill closes
    mask = torch.from_numpy(a.astype(np.uint8)).cuda()
    before = mask.clone()
    dev = mask.device
    for bad in (torch.zeros((3, 5, 7), dtype=torch.float32, device=dev), torch.zeros((3, 5, 6), dtype=torch.uint8, device=dev),
                torch.zeros((3, 5, 14), dtype=torch.uint8, device=dev)[:, :, ::2]):
        with pytest.raises(ValueError, match="out must be a contiguous uint8 tensor") as fill:
            t2.fill_holes(mask, slice_axis=0, out=bad)
        with pytest.raises(ValueError) as morph:
            t2.binary_dilate(mask, np.ones((1, 3, 3), bool), out=bad)
        assert str(fill.value) == str(morph.value)
        assert torch.equal(mask, before)
    for axis in (None, 0):
        want = t2.fill_holes(mask, slice_axis=axis)
        assert torch.equal(mask, before)
        buf = torch.full((3, 5, 7), 9, dtype=torch.uint8, device=dev)
        got = t2.fill_holes(mask, slice_axis=axis, out=buf)
        assert got is buf and torch.equal(got, want)
        inplace = mask.clone()
        assert t2.fill_holes(inplace, slice_axis=axis, out=inplace) is inplace and torch.equal(inplace, want)
    assert int(t2.fill_holes(mask, slice_axis=0).sum()) > int(before.sum())


@pytest.mark.gpu
def test_fit_voxels_trace_checks_the_stack_shape_as_fit_voxels_does(t2):
    """A (10, 5) stack for a six-echo config: the library would read six floats per row."""
    from fetal_t2mapping_amd import synth

    te = synth.te_vector(6)
    table = t2.fit_table("gaussian", True)
    stack = np.full((10, 5), 500.0, np.float32)
    for call in (t2.fit_voxels, t2.fit_voxels_trace):
        with pytest.raises(ValueError, match=r"reshaped_t2w must be \(N, nTE\)"):
            call(np.arange(10), "gaussian", table, te, stack, True, False)
        with pytest.raises(ValueError, match=r"reshaped_t2w must be \(N, nTE\)"):
            call(np.arange(10), "gaussian", table, te, stack.reshape(-1), True, False)
    good = np.full((10, 6), 500.0, np.float32) * np.exp(-te / 150.0).astype(np.float32)
    assert len(t2.fit_voxels_trace(np.arange(10), "gaussian", table, te, good, True, False)) == 6


@pytest.mark.gpu
def test_roi_erode_above_256_labels_equals_its_two_halves(t2):
    """300 labels on (6, 40, 40) run through the library in two groups (1..256, 257..300).  The regions are 3 x 3 x 3
    blocks -- the smallest of which the 3-D cross (connectivity 1, one iteration) leaves a voxel, the centre; a block
    only two voxels thick along an axis is eroded away and the comparison would hold on empty volumes."""
    import torch

    lab = np.zeros((6, 40, 40), np.int32)
    slots = [(z, y, x) for z in range(0, 6, 3) for y in range(0, 39, 3) for x in range(0, 39, 3)]
    assert len(slots) >= 300
    for i, (z, y, x) in enumerate(slots[:300]):
        lab[z:z + 3, y:y + 3, x:x + 3] = i + 1
    lab_d = torch.from_numpy(lab).cuda()
    zero = torch.zeros_like(lab_d)
    whole = t2.roi_erode(lab_d, connectivity=1, iterations=1)
    first = t2.roi_erode(torch.where(lab_d <= 256, lab_d, zero), labels=range(1, 257), connectivity=1, iterations=1)
    second = t2.roi_erode(torch.where(lab_d > 256, lab_d - 256, zero), labels=range(1, 45), connectivity=1, iterations=1)
    assert whole.dtype == torch.int32 and whole.shape == lab_d.shape
    assert torch.equal(torch.where(whole <= 256, whole, zero), first)
    assert torch.equal(torch.where(whole > 256, whole - 256, zero), second)
    assert torch.equal(whole, first + torch.where(second > 0, second + 256, zero))
    # every label keeps exactly the centre of its block
    want = np.zeros_like(lab)
    for i, (z, y, x) in enumerate(slots[:300]):
        want[z + 1, y + 1, x + 1] = i + 1
    assert np.array_equal(whole.cpu().numpy(), want)
    assert torch.equal(t2.roi_erode(lab, labels=range(1, 301), connectivity=1, iterations=1), whole)


@pytest.mark.gpu
def test_fit_volume_numpy_and_torch_entries_fill_the_same_maps(t2):
    """One table drives allocation, the out= check and the pointer fill of both entries: the nine maps of an
    (8, 2, 3, 5) stack are the same bytes from the host entry, from the device entry, and from a second call of either
    that writes into the first call's maps."""
    import torch

    from fetal_t2mapping_amd import synth
    from fetal_t2mapping_amd._gpu_fit import MAP_FIELDS

    echoes, _, te = synth.brain_volume((2, 3, 5), 8, seed=3)
    assert echoes.shape == (8, 2, 3, 5)
    mask = np.ones((2, 3, 5), np.uint8)
    mask[0, 0, 0] = 0
    table = t2.fit_table("gaussian_rician", True)
    host = t2.fit_volume(echoes, mask, te, "gaussian_rician", table, extras=True)
    e_d, m_d = torch.from_numpy(echoes).cuda(), torch.from_numpy(mask).cuda()
    dev = t2.fit_volume(e_d, m_d, te, "gaussian_rician", table, extras=True)
    kept = {}
    for name, dtype, _ in MAP_FIELDS:
        h, d = getattr(host, name), getattr(dev, name)
        assert isinstance(h, np.ndarray) and h.dtype == np.dtype(dtype) and h.shape == (2, 3, 5), name
        assert torch.is_tensor(d) and d.is_cuda and d.dtype == getattr(torch, dtype) and d.shape == (2, 3, 5), name
        assert h.tobytes() == d.cpu().numpy().tobytes(), name
        kept[name] = h.copy()
        h.fill(77)
        d.fill_(77)
    assert host.status.dtype == np.uint8 and np.count_nonzero(kept["status"]) == 29 and kept["t2"][0, 0, 0] == 0
    assert t2.fit_volume(echoes, mask, te, "gaussian_rician", table, extras=True, out=host) is host
    assert t2.fit_volume(e_d, m_d, te, "gaussian_rician", table, extras=True, out=dev) is dev
    for name in kept:
        assert getattr(host, name).tobytes() == kept[name].tobytes(), name
        assert getattr(dev, name).cpu().numpy().tobytes() == kept[name].tobytes(), name
