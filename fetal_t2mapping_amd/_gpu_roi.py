"""In-vivo atlas ROI statistics on the GPU: eroded per-label regions and their mean / std / median (the reference's
utils/ada_utils.py:130-216 get_t2_per_roi, :885-968 compute_t2_per_tissue_feta)."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

from ._gpu import current_stream, flat, int_labels, pick_device
from ._lib import check, require_gpu

ROI_MAX_LABELS = 256  # labels per library call (one 8-bit digit of its counting sort); more run in chunks here


@dataclass
class RoiStats:
    """Per-label statistics of one map, numpy arrays of length n_labels: ``mean`` / ``std`` (ddof = 0) / ``median``
    float64 over the non-NaN values (NaN for a label without any; ``median`` is None when it was not asked for),
    ``count`` int64 = voxels of the region (the reference's ``nvoxel``), ``valid`` int64 = those that are not NaN."""
    mean: np.ndarray
    std: np.ndarray
    median: Optional[np.ndarray]
    count: np.ndarray
    valid: np.ndarray


def dense_labels(label, labels):
    """Remap the label ids of interest to the dense range the kernels work on: voxels whose value is ``labels[i]``
    become ``i + 1``, every other voxel 0.  ``label``: integer torch tensor on any device (torch ops only, no copy to
    the host); ``labels``: distinct integer ids, e.g. the ``index`` values of an atlas XML or FreeSurfer ids.
    Returns an int32 tensor on the same device."""
    import torch

    ids = [int(v) for v in labels]
    if not ids:
        raise ValueError("labels is empty")
    if len(set(ids)) != len(ids):
        raise ValueError("labels holds an id twice")
    ids_t = torch.tensor(ids, dtype=torch.int64, device=label.device)
    sorted_ids, order = torch.sort(ids_t)
    lab = label.to(torch.int64)
    pos = torch.searchsorted(sorted_ids, lab.reshape(-1)).clamp_(max=len(ids) - 1).reshape(lab.shape)
    hit = sorted_ids[pos] == lab
    return torch.where(hit, order[pos] + 1, torch.zeros_like(pos)).to(torch.int32)


def _label_range(lab):
    """The default labels of a volume are ``1..lab.max()``: their number (at least one)."""
    return max(int(lab.max().item()) if lab.numel() else 0, 1)


def _label_chunks(lab, n_labels):
    """The labels ``1..n_labels`` of the dense int32 tensor `lab` in groups the library takes: yields ``(lo, k, chunk)``
    where `chunk` holds the labels ``lo + 1..lo + k`` as ``1..k`` and 0 elsewhere -- `lab` itself, without a copy, when
    one group holds them all."""
    import torch

    if n_labels <= ROI_MAX_LABELS:
        yield 0, n_labels, lab
        return
    for lo in range(0, n_labels, ROI_MAX_LABELS):
        k = min(ROI_MAX_LABELS, n_labels - lo)
        yield lo, k, torch.where((lab > lo) & (lab <= lo + k), lab - lo, torch.zeros_like(lab)).contiguous()


def roi_erode(label, tissue=None, tissue_value=None, *, labels=None, connectivity: int = 3, iterations: int = 1,
              device: int = 0):
    """The eroded region of every label at once: for each id ``L`` of ``labels`` the voxels of
    ``binary_erosion((tissue == tissue_value) & (label == L), generate_binary_structure(3, connectivity),
    iterations)`` (utils/ada_utils.py:165-169, :192-196, :925-933), as ONE int32 CUDA tensor shaped like ``label``
    that holds ``i + 1`` on the eroded region of ``labels[i]`` and 0 elsewhere (the masks of one atlas are disjoint).
    ``label`` / ``tissue``: 3-D numpy arrays or tensors of any integer dtype; ``labels`` defaults to
    ``1..label.max()``; ``iterations = 0`` returns the regions as they are."""
    import torch

    lib = require_gpu()
    dev = pick_device((label, tissue), device)
    lab = int_labels(label)
    if lab.dim() != 3:
        raise ValueError("label must be a 3-D volume (z, y, x)")
    lab = lab.to(dev)
    tis = None
    if tissue is not None:
        if tissue_value is None:
            raise ValueError("tissue_value is required with tissue")
        tis = int_labels(tissue)
        if tuple(tis.shape) != tuple(lab.shape):
            raise ValueError("tissue shape does not match the label volume")
        tv = int(tissue_value)
        # the library compares int32 values: a wider tissue volume is reduced to {0, 1} first
        if tis.dtype in (torch.int64,) or not -2**31 <= tv < 2**31:
            tis, tv = (tis.to(dev) == tv).to(torch.int32), 1
        tis = tis.to(dev, torch.int32).contiguous()
    if labels is not None:
        lab, n = dense_labels(lab, labels), len(list(labels))
    else:
        n = _label_range(lab)
        lab = torch.where((lab >= 1) & (lab <= n), lab, torch.zeros_like(lab)).to(torch.int32)
    lab = lab.contiguous()
    nz, ny, nx = (int(v) for v in lab.shape)
    chunked = n > ROI_MAX_LABELS  # more than one group: each result is added to `out`
    with torch.cuda.device(dev):
        st = current_stream()
        out = torch.zeros_like(lab) if chunked else torch.empty_like(lab)
        part = torch.empty_like(lab) if chunked else out
        for lo, k, chunk in _label_chunks(lab, n):
            check(lib.t2fit_roi_erode_dev(chunk.data_ptr(), tis.data_ptr() if tis is not None else None,
                                          tv if tis is not None else 0, nz, ny, nx, k, int(connectivity), int(iterations),
                                          part.data_ptr(), st))
            if chunked:  # the regions are disjoint, the results add up
                out += torch.where(part > 0, part + lo, torch.zeros_like(part))
    return out


def roi_stats(map_, roi, n_labels: int, *, median: bool = True, device: int = 0) -> RoiStats:
    """``np.mean`` / ``np.std`` / ``np.median`` / ``len`` of ``map_[roi == L]`` for L in 1..n_labels on the GPU
    (utils/ada_utils.py:171-189).  ``map_``: float32 numpy array or CUDA tensor; ``roi``: integer array / tensor of the
    same shape, e.g. what :func:`roi_erode` returned.  NaN map values are left out and show as ``valid < count``."""
    import torch

    lib = require_gpu()
    n_labels = int(n_labels)
    if n_labels < 1:
        raise ValueError("n_labels must be at least 1")
    dev = pick_device((map_, roi), device)
    r = int_labels(roi, dev)
    if tuple(np.shape(map_)) != tuple(r.shape):
        raise ValueError("roi shape does not match the map")
    m = flat(map_, dev)
    if r.dtype != torch.int32:
        r = torch.where((r >= 1) & (r <= n_labels), r, torch.zeros_like(r)).to(torch.int32)
    r = r.contiguous().reshape(-1)
    mean = torch.empty(n_labels, dtype=torch.float64, device=dev)
    std = torch.empty(n_labels, dtype=torch.float64, device=dev)
    med = torch.empty(n_labels, dtype=torch.float64, device=dev) if median else None
    cnt = torch.empty(n_labels, dtype=torch.int64, device=dev)
    val = torch.empty(n_labels, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        st = current_stream()
        for lo, k, rc in _label_chunks(r, n_labels):
            check(lib.t2fit_roi_stats_dev(m.data_ptr(), rc.data_ptr(), m.numel(), k, mean[lo:].data_ptr(), std[lo:].data_ptr(),
                                          med[lo:].data_ptr() if median else None, cnt[lo:].data_ptr(), val[lo:].data_ptr(), st))
    return RoiStats(mean.cpu().numpy(), std.cpu().numpy(), med.cpu().numpy() if median else None, cnt.cpu().numpy(),
                    val.cpu().numpy())


def roi_frame(index, names, count, valid, stats: dict):
    """The table :func:`roi_table` returns, from statistics that are already computed: ``stats`` maps a map's name to
    ``(mean, std, median)``.  ``np.mean`` / ``np.std`` / ``np.median`` of a float32 map are float32 numbers, so the
    statistics are rounded to float32 (and stored as float64, as ``phantom_frame`` does): the text pandas writes then
    has the digits numpy returns on the float32 map."""
    import pandas as pd

    index = [int(v) for v in index]
    names = [str(v) for v in (names if names is not None else index)]
    if len(names) != len(index):
        raise ValueError("names and labels differ in length")
    cols = {"roi": names, "index": index, "nvoxel": np.asarray(count, np.int64), "nvalid": np.asarray(valid, np.int64)}
    for m, (mean, std, med) in stats.items():
        for stat, v in (("mean", mean), ("std", std), ("median", med)):
            cols[f"{stat}_{m}"] = np.asarray(v, np.float64).astype(np.float32).astype(np.float64)
    return pd.DataFrame(cols)


def roi_table(maps: dict, label, tissue=None, tissue_value=None, *, labels=None, names=None, connectivity: int = 3,
              iterations: int = 1, device: int = 0):
    """``get_t2_per_roi`` for one atlas (utils/ada_utils.py:130-216) as a ``pandas.DataFrame``: the regions are eroded
    once (:func:`roi_erode`), then every map of ``maps`` (name -> float32 volume) is reduced per region
    (:func:`roi_stats`).  One row per id of ``labels`` (default ``1..label.max()``); columns ``roi`` (``names[i]``, the
    id when there are none), ``index`` (the id), ``nvoxel``, ``nvalid``, then ``mean_<m>``, ``std_<m>``, ``median_<m>``
    per map."""
    if not maps:
        raise ValueError("maps is empty")
    roi = roi_erode(label, tissue, tissue_value, labels=labels, connectivity=connectivity, iterations=iterations, device=device)
    if labels is not None:
        index = [int(v) for v in labels]
    else:
        index = list(range(1, _label_range(int_labels(label)) + 1))
    count = valid = None
    stats = {}
    for name, m in maps.items():
        if tuple(m.shape) != tuple(roi.shape):
            raise ValueError(f"map {name!r} does not have the label volume's shape")
        s = roi_stats(m, roi, len(index), device=device)
        stats[name] = (s.mean, s.std, s.median)
        # nvoxel is the same for every map; nvalid is the first map's (the maps of one fit are NaN in the same voxels)
        count, valid = (s.count, s.valid) if count is None else (count, valid)
    return roi_frame(index, names, count, valid, stats)
