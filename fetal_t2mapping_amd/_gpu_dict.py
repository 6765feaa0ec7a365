"""Dictionary-matching fit on the GPU (``t2map.dictionary``): any signal model as a table of decay curves, matched on the
matrix cores and re-scored in float64; :mod:`fetal_t2mapping_amd._dict` states the result in numpy and holds the builders
both paths share."""
import ctypes as C

import numpy as np

from . import _abi
from ._dict import Dictionary, biexp, check_atoms, log_grid, lookup, monoexp  # noqa: F401  (the namespace's builders)
from ._gpu import current_stream, flat, is_tensor, mask_u8, pick_device, release, require
from ._gpu_fit import T2Maps
from ._lib import check, load


def pack(atoms):
    """The packed dictionary (``uint8`` numpy array) as ``t2fit_dict_pack_host`` writes it; no device.  ``atoms``: a
    :class:`Dictionary` or float32 ``(A, nTE)``.  The library refuses what :func:`_dict.check_atoms` refuses."""
    a = np.ascontiguousarray(atoms.atoms if isinstance(atoms, Dictionary) else atoms, dtype=np.float32)
    if a.ndim != 2:
        raise ValueError(f"a dictionary is (A, nTE), got shape {a.shape}")
    lib = load()
    need = C.c_size_t(0)
    check(lib.t2fit_dict_pack_bytes(a.shape[0], a.shape[1], C.byref(need)))
    out = np.zeros(need.value, np.uint8)
    check(lib.t2fit_dict_pack_host(a.shape[0], a.shape[1], a.ctypes.data, out.ctypes.data, out.nbytes))
    return out


def _packed_on(dictionary, dev):
    """The packed block on `dev`; a :class:`Dictionary` keeps it for the next call."""
    import torch

    cache = getattr(dictionary, "_packed_dev", None) if isinstance(dictionary, Dictionary) else None
    key = str(dev)
    if cache is not None and key in cache:
        return cache[key]
    t = torch.from_numpy(pack(dictionary)).to(dev)
    if t.data_ptr() % 16:
        raise RuntimeError("the device allocator returned a block that is not aligned to 16 bytes")
    if isinstance(dictionary, Dictionary):
        if cache is None:
            cache = dictionary._packed_dev = {}
        cache[key] = t
    return t


def match(echoes, dictionary, mask=None, device=0):
    """``(index int32, scale float32, rmse float32)`` CUDA tensors of the echoes' spatial shape.  ``echoes``: float32
    ``(nTE, ...)``, numpy array or tensor; ``dictionary``: a :class:`Dictionary` or float32 atoms ``(A, nTE)``; ``mask``: 0 /
    not 0 of the spatial shape, or None.  ``index``: the best atom (the float64 argmax of the normalised inner product, the
    lowest index on a tie), -1 outside the mask and where a sample is not finite; ``scale``: the projection onto the atom as
    given, not below 0; ``rmse``: the root mean square residual of ``scale * atom``.  Bit for bit :func:`_dict.match`."""
    import torch

    lib = require(*_abi.DICT_SYMBOLS)
    n_te = int((dictionary.atoms if isinstance(dictionary, Dictionary) else np.asarray(dictionary)).shape[-1])
    shape = tuple(int(v) for v in echoes.shape)
    if len(shape) < 1 or shape[0] != n_te:
        raise ValueError(f"the echoes are TE-major with {shape[0] if shape else 0} echoes, the dictionary has {n_te}")
    spatial = shape[1:]
    n_vox = int(np.prod(spatial, dtype=np.int64))
    dev = pick_device((echoes, mask), device)
    with torch.cuda.device(dev):
        packed = _packed_on(dictionary, dev)
        y = flat(echoes, dev)
        msk = None if mask is None else mask_u8(mask, dev, n_vox)
        index = torch.empty(n_vox, dtype=torch.int32, device=dev)
        scale = torch.empty(n_vox, dtype=torch.float32, device=dev)
        rmse = torch.empty(n_vox, dtype=torch.float32, device=dev)
        check(lib.t2fit_dict_match_dev(y.data_ptr(), n_te, n_vox, None if msk is None else msk.data_ptr(), packed.data_ptr(),
                                       index.data_ptr(), scale.data_ptr(), rmse.data_ptr(), current_stream()))
        release(y, msk)
    return index.reshape(spatial), scale.reshape(spatial), rmse.reshape(spatial)


def fit_volume_dict(echoes, mask, dictionary, device=0):
    """The dictionary fit as a :class:`T2Maps` plus ``extras``: ``t2`` from the dictionary's ``t2`` column, ``k`` the scale,
    ``sigma`` zero, ``res`` the RMSE of the matched atom, ``status`` converged / masked / non-finite; ``extras`` maps every
    other parameter column's name, and ``'index'``, to its map.  numpy echoes give numpy maps, a tensor gives tensors."""
    import torch

    if not isinstance(dictionary, Dictionary):
        raise ValueError("fit_volume_dict takes a Dictionary (its params name what an atom stands for)")
    if "t2" not in dictionary.names:
        raise ValueError(f"the dictionary has no 't2' column (it has {', '.join(dictionary.names)})")
    index, scale, rmse = match(echoes, dictionary, mask, device)
    dev = index.device
    table = torch.from_numpy(dictionary.params).to(dev)
    hit = index >= 0
    safe = index.clamp(min=0).long()
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    column = {n: torch.where(hit, table[:, c][safe], zero) for c, n in enumerate(dictionary.names)}
    status = torch.full(index.shape, _abi.ST_NONFINITE, dtype=torch.uint8, device=dev)  # in the mask and not matched
    if mask is not None:
        status[mask_u8(mask, dev, index.numel()).reshape(index.shape) == 0] = _abi.ST_MASKED
    status[hit] = _abi.ST_CONVERGED
    host = (lambda t: t) if is_tensor(echoes) else (lambda t: t.cpu().numpy())
    maps = T2Maps(t2=host(column.pop("t2")), k=host(scale), sigma=host(torch.zeros_like(scale)), res=host(rmse), status=host(status))
    extras = {n: host(t) for n, t in column.items()}
    extras["index"] = host(index)
    return maps, extras
