"""Marshalling shared by the stage bindings (``_gpu_*.py``): numpy arrays and tensors in, checked device buffers, the
stream and the workspace as the C ABI takes them.  Nothing here knows a stage."""
import ctypes as C

import numpy as np

from ._lib import require_gpu


def is_tensor(a) -> bool:
    import torch

    return torch.is_tensor(a)


def pick_device(arrays, device):
    """The first CUDA tensor's device, else ``cuda:device``."""
    import torch

    for a in arrays:
        if a is not None and is_tensor(a) and a.is_cuda:
            return a.device
    return torch.device("cuda", device)


def flat(a, dev, n=None, what="array", dtype="float32"):
    """numpy array (converted on the host) or tensor -> contiguous flat tensor of `dtype` on `dev`, of `n` elements
    when `n` is given."""
    import torch

    t = a if is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype))
    t = t.to(dev, getattr(torch, dtype)).contiguous().reshape(-1)
    if n is not None and t.numel() != n:
        raise ValueError(f"{what} has {t.numel()} elements, the volume has {n}")
    return t


def int_labels(a, dev=None):
    """An integer label volume (numpy array of any integer dtype, or a tensor) as a torch tensor, shape kept: int32, or
    int64 where the ids may not fit (the caller reduces those).  Moved to `dev` when one is given."""
    import torch

    if is_tensor(a):
        if a.dtype.is_floating_point or a.dtype == torch.bool:
            raise ValueError("label volumes must have an integer dtype")
    else:
        a = np.asarray(a)
        if a.dtype.kind not in "iu":
            raise ValueError("label volumes must have an integer dtype")
        a = torch.from_numpy(np.ascontiguousarray(a).astype(np.int64 if a.dtype.itemsize > 4 or a.dtype == np.uint32 else np.int32))
    return a if dev is None else a.to(dev)


def mask_u8(mask, dev, n):
    """0 / not 0 -> contiguous flat uint8 0 / 1 on `dev`; None is all ones."""
    import torch

    if mask is None:
        return torch.ones(n, dtype=torch.uint8, device=dev)
    m = mask if is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0).view(np.uint8))
    m = (m != 0).to(dev, torch.uint8).contiguous().reshape(-1)
    if m.numel() != n:
        raise ValueError("mask shape does not match the volume")
    return m


def volume(a, dtype, dev, what="volume"):
    """A 3-D numpy array or tensor -> contiguous tensor of `dtype` on `dev` (a mask: 0 / not 0 -> uint8 0 / 1)."""
    import torch

    t = a if is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dim() != 3:
        raise ValueError(f"{what} must be 3-D (z, y, x), got shape {tuple(t.shape)}")
    if dtype == torch.uint8 and t.dtype != torch.uint8:
        t = t != 0
    return t.to(dev, dtype).contiguous()


def check_out(out, dtype, shape_or_numel, dev, what="out"):
    """Refuse an ``out=`` buffer before the library writes raw bytes of `dtype` (a torch dtype or its name) through its
    pointer: a contiguous tensor on `dev`, or with ``dev=None`` (the host entry) a writable C-contiguous numpy array; of
    exactly the shape given, or of the element count when that is an int."""
    import torch

    name = str(dtype).split(".")[-1]
    if dev is None:
        kind = f"writable C-contiguous {name} numpy array"
        ok = isinstance(out, np.ndarray) and out.dtype == np.dtype(name) and out.flags.c_contiguous and out.flags.writeable
    else:
        kind = f"contiguous {name} tensor on {dev}"
        ok = torch.is_tensor(out) and out.dtype == getattr(torch, name) and out.device == dev and out.is_contiguous()
    if isinstance(shape_or_numel, (int, np.integer)):
        size = f"with {shape_or_numel} elements"
        ok = ok and int(np.prod(out.shape)) == shape_or_numel
    else:
        size = f"of shape {tuple(shape_or_numel)}"
        ok = ok and tuple(out.shape) == tuple(shape_or_numel)
    if not ok:
        raise ValueError(f"{what} must be a {kind} {size}")


def current_stream():
    """The current device's current torch stream, as the C ABI takes one."""
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def workspace(nbytes, dev):
    """A device workspace of nbytes for the library: the tensor that owns it and the pointer, 256-byte aligned.  Hand
    the tensor to :func:`release` after the launch."""
    import torch

    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    return ws, (ws.data_ptr() + 255) // 256 * 256


def release(*tensors):
    """After a launch on the current stream that reads or writes these temporaries.  They are dropped when the caller
    returns, while the launch may still be queued: recording the stream keeps the caching allocator from handing their
    memory to work on another stream before that launch has run."""
    import torch

    for t in tensors:
        if t is not None:
            t.record_stream(torch.cuda.current_stream())


def require(*symbols):
    """The library, with these entry points (additive symbols of ABI 5: looked up, not assumed)."""
    lib = require_gpu()
    missing = [name for name in symbols if not hasattr(lib, name)]
    if missing:
        raise RuntimeError(f"this build of libt2fit_hip.so lacks {', '.join(missing)}: rebuild it "
                           "(python -m fetal_t2mapping_amd.build)")
    return lib
