"""Builder and loader for the device probe (test infrastructure, see devprobe.hip): the device-only side of the lane
headers, one small kernel per sequence, behind host-pointer launchers.  Mirrors tests/hostsim/sim.py."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from fetal_t2mapping_amd import _abi
from fetal_t2mapping_amd import build as product_build

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libt2fit_devprobe.so")
SRC = os.path.join(HERE, "devprobe.hip")
REPO = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(REPO, "fetal_t2mapping_amd", "csrc")

# the operation numbers of devprobe.hip
UNARY = {"exp_core": 0, "exp_lib": 1, "sqrt_core": 2, "sqrt_lib": 3, "fast_rcp": 4, "fast_rsqrt": 5, "log_lean": 6,
         "i0e": 7, "sqrt_core_h": 8}
BINARY = {"fdiv": 0, "div_by_rcp": 1, "div_ieee": 2}
UNARY_F32 = {"exp": 0, "log": 1, "rsqrt": 2, "rcp": 3}


def command(out: str = SO):
    """The flags of fetal_t2mapping_amd/build.py (same compiler lookup): what the kernels are compiled with."""
    return [product_build.hipcc(), "-O3", "-std=c++17", f"--offload-arch={product_build.ARCH}", "-ffp-contract=off",
            "-fno-gpu-rdc", "-shared", "-fPIC", "-o", out, SRC]


def build(force: bool = False, out: str = SO) -> str:
    deps = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    deps.append(os.path.join(REPO, "include", "t2fit.h"))
    if not force and os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    subprocess.check_call(command(out))
    return out


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        p, i64 = C.c_void_p, C.c_int64
        L.devprobe_unary.argtypes = [C.c_int, p, i64, p, p]
        L.devprobe_binary.argtypes = [C.c_int, p, p, i64, p]
        L.devprobe_sqrt_near.argtypes = [p, p, i64, p, p, p]
        L.devprobe_i0e4.argtypes = [C.c_int, p, i64, C.c_int, p]
        L.devprobe_unary_f32.argtypes = [C.c_int, p, i64, p]
        L.devprobe_eval.argtypes = [C.POINTER(_abi.T2FitConfig), p, p, i64, C.c_int, p]
        L.devprobe_config_default.argtypes = [C.POINTER(_abi.T2FitConfig), C.c_int, C.c_int]
        L.devprobe_dict_scores.argtypes = [p, C.c_size_t, p, C.c_int, i64, p]
        _lib = L
    return _lib


def device_count() -> int:
    return int(lib().devprobe_device_count())


_failed = None  # the first call that returned a HIP error: nothing more is sent to the device after it


def _call(what, fn, *args):
    global _failed
    if _failed is not None:
        raise RuntimeError(f"{what}: not run, an earlier probe call failed ({_failed})")
    rc = fn(*args)
    if rc != 0:
        _failed = f"{what}: HIP error {rc}"
        raise RuntimeError(_failed)


def unary(op: str, x):
    """One of UNARY on a float64 array -> result (same shape); for "sqrt_core_h" -> (root, h)."""
    x = np.ascontiguousarray(x, np.float64)
    y, y2 = np.empty_like(x), np.empty_like(x)
    _call(op, lib().devprobe_unary, UNARY[op], x.ctypes.data, x.size, y.ctypes.data, y2.ctypes.data)
    return (y, y2) if op == "sqrt_core_h" else y


def binary(op: str, a, b):
    """One of BINARY on two float64 arrays of one shape -> the quotient."""
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    assert a.shape == b.shape
    q = np.empty_like(a)
    _call(op, lib().devprobe_binary, BINARY[op], a.ctypes.data, b.ctypes.data, a.size, q.ctypes.data)
    return q


def sqrt_near(x, a):
    """h from t2_sqrt_core_h(x); -> (t2_sqrt_near(a, h), h' = t2_rsqrt_half_near(a, h), t2_sqrt_from_h(a, h'))."""
    x = np.ascontiguousarray(x, np.float64)
    a = np.ascontiguousarray(a, np.float64)
    assert a.shape == x.shape
    near, half, from_h = np.empty_like(x), np.empty_like(x), np.empty_like(x)
    _call("sqrt_near", lib().devprobe_sqrt_near, x.ctypes.data, a.ctypes.data, x.size, near.ctypes.data, half.ctypes.data,
          from_h.ctypes.data)
    return near, half, from_h


def log_i0e4(x, near: bool = False):
    """x: (n, 4) float64; row i is lane i % 64 of wave i // 64 -> t2_log_i0e4 of every row, (n, 4)."""
    x = np.ascontiguousarray(x, np.float64)
    assert x.ndim == 2 and x.shape[1] == 4
    out = np.empty_like(x)
    _call("log_i0e4", lib().devprobe_i0e4, 0, x.ctypes.data, len(x), int(near), out.ctypes.data)
    return out


def i0e4_by_lane(x, near: bool = False):
    """x: (n, 4) float64, every row on one side of 8 -> t2_i0e4_by_lane of every row (values of i0e), (n, 4)."""
    x = np.ascontiguousarray(x, np.float64)
    assert x.ndim == 2 and x.shape[1] == 4
    out = np.empty_like(x)
    _call("i0e4_by_lane", lib().devprobe_i0e4, 1, x.ctypes.data, len(x), int(near), out.ctypes.data)
    return out


def unary_f32(op: str, x):
    """One of UNARY_F32 (the float32 intrinsics of the LM path) on a float32 array."""
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty_like(x)
    _call(op, lib().devprobe_unary_f32, UNARY_F32[op], x.ctypes.data, x.size, y.ctypes.data)
    return y


def eval_points(cfg, rows, xs, nte_special: bool = False):
    """One Lbfgsb::eval per row.  rows: (n, n_te) float32, xs: (n, 3) float64 -> (n, 4): f, g0, g1, g2.  Row i is lane
    i % 64 of wave i // 64.  nte_special: the six-echo specialisation."""
    rows = np.ascontiguousarray(rows, np.float32)
    xs = np.ascontiguousarray(xs, np.float64)
    assert rows.shape == (len(xs), cfg.n_te) and xs.shape[1] == 3
    out = np.empty((len(xs), 4))
    _call("eval", lib().devprobe_eval, C.byref(cfg), rows.ctypes.data, xs.ctypes.data, len(xs), int(nte_special),
          out.ctypes.data)
    return out


def dict_scores(packed, y):
    """The float32 scores of the matrix instruction as the dictionary fit issues it.  packed: the
    bytes of _dict.pack; y: (n_te, n_vox) float32 -> (n_vox, 32 * n_tiles) float32, the padded rows of a ragged last tile
    included (they score 0)."""
    packed = np.ascontiguousarray(packed, np.uint8)
    y = np.ascontiguousarray(y, np.float32)
    assert y.ndim == 2
    n_atoms = int(packed[4:8].view(np.int32)[0])
    out = np.empty((y.shape[1], (n_atoms + 31) // 32 * 32), np.float32)
    _call("dict_scores", lib().devprobe_dict_scores, packed.ctypes.data, packed.size, y.ctypes.data, y.shape[0], y.shape[1],
          out.ctypes.data)
    return out


def config(mode: str, low_field: bool, te, numpy_legacy: bool = False):
    cfg = _abi.T2FitConfig()
    assert lib().devprobe_config_default(C.byref(cfg), _abi.MODELS[mode], int(low_field)) == 0
    te = np.asarray(te, np.float64)
    cfg.n_te = len(te)
    for i, t in enumerate(te):
        cfg.te_ms[i] = t
    cfg.numpy_legacy = int(numpy_legacy)
    return cfg
