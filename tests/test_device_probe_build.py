"""The device probe (tests/devprobe) must keep compiling for gfx950 where there is no GPU: the tests that run it
(test_device_arithmetic_gpu.py) are skipped there and would otherwise rot unnoticed."""
import ctypes
import shutil

import pytest


def _hipcc():
    from fetal_t2mapping_amd import build as product_build

    try:
        return product_build.hipcc()
    except RuntimeError:
        return None


@pytest.mark.skipif(_hipcc() is None and shutil.which("hipcc") is None, reason="hipcc not installed")
def test_device_probe_cross_compiles_for_gfx950(tmp_path):
    from devprobe import probe
    from fetal_t2mapping_amd import build as product_build

    cmd = probe.command()
    assert "--offload-arch=gfx950" in cmd
    # the flags of the product build that decide what the arithmetic compiles to
    for flag in ("-O3", "-std=c++17", "-ffp-contract=off", "-fno-gpu-rdc", "-shared", "-fPIC"):
        assert flag in cmd, flag
    assert cmd[0] == product_build.hipcc()
    so = probe.build(force=True, out=str(tmp_path / "libt2fit_devprobe.so"))
    lib = ctypes.CDLL(so)
    for name in ("devprobe_unary", "devprobe_binary", "devprobe_sqrt_near", "devprobe_i0e4", "devprobe_unary_f32",
                 "devprobe_eval", "devprobe_config_default", "devprobe_device_count"):
        assert hasattr(lib, name), name
