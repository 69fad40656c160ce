"""Modular frames (JXLH_FRAME_MODULAR) without a GPU: the header declares and the cross-compiled library exports
jxlh_frame_set_modular_channels, lib.py binds it, frame_begin and the setter validate before touching the device, and
the builder mirror lowers a Modular frame's full stage list (tests/cpp/modular_frame_lowering.cc)."""
import ctypes as C
import os
import re
import subprocess

from test_cpp_host import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_setter():
    from jxl_rs_amd import lib
    src = open(os.path.join(ROOT, "include", "jxl_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"jxlh_status\s+jxlh_frame_set_modular_channels\s*\(", code)
    assert re.search(r"JXLH_FRAME_MODULAR\s*=\s*1u\s*<<\s*4", code) and re.search(r"#define\s+JXLH_MODULAR_XYB\s+\(1u\s*<<\s*16\)", code)
    assert re.search(r"#define\s+JXLH_ABI_VERSION\s+6\b", code), "additions only: the ABI version stays"
    L = lib.load()
    assert hasattr(L, "jxlh_frame_set_modular_channels")
    assert "jxlh_frame_set_modular_channels" in lib.ABI_SYMBOLS
    assert lib.FRAME_MODULAR == 1 << 4 and lib.MODULAR_XYB == 1 << 16
    assert [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
            C.c_uint32] == list(L.jxlh_frame_set_modular_channels.argtypes)
    assert callable(lib.Context.modular_frame_begin) and callable(lib.Context.set_modular_channels)
    from jxl_rs_amd.modular import ModularChain
    assert callable(ModularChain.feed_frame)


def test_begin_and_setter_validate_before_touching_the_device():
    """what the calls reject without a context is the call itself (tests/test_abi_symbols.py does the same for VarDCT
    frames); the rules that need a context are in tests/test_gpu_modular_frame.py::test_state_and_argument_rules"""
    from jxl_rs_amd import lib
    L = lib.load()
    p = lib.FrameParams()
    L.jxlh_default_frame_params(C.byref(p), 70, 37)
    p.flags |= lib.FRAME_MODULAR
    assert p.epf_sigma_for_modular == 1.0
    assert L.jxlh_frame_begin(None, C.byref(p)) == lib.ERR_INVALID_ARGUMENT
    a = (C.c_int32 * 16)()
    assert L.jxlh_frame_set_modular_channels(None, 0, 0, 4, 4, a, a, a, 4, 8) == lib.ERR_INVALID_ARGUMENT
    assert L.jxlh_frame_run(None, 0, 1) == lib.ERR_INVALID_ARGUMENT


def test_lower_modular_frame(tmp_path):
    exe = _build(tmp_path, "modular_frame_lowering")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "modular frame lowering: ok" in r.stdout, (r.stdout + r.stderr)[-2000:]
