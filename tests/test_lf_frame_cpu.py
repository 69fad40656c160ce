"""The LF-frame entry points (LF slots, jxlh_frame_set_lf_from_slot, jxlh_lf_preview) exist, are bound with the
header's prototypes, and refuse what they can refuse before they touch a device."""
import ctypes as C
import os
import re

import numpy as np

from jxl_rs_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["jxlh_ctx_set_lf_frame", "jxlh_frame_save_lf", "jxlh_ctx_clear_lf_frame", "jxlh_frame_set_lf_from_slot",
         "jxlh_lf_preview", "jxlh_lf_preview_async"]


def header():
    src = open(os.path.join(ROOT, "include", "jxl_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_symbols_are_exported_and_bound():
    L = lib.load()
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in lib.ABI_SYMBOLS, n
        assert getattr(L, n).argtypes is not None, n
    for m in ("set_lf_frame", "save_lf", "clear_lf_frame", "set_lf_from_slot", "lf_preview"):
        assert callable(getattr(lib.Context, m)), m


def c_to_ctypes(param):
    """the ctypes type lib.py should bind a C parameter declaration with; a pointer to a struct of the header is bound
    as lib.StructPtr(that struct) and stands here as ("struct*", that struct)"""
    p = param.strip()
    if "*" in p:
        if re.match(r"const jxlh_output_desc\s*\*", p):
            return "struct*", lib.OutputDesc
        if re.match(r"const jxlh_save_desc\s*\*", p):
            return "struct*", lib.SaveDesc.__base__  # lib.SaveDesc adds two properties to the header's struct
        return C.c_void_p
    ty = p.rsplit(None, 1)[0]
    return {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "size_t": C.c_size_t}[ty]


def test_python_prototypes_agree_with_the_header():
    L = lib.load()
    src = header()
    for n in NAMES:
        m = re.search(r"jxlh_status\s+" + n + r"\s*\(([^)]*)\)", src)
        assert m, n
        want = [c_to_ctypes(p) for p in m.group(1).split(",")]
        got = [("struct*", t.struct) if isinstance(t, lib.StructPtr) else t for t in getattr(L, n).argtypes]
        assert got == want, n
    assert re.search(r"#define\s+JXLH_NUM_LF_FRAMES\s+4\b", src) and lib.NUM_LF_FRAMES == 4
    # additions only: the ABI version and the parameter struct are what they were
    assert re.search(r"#define\s+JXLH_ABI_VERSION\s+6\b", src) and L.jxlh_abi_version() == 6
    assert C.sizeof(lib.SaveDesc) == 16 * 4 + 8 * 20  # 16 words, then spot[8] of 5 words each


def test_entry_points_refuse_a_null_context_without_a_device():
    L = lib.load()
    INV = lib.ERR_INVALID_ARGUMENT
    planes = [np.zeros((2, 2), np.float32) for _ in range(3)]
    p = [a.ctypes.data for a in planes]
    assert L.jxlh_ctx_set_lf_frame(None, 0, 2, 2, p[0], p[1], p[2], 2) == INV
    assert L.jxlh_ctx_set_lf_frame(None, 4, 2, 2, p[0], p[1], p[2], 2) == INV
    assert L.jxlh_ctx_set_lf_frame(None, 0, 0, 0, None, None, None, 0) == INV
    assert L.jxlh_frame_save_lf(None, 0) == INV
    assert L.jxlh_ctx_clear_lf_frame(None, 0) == INV
    assert L.jxlh_frame_set_lf_from_slot(None, 0) == INV
    colour = lib.Context.output_desc(lib.COLOR_XYB, "srgb", np.zeros(16, np.float32))
    d = lib.save_desc([0, 1, 2], lib.SAVE_U8)
    out = np.full(16 * 16 * 3, 0xA5, np.uint8)
    for fn in (L.jxlh_lf_preview, L.jxlh_lf_preview_async):
        assert fn(None, 0, 16, 16, 0, 0, 2, 2, C.byref(colour), C.byref(d), out.ctypes.data, 48) == INV
        assert fn(None, 0, 16, 16, 0, 0, 2, 2, None, None, None, 0) == INV
    assert np.all(out == 0xA5)
