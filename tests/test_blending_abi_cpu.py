"""The blending entry points exist and refuse a null context before they touch a device."""
import ctypes as C

from jxl_rs_amd import lib


def test_blend_entry_points_reject_null_without_a_device():
    L = lib.load()
    d = lib.blend_desc(0, 0, 16, 16, (lib.BLEND_REPLACE, 0, 0, 0))
    assert L.jxlh_frame_blend(None, C.byref(d), None) == lib.ERR_INVALID_ARGUMENT
    assert L.jxlh_frame_blend(None, None, None) == lib.ERR_INVALID_ARGUMENT
    planes = (C.c_void_p * 3)()
    assert L.jxlh_stage_blend(None, C.byref(d), planes, 3, 16, 16, 16, planes, 16) == lib.ERR_INVALID_ARGUMENT
    assert L.jxlh_stage_blend(None, None, None, 3, 16, 16, 16, None, 16) == lib.ERR_INVALID_ARGUMENT


def test_python_structs_have_the_header_layout():
    # jxlh_blending_info: 4 x u32; jxlh_blend_desc: 2 x i32, 2 x u32, info, u32, 8 x info, 8 x u32
    assert C.sizeof(lib.BlendingInfo) == 16
    assert C.sizeof(lib.BlendDesc) == 16 + 16 + 4 + 8 * 16 + 8 * 4
    assert lib.BlendDesc.ec.offset == 36 and lib.BlendDesc.ec_flags.offset == 36 + 128
    assert (lib.BLEND_REPLACE, lib.BLEND_ADD, lib.BLEND_BLEND, lib.BLEND_ALPHA_WEIGHTED_ADD, lib.BLEND_MUL) == (0, 1, 2, 3, 4)
