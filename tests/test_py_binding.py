"""The Python side of the boundary: jxl_rs_amd/_abi.py is generated from include/jxl_hip.h (and the entry points of
include/jxl_hip_dev.h) by tools/gen_py_binding.py, the way the Rust -sys crate is.  Checked here, without a GPU: the
committed file is what the generator produces now; every struct is laid out as the C compiler lays it out; jxl_rs_amd.lib
still offers every public name, value, layout and signature it offered while the binding was written by hand
(tests/golden/lib_public_abi.json, recorded by tools/record_lib_abi.py on that commit); bind() covers every entry point
and skips what a library lacks."""
import ctypes as C
import json
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_committed_binding_is_current():
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_py_binding.py"), "--check"], check=True)


def test_struct_layouts_match_the_c_compiler(tmp_path):
    import gen_py_binding as g
    from helpers import c_struct_layouts
    from jxl_rs_amd import _abi
    structs = g.parse_header(open(g.HEADER).read())[2]
    assert len(structs) == 20
    got = c_struct_layouts(tmp_path, {n: [f for _, f, _ in fields] for n, fields in structs})
    for n, fields in structs:
        cls = getattr(_abi, g.class_name(n))
        assert issubclass(cls, C.Structure) and [f[0] for f in cls._fields_] == [f for _, f, _ in fields], n
        assert C.sizeof(cls) == got[(n, "size")], n
        for _, f, _ in fields:
            assert (getattr(cls, f).offset, getattr(cls, f).size) == (got[(n, f)], got[(n, f + ".size")]), (n, f)


# the one field whose hand-written type was not the header's: jxlh_output_desc.xyb is a jxlh_xyb_params (16 floats)
RETYPED = {("OutputDesc", "xyb"): ("c_float_Array_16", "XybParams")}


def test_nothing_public_moved():
    from record_lib_abi import snapshot
    from jxl_rs_amd import lib
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "lib_public_abi.json")))
    got = snapshot(lib)
    assert len(want["names"]) == 97 and len(want["functions"]) == 135
    for name, w in want["names"].items():
        g = got["names"].get(name)
        assert g is not None, f"lib.{name} is gone"
        if w["kind"] != "struct":
            assert g == w, name
            continue
        assert g["kind"] == "struct" and g["size"] == w["size"], name
        assert [r[:1] + r[2:] for r in g["fields"]] == [r[:1] + r[2:] for r in w["fields"]], name  # field, offset, size
        for gr, wr in zip(g["fields"], w["fields"]):
            assert (wr[1], gr[1]) == RETYPED.get((name, wr[0]), (wr[1], wr[1])), (name, wr[0])
    for name, w in want["functions"].items():
        g = got["functions"].get(name)
        assert g is not None, name
        assert g["ret"] == w["ret"], name
        if w["args"] is not None:  # jxlh_abi_version carried a return type alone
            assert g["args"] == w["args"], name


def test_bind_covers_every_entry_point():
    import gen_py_binding as g
    from jxl_rs_amd import lib
    L = lib.load()
    arity = {f[0]: len(f[2]) for h in (g.HEADER, g.DEV_HEADER) for f in g.parse_header(open(h).read())[4]}
    assert len(arity) == 137 and sorted(arity) == sorted(lib.ABI_SYMBOLS + lib.DEV_SYMBOLS)
    for name, n in arity.items():
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == n, name


def test_bind_skips_what_the_library_lacks():
    from jxl_rs_amd import _abi
    have = ["jxlh_frame_run", "jxlh_ctx_destroy", "jxlh_status_string", "jxlh_live_resources"]
    stand_in = types.SimpleNamespace(**{n: types.SimpleNamespace() for n in have})
    assert _abi.bind(stand_in) is stand_in
    assert sorted(vars(stand_in)) == sorted(have)
    assert stand_in.jxlh_frame_run.argtypes == [C.c_void_p, C.c_uint32, C.c_uint32] and stand_in.jxlh_frame_run.restype is C.c_int32
    assert stand_in.jxlh_ctx_destroy.restype is None and stand_in.jxlh_status_string.restype is C.c_char_p
    assert len(stand_in.jxlh_live_resources.argtypes) == 1


def test_struct_pointer_parameters_take_structs_and_addresses():
    """a `struct*` parameter takes the struct (by reference, as POINTER(struct) does), byref(struct), an address, None"""
    from jxl_rs_amd import lib
    L = lib.load()
    p = lib.FrameParams()
    assert L.jxlh_default_frame_params(p, 40, 24) == lib.OK and (p.xsize, p.ysize) == (40, 24)
    assert L.jxlh_default_frame_params(C.byref(p), 41, 25) == lib.OK and (p.xsize, p.ysize) == (41, 25)
    assert L.jxlh_default_frame_params(C.c_void_p(C.addressof(p)), 42, 26) == lib.OK and (p.xsize, p.ysize) == (42, 26)
    assert L.jxlh_default_frame_params(C.addressof(p), 43, 27) == lib.OK and (p.xsize, p.ysize) == (43, 27)
    assert L.jxlh_default_frame_params(None, 1, 1) == lib.ERR_INVALID_ARGUMENT
