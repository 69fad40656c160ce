"""include/jxl_hip_local_extra.h without a device: the header compiles as C11 in either include order, its two symbols are
exported and bound and belong to no other list, the ABI version is 6, every older per-header list has the length it had,
both binding generators are current, jxlh_local_dest has one layout for gcc, ctypes and Rust's repr(C) rules, and the C++
and Python layers name the calls.  And the proof on the oracle that the inputs of tests/test_gpu_modular_local_extra.py
(tests/modular_local_extra_cases.py) can tell mistakes apart:
  * every finished channel differs from every coded channel of its group and from every other finished channel on more
    than half of its samples (a channel no step touches IS its coded channel -- the step list "none", the alpha beside an
    RCT -- and is held to the other coded channels and to the finished ones): a plain copy or a slot mix-up cannot pass;
  * for the palettes over all four channels at least 5 % of the indices fall on each of explicit entries, implicit
    entries and (general palettes) delta entries.
These are conditions on the inputs, asserted for the seeds the GPU tests use.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import modular_local_extra_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SYMBOLS = ["jxlh_frame_set_modular_groups_extra", "jxlh_frame_set_modular_groups_extra_async"]
# the per-header lists as they were before this header existed
OLDER = {
    "ABI_SYMBOLS": 121, "PREVIEW_SYMBOLS": 2, "SAVE_RECTS_SYMBOLS": 4, "PREVIEW_TILES_SYMBOLS": 2, "EXTRA_RECTS_SYMBOLS": 4,
    "REPAINT_SYMBOLS": 2, "LOCAL_PALETTE_SYMBOLS": 4, "LOCAL_SQUEEZE_SYMBOLS": 5, "BLEND_RECTS_SYMBOLS": 3,
}


def test_header_compiles_as_c_and_its_symbols_are_exported(tmp_path):
    import gen_rust_binding as g
    from jxl_rs_amd import _abi, lib
    parsed = g.parse_header(open(g.LOCAL_EXTRA_HEADER).read())
    declared = [f[0] for f in parsed[4]]
    assert declared == SYMBOLS == _abi.LOCAL_EXTRA_SYMBOLS == lib.LOCAL_EXTRA_SYMBOLS
    assert not parsed[0] and not parsed[1] and [s[0] for s in parsed[2]] == ["jxlh_local_dest"], "one struct, no constants"
    others = (_abi.ABI_SYMBOLS + _abi.DEV_SYMBOLS + _abi.PREVIEW_SYMBOLS + _abi.SAVE_RECTS_SYMBOLS + _abi.PREVIEW_TILES_SYMBOLS +
              _abi.EXTRA_RECTS_SYMBOLS + _abi.REPAINT_SYMBOLS + _abi.LOCAL_PALETTE_SYMBOLS + _abi.LOCAL_SQUEEZE_SYMBOLS +
              _abi.BLEND_RECTS_SYMBOLS)
    assert not set(SYMBOLS) & set(others)
    L = lib.load()
    for name in SYMBOLS:
        fn = getattr(L, name)  # AttributeError: declared but not exported
        assert fn.restype is C.c_int32 and len(fn.argtypes) == 13, name
    main = open(g.HEADER).read()
    assert main.rstrip().endswith('#include "jxl_hip_local_extra.h"\n\n#endif /* JXL_HIP_H_ */'), "included at the header's end"
    code = re.sub(r"/\*.*?\*/", "", main, flags=re.S)
    assert re.search(r"#define\s+JXLH_ABI_VERSION\s+6\b", code) and lib.ABI_VERSION == 6 and L.jxlh_abi_version() == 6
    for name in SYMBOLS:
        assert name not in code, "declared in the header of its own only"
        for h in ("jxl_hip_local_squeeze.h", "jxl_hip_local_palette.h", "jxl_hip_extra_rects.h"):
            assert name not in re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
    for i, first in enumerate(("jxl_hip.h", "jxl_hip_local_extra.h", "jxl_hip_local_squeeze.h", "jxl_hip_local_palette.h",
                               "jxl_hip_extra_rects.h")):
        src = os.path.join(str(tmp_path), f"order{i}.c")
        with open(src, "w") as f:
            f.write(f'#include "{first}"\n#include "jxl_hip.h"\n'
                    "typedef jxlh_status (*call)(jxlh_ctx*, const int32_t*, uint64_t, const jxlh_local_squeeze_group*, size_t,\n"
                    "                            const jxlh_local_coded_channel*, size_t, const jxlh_squeeze_params*, size_t,\n"
                    "                            const jxlh_wp_header*, uint32_t, const jxlh_local_dest*, size_t*);\n"
                    "call a = jxlh_frame_set_modular_groups_extra, b = jxlh_frame_set_modular_groups_extra_async;\n"
                    "jxlh_local_dest d = {3, 1, {0, 0, 0, 0}, 0};\n"
                    "int main(void) { return (int)d.n_ec - 1; }\n")
        r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), src,
                            "-o", src + ".o"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]


def test_generators_are_current_and_older_lists_keep_their_lengths():
    import gen_py_binding
    import gen_rust_binding as g
    from jxl_rs_amd import _abi
    for tool in ("gen_py_binding.py", "gen_rust_binding.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--check"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    assert open(gen_py_binding.OUT).read() == gen_py_binding.generate()
    rust = open(g.OUT_LOCAL_EXTRA).read()
    assert rust == g.generate_local_extra() and "pub mod local_extra;" in open(g.OUT).read()
    for name in SYMBOLS:
        assert f"pub fn {name}(" in rust and name in _abi.SIGNATURES
    for listname, n in OLDER.items():
        assert len(getattr(_abi, listname)) == n, listname
    headers = {"PREVIEW_SYMBOLS": g.PREVIEW_HEADER, "SAVE_RECTS_SYMBOLS": g.SAVE_RECTS_HEADER,
               "PREVIEW_TILES_SYMBOLS": g.PREVIEW_TILES_HEADER, "EXTRA_RECTS_SYMBOLS": g.EXTRA_RECTS_HEADER,
               "REPAINT_SYMBOLS": g.REPAINT_HEADER, "LOCAL_PALETTE_SYMBOLS": g.LOCAL_PALETTE_HEADER,
               "LOCAL_SQUEEZE_SYMBOLS": g.LOCAL_SQUEEZE_HEADER, "BLEND_RECTS_SYMBOLS": g.BLEND_RECTS_HEADER, "ABI_SYMBOLS": g.HEADER}
    for listname, header in headers.items():
        assert getattr(_abi, listname) == [f[0] for f in g.parse_header(open(header).read())[4]], listname


def test_struct_layout_gcc_ctypes_rust(tmp_path):
    import gen_rust_binding as g
    from jxl_rs_amd import lib
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "jxl_hip_local_extra.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(jxlh_local_dest), _Alignof(jxlh_local_dest),\n'
                   "         offsetof(jxlh_local_dest, n_colour), offsetof(jxlh_local_dest, n_ec), offsetof(jxlh_local_dest, ec),\n"
                   "         offsetof(jxlh_local_dest, bit_depth));\n  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    D = lib.LocalDest
    assert got == [C.sizeof(D), C.alignment(D), D.n_colour.offset, D.n_ec.offset, D.ec.offset, D.bit_depth.offset] == [28, 4, 0, 4, 8, 24]
    # Rust's repr(C): fields in declaration order, each at the next multiple of its alignment, the size rounded up to the
    # struct's -- from the generated module's own field list
    m = re.search(r"pub struct jxlh_local_dest \{(.*?)\n\}", open(g.OUT_LOCAL_EXTRA).read(), flags=re.S)
    fields = re.findall(r"pub (\w+): ([^,\n]+),", m.group(1))
    assert [f for f, _ in fields] == [f for f, _ in D._fields_]
    size = {"u32": (4, 4), "[u32; 4]": (16, 4)}
    at, align, offs = 0, 1, []
    for _, ty in fields:
        n, a = size[ty]
        at = -(-at // a) * a
        offs.append(at)
        at += n
        align = max(align, a)
    assert offs == got[2:] and -(-at // align) * align == got[0] and align == got[1]
    assert "#[repr(C)]" in open(g.OUT_LOCAL_EXTRA).read()


def test_layers_name_the_calls():
    from jxl_rs_amd import lib
    assert callable(lib.Context.set_modular_groups_extra) and callable(lib.Context.try_set_modular_groups_extra)
    d = lib.local_dest(3, [2])
    assert (d.n_colour, d.n_ec, list(d.ec), d.bit_depth) == (3, 1, [2, 0, 0, 0], 0)
    d = lib.local_dest(0, [1, 0, 3], bit_depth=12)
    assert (d.n_colour, d.n_ec, list(d.ec), d.bit_depth) == (0, 3, [1, 0, 3, 0], 12)
    hpp = open(os.path.join(ROOT, "include", "jxl_hip.hpp")).read()
    assert "void set_modular_groups_extra(" in hpp and "jxlh_frame_set_modular_groups_extra_async(" in hpp
    pipe = open(os.path.join(ROOT, "include", "jxl_hip_pipeline.hpp")).read()
    assert re.search(r"void set_groups\([^)]*const LocalSqueezeGroups& batch, const jxlh_local_dest& dest", pipe)
    assert re.search(r"void set_extra_groups\([^)]*const jxlh_local_dest& dest", pipe)
    rust = open(os.path.join(ROOT, "bindings", "rust", "jxl_hip", "src", "lib.rs")).read()
    assert "pub fn set_modular_groups_extra(" in rust and "sys::local_extra::jxlh_frame_set_modular_groups_extra(" in rust


def test_calls_validate_before_touching_the_device():
    from jxl_rs_amd import lib
    L = lib.load()
    sp = ec.spec("none", 1, 0, 0, 8, 8, 4)
    arena, (groups, coded, params) = lib.pack_local_squeeze_groups([sp])
    d = lib.local_dest(3, [0])
    a = (arena.ctypes.data, arena.size, groups, 1, coded, len(coded), params, len(params), None, 8)
    for fn in (L.jxlh_frame_set_modular_groups_extra, L.jxlh_frame_set_modular_groups_extra_async):
        assert fn(None, *a, C.byref(d), None) == lib.ERR_INVALID_ARGUMENT


# ---------------------------------------------------------------- the inputs are not vacuous
def _pairs():
    out = []
    for layout, (n_colour, n_ec) in ec.LAYOUTS.items():
        n = n_colour + n_ec
        frames = [ec.ALIGNED, ec.RAGGED] if layout == "rgba" else [ec.GREY] if n_colour == 1 else [(128, 128, 128)]
        for name in ec.lists_for(n):
            for frame in frames:
                out.append((layout, name, frame))
    return out


@pytest.mark.parametrize("layout,name,frame", _pairs(), ids=lambda v: v if isinstance(v, str) else "%dx%d" % v[:2])
def test_inputs_tell_mistakes_apart(oracle, layout, name, frame):
    n = sum(ec.LAYOUTS[layout])
    for sp in ec.frame_specs(name, frame, n):
        if sp["w"] * sp["h"] < 64:
            continue  # (the 11 x 9 corner cell: shares of so few samples say nothing)
        fin = ec.finished(oracle, sp)
        assert len(fin) == n and all(f.shape == (sp["h"], sp["w"]) for f in fin)
        changed = ec.touched(sp)
        for c, f in enumerate(fin):
            same = [k for k, cd in enumerate(sp["coded"]) if cd.shape == f.shape and np.array_equal(cd, f)]
            if c in changed:
                assert not same, (c, "a touched channel equals a coded one")
            else:
                assert len(same) == 1, (c, "an untouched channel is exactly its coded channel")
            for k, cd in enumerate(sp["coded"]):
                if cd.shape == f.shape and k not in same:
                    assert float((cd != f).mean()) > 0.5, (name, c, k, float((cd != f).mean()))
            for c2 in range(c):
                assert float((fin[c2] != f).mean()) > 0.5, (name, c2, c, float((fin[c2] != f).mean()))
        if n == 4 and name in ("palette_all", "general_p0", "general_p5", "general_p6", "general_p13"):
            step = sp["ref_steps"][0]
            assert len(sp["index_planes"]) == 1
            shares = ec.arm_shares(sp["index_planes"][0], step["num_colors"], step["num_deltas"])
            print(name, shares)
            for arm in ("explicit", "implicit") + (("delta",) if step["num_deltas"] else ()):
                assert shares[arm] >= 0.05, (name, arm, shares)
