#!/usr/bin/env python3
"""Generates the raw Rust binding of include/jxl_hip.h (the `jxl_hip_sys` crate a jxl-rs maintainer would add):

    python tools/gen_rust_binding.py            # rewrites bindings/rust/jxl_hip_sys/src/lib.rs
    python tools/gen_rust_binding.py --check    # exit 1 if the committed file is stale

The header is the single source of truth: every struct (#[repr(C)], same field order), every status / flag constant
and every entry point is derived from it, so the binding cannot drift from the ABI the way a hand-pasted block does.
tests/test_rust_binding.py runs --check and compares the struct layouts with the C compiler's.
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jxl_hip.h")
OUT = os.path.join(ROOT, "bindings", "rust", "jxl_hip_sys", "src", "lib.rs")
# entry points added in headers of their own (included by jxl_hip.h): one module of the crate each
PREVIEW_HEADER = os.path.join(ROOT, "include", "jxl_hip_preview.h")
OUT_PREVIEW = os.path.join(ROOT, "bindings", "rust", "jxl_hip_sys", "src", "preview.rs")
SAVE_RECTS_HEADER = os.path.join(ROOT, "include", "jxl_hip_save_rects.h")
OUT_SAVE_RECTS = os.path.join(ROOT, "bindings", "rust", "jxl_hip_sys", "src", "save_rects.rs")
PREVIEW_TILES_HEADER = os.path.join(ROOT, "include", "jxl_hip_preview_tiles.h")
OUT_PREVIEW_TILES = os.path.join(ROOT, "bindings", "rust", "jxl_hip_sys", "src", "preview_tiles.rs")
EXTRA_RECTS_HEADER = os.path.join(ROOT, "include", "jxl_hip_extra_rects.h")
OUT_EXTRA_RECTS = os.path.join(ROOT, "bindings", "rust", "jxl_hip_sys", "src", "extra_rects.rs")
REPAINT_HEADER = os.path.join(ROOT, "include", "jxl_hip_repaint.h")
OUT_REPAINT = os.path.join(ROOT, "bindings", "rust", "jxl_hip_sys", "src", "repaint.rs")
BLEND_RECTS_HEADER = os.path.join(ROOT, "include", "jxl_hip_blend_rects.h")
OUT_BLEND_RECTS = os.path.join(ROOT, "bindings", "rust", "jxl_hip_sys", "src", "blend_rects.rs")
# ... and a header that includes jxl_hip.h rather than being included by it
LOCAL_PALETTE_HEADER = os.path.join(ROOT, "include", "jxl_hip_local_palette.h")
OUT_LOCAL_PALETTE = os.path.join(ROOT, "bindings", "rust", "jxl_hip_sys", "src", "local_palette.rs")
LOCAL_SQUEEZE_HEADER = os.path.join(ROOT, "include", "jxl_hip_local_squeeze.h")
OUT_LOCAL_SQUEEZE = os.path.join(ROOT, "bindings", "rust", "jxl_hip_sys", "src", "local_squeeze.rs")
# ... and one that jxl_hip.h includes and that includes those two
LOCAL_EXTRA_HEADER = os.path.join(ROOT, "include", "jxl_hip_local_extra.h")
OUT_LOCAL_EXTRA = os.path.join(ROOT, "bindings", "rust", "jxl_hip_sys", "src", "local_extra.rs")

SCALARS = {"uint8_t": "u8", "int8_t": "i8", "uint16_t": "u16", "int16_t": "i16", "uint32_t": "u32", "int32_t": "i32",
           "uint64_t": "u64", "int64_t": "i64", "size_t": "usize", "float": "f32", "double": "f64", "char": "c_char",
           "void": "c_void", "jxlh_status": "jxlh_status"}


def strip_comments(src):
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def rust_base(name):
    return SCALARS.get(name, name)


def parse_declarator(text):
    """'const float* const tables[17]' -> (rust type, name).  Array parameters decay to pointers."""
    text = text.strip()
    arr = None
    m = re.search(r"\[(\w*)\]\s*$", text)
    if m:
        arr = m.group(1)
        text = text[:m.start()].strip()
    m = re.search(r"(\w+)$", text)
    name = m.group(1)
    left = text[:m.start()].strip()
    toks = re.findall(r"\w+|\*", left)
    # base type with its constness
    const = False
    base = None
    i = 0
    while i < len(toks) and toks[i] != "*":
        if toks[i] == "const":
            const = True
        elif toks[i] != "struct":
            base = toks[i]
        i += 1
    ty, ty_const = rust_base(base), const
    while i < len(toks):
        if toks[i] == "*":
            ty = ("*const " if ty_const else "*mut ") + ty
            ty_const = False
        elif toks[i] == "const":
            ty_const = True
        i += 1
    return ty, ty_const, name, arr


def param_type(text):
    ty, ty_const, name, arr = parse_declarator(text)
    if arr is not None:  # array parameter: pointer to the element
        ty = ("*const " if ty_const else "*mut ") + ty
    return ty, name


def parse_header(src):
    src = strip_comments(src)
    defines = re.findall(r"^#define\s+(JXLH_\w+)\s+(\d+)\s*$", src, flags=re.M)
    enums = []
    for body in re.findall(r"enum\s*\{(.*?)\}\s*;", src, flags=re.S):
        for item in body.split(","):
            item = item.strip()
            if not item:
                continue
            m = re.match(r"(\w+)\s*=\s*(.+)$", item, flags=re.S)
            enums.append((m.group(1), " ".join(m.group(2).split())))
    structs = []
    for m in re.finditer(r"typedef\s+struct\s*(\w*)\s*\{(.*?)\}\s*(\w+)\s*;", src, flags=re.S):
        fields = []
        for decl in m.group(2).split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            first, *rest = [d.strip() for d in decl.split(",")]
            ty, _, name, arr = parse_declarator(first)
            prefix = first[:first.rindex(name)] if arr is None else first[:re.search(r"\w+\s*\[", first).start()]
            fields.append((ty, name, arr))
            for r in rest:  # 'float gab_w1[3], gab_w2[3]': further declarators share the base type
                t2, _, n2, a2 = parse_declarator(prefix + r)
                fields.append((t2, n2, a2))
        structs.append((m.group(3), fields))
    opaque = re.findall(r"typedef\s+struct\s+(\w+)\s+(\w+)\s*;", src)
    funcs = []
    body = re.sub(r"typedef\s+struct\s*\w*\s*\{.*?\}\s*\w+\s*;", "", src, flags=re.S)
    for m in re.finditer(r"^\s*((?:const\s+)?\w+\s*\**)\s*(jxlh_\w+)\s*\(([^;{]*?)\)\s*;", body, flags=re.S | re.M):
        ret = " ".join(m.group(1).split())
        params = " ".join(m.group(3).split())
        plist = [] if params in ("void", "") else [param_type(p) for p in params.split(",")]
        rty, rconst, _, _ = parse_declarator(ret + " x")
        funcs.append((m.group(2), rty, plist))
    return defines, enums, structs, opaque, funcs


def emit(defines, enums, structs, opaque, funcs):
    out = []
    w = out.append
    w("// GENERATED by tools/gen_rust_binding.py from include/jxl_hip.h -- do not edit.")
    w("// Raw FFI of libjxl_hip.so (the MI355X-native JPEG XL reconstruction path) for a `jxl_hip_sys` crate.")
    w("#![allow(non_camel_case_types, non_upper_case_globals, dead_code)]")
    w("use std::os::raw::{c_char, c_void};")
    w("")
    w("pub type jxlh_status = i32;")
    for name, val in defines:
        w(f"pub const {name}: u32 = {val};")
    for name, val in enums:
        v = val.replace("1u", "1u32")
        neg = v.startswith("-")
        w(f"pub const {name}: {'i32' if neg or name.startswith(('JXLH_OK', 'JXLH_ERR')) else 'u32'} = {v};")
    w("")
    for _, name in opaque:
        w("#[repr(C)]")
        w(f"pub struct {name} {{")
        w("    _private: [u8; 0],")
        w("}")
    for name, fields in structs:
        w("")
        w("#[repr(C)]")
        w("#[derive(Clone, Copy)]")
        w(f"pub struct {name} {{")
        for ty, fname, arr in fields:
            w(f"    pub {fname}: {ty if arr is None else '[%s; %s]' % (ty, arr)},")
        w("}")
    w("")
    w('#[link(name = "jxl_hip")]')
    w('extern "C" {')
    for name, ret, plist in funcs:
        ps = ", ".join(f"{('r#' + n) if n in ('in', 'type', 'box', 'ref', 'mod') else n}: {t}" for t, n in plist)
        r = "" if ret == "c_void" else f" -> {ret}"
        w(f"    pub fn {name}({ps}){r};")
    w("}")
    w("")
    w("// include/jxl_hip_preview.h (tools/gen_rust_binding.py writes src/preview.rs from it)")
    w("pub mod preview;")
    w("// include/jxl_hip_save_rects.h (... src/save_rects.rs)")
    w("pub mod save_rects;")
    w("// include/jxl_hip_preview_tiles.h (... src/preview_tiles.rs)")
    w("pub mod preview_tiles;")
    w("// include/jxl_hip_extra_rects.h (... src/extra_rects.rs)")
    w("pub mod extra_rects;")
    w("// include/jxl_hip_repaint.h (... src/repaint.rs)")
    w("pub mod repaint;")
    w("// include/jxl_hip_blend_rects.h (... src/blend_rects.rs)")
    w("pub mod blend_rects;")
    w("// include/jxl_hip_local_palette.h (... src/local_palette.rs)")
    w("pub mod local_palette;")
    w("// include/jxl_hip_local_squeeze.h (... src/local_squeeze.rs)")
    w("pub mod local_squeeze;")
    w("// include/jxl_hip_local_extra.h (... src/local_extra.rs)")
    w("pub mod local_extra;")
    return "\n".join(out) + "\n"


def emit_extension(header_name, defines, enums, structs, opaque, funcs, uses=()):
    """a header that adds constants, plain structs and entry points, as a module on top of the crate's types (uses: the
    sibling modules whose structs its signatures name)"""
    assert not opaque, header_name
    out = []
    w = out.append
    w(f"// GENERATED by tools/gen_rust_binding.py from include/{header_name} -- do not edit.")
    w("#![allow(non_camel_case_types, non_upper_case_globals, dead_code)]")
    w("use super::*;")
    for dep in uses:
        w(f"use super::{dep}::*;")
    w("")
    for name, val in defines + enums:
        w(f"pub const {name}: u32 = {val};")
    w("")
    for name, fields in structs:
        w("#[repr(C)]")
        w("#[derive(Clone, Copy)]")
        w(f"pub struct {name} {{")
        for ty, fname, arr in fields:
            w(f"    pub {fname}: {ty if arr is None else '[%s; %s]' % (ty, arr)},")
        w("}")
        w("")
    w('#[link(name = "jxl_hip")]')
    w('extern "C" {')
    for name, ret, plist in funcs:
        ps = ", ".join(f"{n}: {t}" for t, n in plist)
        w(f"    pub fn {name}({ps}) -> {ret};")
    w("}")
    return "\n".join(out) + "\n"


def generate():
    return emit(*parse_header(open(HEADER).read()))


def generate_preview():
    return emit_extension(os.path.basename(PREVIEW_HEADER), *parse_header(open(PREVIEW_HEADER).read()))


def generate_save_rects():
    return emit_extension(os.path.basename(SAVE_RECTS_HEADER), *parse_header(open(SAVE_RECTS_HEADER).read()))


def generate_preview_tiles():
    return emit_extension(os.path.basename(PREVIEW_TILES_HEADER), *parse_header(open(PREVIEW_TILES_HEADER).read()))


def generate_extra_rects():
    return emit_extension(os.path.basename(EXTRA_RECTS_HEADER), *parse_header(open(EXTRA_RECTS_HEADER).read()),
                          uses=("save_rects",))


def generate_repaint():
    return emit_extension(os.path.basename(REPAINT_HEADER), *parse_header(open(REPAINT_HEADER).read()), uses=("save_rects",))


def generate_blend_rects():
    return emit_extension(os.path.basename(BLEND_RECTS_HEADER), *parse_header(open(BLEND_RECTS_HEADER).read()),
                          uses=("save_rects",))


def generate_local_palette():
    return emit_extension(os.path.basename(LOCAL_PALETTE_HEADER), *parse_header(open(LOCAL_PALETTE_HEADER).read()))


def generate_local_squeeze():
    return emit_extension(os.path.basename(LOCAL_SQUEEZE_HEADER), *parse_header(open(LOCAL_SQUEEZE_HEADER).read()),
                          uses=("local_palette",))


def generate_local_extra():
    return emit_extension(os.path.basename(LOCAL_EXTRA_HEADER), *parse_header(open(LOCAL_EXTRA_HEADER).read()),
                          uses=("local_palette", "local_squeeze"))


def main():
    for out, text in ((OUT, generate()), (OUT_PREVIEW, generate_preview()), (OUT_SAVE_RECTS, generate_save_rects()),
                      (OUT_PREVIEW_TILES, generate_preview_tiles()), (OUT_EXTRA_RECTS, generate_extra_rects()),
                      (OUT_REPAINT, generate_repaint()), (OUT_BLEND_RECTS, generate_blend_rects()),
                      (OUT_LOCAL_PALETTE, generate_local_palette()),
                      (OUT_LOCAL_SQUEEZE, generate_local_squeeze()), (OUT_LOCAL_EXTRA, generate_local_extra())):
        if "--check" in sys.argv:
            cur = open(out).read() if os.path.exists(out) else ""
            if cur != text:
                print(f"{os.path.relpath(out, ROOT)} is stale: run tools/gen_rust_binding.py", file=sys.stderr)
                sys.exit(1)
            continue
        os.makedirs(os.path.dirname(out), exist_ok=True)
        open(out, "w").write(text)
        print("wrote", os.path.relpath(out, ROOT))


if __name__ == "__main__":
    main()
