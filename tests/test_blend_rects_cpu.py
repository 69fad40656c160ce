"""include/jxl_hip_blend_rects.h without a device: the header compiles as C in either include order, its three symbols
are exported and bound, both binding generators are current and every older per-header symbol list holds what it held;
the cap protocol and null handling of jxlh_blend_image_rects; the mapping against a numpy restatement over origins from
(-2^31, -2^31) to (2^30, 2^30); and the non-vacuity of every frame case tests/test_gpu_blend_rects.py runs, on the oracle
and blending_ref.blend_frame: in every rect at least half of the pixels change, on both sides of a frame edge it
straddles -- a device test cannot pass by writing nothing.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import blend_rects_cases as bc
import blending_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SYMBOLS = ["jxlh_blend_image_rects", "jxlh_frame_blend_rects", "jxlh_stage_blend_rects"]
# the per-header lists as they were before this header existed
OLDER = {
    "ABI_SYMBOLS": 121, "PREVIEW_SYMBOLS": 2, "SAVE_RECTS_SYMBOLS": 4, "PREVIEW_TILES_SYMBOLS": 2, "EXTRA_RECTS_SYMBOLS": 4,
    "REPAINT_SYMBOLS": 2, "LOCAL_PALETTE_SYMBOLS": 4, "LOCAL_SQUEEZE_SYMBOLS": 5,
}


def test_header_compiles_as_c_and_its_symbols_are_exported(tmp_path):
    import gen_rust_binding as g
    from jxl_rs_amd import _abi, lib
    parsed = g.parse_header(open(g.BLEND_RECTS_HEADER).read())
    declared = [f[0] for f in parsed[4]]
    assert declared == SYMBOLS == _abi.BLEND_RECTS_SYMBOLS
    assert not parsed[0] and not parsed[1] and not parsed[2], "no new constants or structs"
    others = (_abi.ABI_SYMBOLS + _abi.DEV_SYMBOLS + _abi.PREVIEW_SYMBOLS + _abi.SAVE_RECTS_SYMBOLS + _abi.PREVIEW_TILES_SYMBOLS +
              _abi.EXTRA_RECTS_SYMBOLS + _abi.REPAINT_SYMBOLS + _abi.LOCAL_PALETTE_SYMBOLS + _abi.LOCAL_SQUEEZE_SYMBOLS)
    assert not set(SYMBOLS) & set(others)
    L = lib.load()
    for name, nargs in zip(SYMBOLS, (8, 5, 11)):
        fn = getattr(L, name)  # AttributeError: declared but not exported
        assert fn.restype is C.c_int32 and len(fn.argtypes) == nargs, name
    main = open(g.HEADER).read()
    assert '#include "jxl_hip_blend_rects.h"' in main
    code = re.sub(r"/\*.*?\*/", "", main, flags=re.S)
    assert re.search(r"#define\s+JXLH_ABI_VERSION\s+6\b", code) and lib.ABI_VERSION == 6 and L.jxlh_abi_version() == 6
    for name in SYMBOLS:
        assert name not in code, "declared in the header of its own only"
    for i, first in enumerate(("jxl_hip.h", "jxl_hip_blend_rects.h")):
        src = os.path.join(str(tmp_path), f"order{i}.c")
        with open(src, "w") as f:
            f.write(f'#include "{first}"\n#include "jxl_hip_blend_rects.h"\n#include "jxl_hip.h"\n'
                    "jxlh_status (*map)(const jxlh_blend_desc*, uint32_t, uint32_t, const jxlh_rect*, uint32_t, jxlh_rect*,\n"
                    "                   uint32_t, uint32_t*) = jxlh_blend_image_rects;\n"
                    "jxlh_status (*blend)(jxlh_ctx*, const jxlh_blend_desc*, const jxlh_output_desc*, const jxlh_rect*, uint32_t) =\n"
                    "    jxlh_frame_blend_rects;\n"
                    "jxlh_status (*stage)(jxlh_ctx*, const jxlh_blend_desc*, const float* const[], uint32_t, uint32_t, uint32_t,\n"
                    "                     size_t, const jxlh_rect*, uint32_t, float* const[], size_t) = jxlh_stage_blend_rects;\n"
                    "int main(void) { return 0; }\n")
        r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", src,
                            "-o", os.path.join(str(tmp_path), f"order{i}.o")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]


def test_generators_are_current_and_the_older_lists_are_unchanged():
    import gen_py_binding
    import gen_rust_binding as g
    from jxl_rs_amd import _abi, lib
    for tool in ("gen_py_binding.py", "gen_rust_binding.py"):
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--check"], check=True)
    assert open(gen_py_binding.OUT).read() == gen_py_binding.generate()
    rust = open(g.OUT_BLEND_RECTS).read()
    assert rust == g.generate_blend_rects() and "pub mod blend_rects;" in open(g.OUT).read()
    for name in SYMBOLS:
        assert f"pub fn {name}(" in rust, name
        assert name in _abi.SIGNATURES
    # every older list: declared by its own header, in order, and of the length it had
    headers = {"PREVIEW_SYMBOLS": g.PREVIEW_HEADER, "SAVE_RECTS_SYMBOLS": g.SAVE_RECTS_HEADER,
               "PREVIEW_TILES_SYMBOLS": g.PREVIEW_TILES_HEADER, "EXTRA_RECTS_SYMBOLS": g.EXTRA_RECTS_HEADER,
               "REPAINT_SYMBOLS": g.REPAINT_HEADER, "LOCAL_PALETTE_SYMBOLS": g.LOCAL_PALETTE_HEADER,
               "LOCAL_SQUEEZE_SYMBOLS": g.LOCAL_SQUEEZE_HEADER, "ABI_SYMBOLS": g.HEADER}
    for listname, header in headers.items():
        names = [f[0] for f in g.parse_header(open(header).read())[4]]
        assert getattr(_abi, listname) == names, listname
        if listname in OLDER:
            assert len(names) == OLDER[listname], listname
    assert _abi.SAVE_RECTS_SYMBOLS == ["jxlh_frame_save_rects", "jxlh_frame_save_rects_async", "jxlh_stage_save_rects",
                                       "jxlh_changed_rects"]
    assert _abi.REPAINT_SYMBOLS == ["jxlh_frame_repaint_groups", "jxlh_repaint_changed_rects"]
    # the layers above name the calls
    hpp = open(os.path.join(ROOT, "include", "jxl_hip.hpp")).read()
    pipe = open(os.path.join(ROOT, "include", "jxl_hip_pipeline.hpp")).read()
    for name in SYMBOLS[:2]:
        assert name + "(" in hpp, name
    for name in ("do_render_rects", "repaint_rects", "repaint_groups_rects"):
        assert name + "(" in pipe, name
    for name in ("blend_rects", "try_blend_rects", "stage_blend_rects", "try_stage_blend_rects"):
        assert hasattr(lib.Context, name), name
    assert callable(lib.blend_image_rects) and callable(lib.try_blend_image_rects)


def _desc(x0, y0, iw, ih):
    from jxl_rs_amd import lib
    return lib.blend_desc(x0, y0, iw, ih, (lib.BLEND_REPLACE, 0, 0, 0))


def test_cap_protocol_and_null_handling():
    from jxl_rs_amd import lib
    L = lib.load()
    INV = lib.ERR_INVALID_ARGUMENT
    d = _desc(-7, 5, 400, 280)
    rects = np.array([[0, 0, 10, 10], [600, 0, 5, 5], [100, 100, 50, 50], [0, 0, 0, 9]], dtype=np.uint32)  # two survive
    out = np.zeros((8, 4), dtype=np.uint32)
    n = C.c_uint32(77)

    def call(dd, r, count, o, cap, nn):
        return L.jxlh_blend_image_rects(dd, 520, 300, None if r is None else r.ctypes.data, count,
                                        None if o is None else o.ctypes.data, cap, nn)
    # the count comes back with cap 0; a cap that is too small is an argument error that still names the count
    assert call(d, rects, 4, None, 0, C.byref(n)) == INV and n.value == 2
    assert call(d, rects, 4, out, 1, C.byref(n)) == INV and n.value == 2 and not out.any()
    assert call(d, rects, 4, out, 2, C.byref(n)) == lib.OK and n.value == 2
    assert out[:2].tolist() == [[0, 5, 3, 10], [93, 105, 50, 50]] and not out[2:].any()
    assert call(d, None, 0, None, 0, C.byref(n)) == lib.OK and n.value == 0
    assert call(d, rects[1:2], 1, None, 0, C.byref(n)) == lib.OK and n.value == 0  # everything dropped: nothing needed
    for bad in ((None, rects, 4, out, 8, C.byref(n)), (d, None, 4, out, 8, C.byref(n)), (d, rects, 4, None, 8, C.byref(n)),
                (d, rects, 4, out, 8, None)):
        assert call(*bad) == INV
    assert lib.try_blend_image_rects(d, 520, 300, rects)[0] == lib.OK
    assert lib.try_blend_image_rects(d, 520, 300, rects, cap=1)[::2] == (INV, 2)
    assert lib.blend_image_rects(d, 520, 300, []).shape == (0, 4)


def _restated(x0, y0, iw, ih, fw, fh, rects):
    """shift, clip, drop -- in Python integers"""
    ox, oy = min(max(x0, -(1 << 30)), 1 << 30), min(max(y0, -(1 << 30)), 1 << 30)
    out = []
    for rx, ry, rw, rh in rects:
        fx0, fy0, fx1, fy1 = rx, ry, min(rx + rw, fw), min(ry + rh, fh)
        ax, ay, bx, by = max(fx0 + ox, 0), max(fy0 + oy, 0), min(fx1 + ox, iw), min(fy1 + oy, ih)
        if fx0 < fx1 and fy0 < fy1 and ax < bx and ay < by:
            out.append([ax, ay, bx - ax, by - ay])
    return out


@pytest.mark.parametrize("fw,fh", [(300, 260), (9, 9)])
@pytest.mark.parametrize("iw,ih", [(1, 1), (400, 280), (517, 11)])
def test_mapping_is_the_restatement(fw, fh, iw, ih):
    from jxl_rs_amd import lib
    rng = np.random.default_rng(fw * 1000 + iw)
    # the eight positions around and across each image edge, and the extremes
    xs = [-(1 << 31), -(1 << 30) - 1, -(1 << 30), -fw - 1, -fw, -fw + 1, -fw // 2, -1, 0, 1, iw - fw - 1, iw - fw, iw - fw + 1,
          iw - fw // 2, iw - 1, iw, iw + 1, 1 << 30]
    ys = [-(1 << 31), -(1 << 30), -fh - 1, -fh, -fh + 1, -fh // 2, -1, 0, 1, ih - fh - 1, ih - fh, ih - fh + 1, ih - fh // 2,
          ih - 1, ih, ih + 1, 1 << 30]
    fixed = [(0, 0, fw, fh), (0, 0, 0xffffffff, 0xffffffff), (fw, 0, 5, 5), (0, fh, 5, 5), (fw - 1, fh - 1, 0xffffffff, 0xffffffff),
             (0xfffffff0, 0xfffffff0, 0xff, 0xff), (1, 1, 0, 5), (1, 1, 5, 0)]
    seen = 0
    for x0 in xs:
        for y0 in ys:
            rects = fixed + [(int(rng.integers(0, fw + 3)), int(rng.integers(0, fh + 3)), int(rng.integers(0, fw + 2)),
                              int(rng.integers(0, fh + 2))) for _ in range(6)]
            got = lib.blend_image_rects(_desc(x0, y0, iw, ih), fw, fh, rects)
            want = _restated(x0, y0, iw, ih, fw, fh, rects)
            assert got.tolist() == want, (x0, y0, got.tolist()[:3], want[:3])
            seen += len(want)
    assert seen > 100


# ---------------------------------------------------------------- the frame cases' non-vacuity, on the oracle
def test_case_check_vardct_sequence(oracle):
    """one group arrives again: the mapped changed rect, under Blend on an alpha channel and under Replace"""
    from jxl_rs_amd import lib
    fa, fab, _ = bc.frames(oracle)
    p = bc.frame_params(*bc.FRAME)
    rects = lib.changed_rects(p, [bc.GROUP])
    for name, d in bc.DESCS.items():
        refs = {0: bc.slot_planes(11, 3 + len(d.ec))}
        image_rects = bc.frame_rects(d, *bc.FRAME, rects)
        assert len(image_rects) == 1
        bc.check_case(d, *bc.FRAME, br.blend_frame(bc.with_ec(oracle, fa, d), refs, d),
                      br.blend_frame(bc.with_ec(oracle, fab, d), refs, d), image_rects, name)
        # ... and the rect is needed: outside it nothing changes, so the whole image can be expected to be the new frame's
        diff = bc.differing(br.blend_frame(bc.with_ec(oracle, fa, d), refs, d), br.blend_frame(bc.with_ec(oracle, fab, d), refs, d))
        assert not (diff & ~bc.union_mask(image_rects, *bc.IMAGE)).any(), name


def test_case_check_stale_outside(oracle):
    d = bc.DESCS["blend_alpha"]
    fa, _, fb = bc.frames(oracle)
    s1, s2 = {0: bc.slot_planes(11, 4)}, {0: bc.slot_planes(12, 4)}
    old = br.blend_frame(bc.with_ec(oracle, fa, d), s1, d)
    bc.check_case(d, *bc.FRAME, old, br.blend_frame(bc.with_ec(oracle, fb, d), s2, d), bc.STALE_RECTS, "frame and slot change")
    box = bc.frame_box(d.x0, d.y0, *bc.FRAME, *bc.IMAGE)
    assert sum(1 for r in bc.STALE_RECTS if r[2] and r[3] and bc.meets(r, box) and r[1] < box[1]) >= 2  # across the top edge
    assert any(r[2] and r[3] and not bc.meets(r, box) for r in bc.STALE_RECTS)                        # extend only
    assert all(not bc.meets(r, box) for r in bc.EXTEND_RECTS)
    bc.check_case(d, *bc.FRAME, old, br.blend_frame(bc.with_ec(oracle, fa, d), s2, d), bc.EXTEND_RECTS, "the slot changes")
    # outside the union the two expectations differ as well: stale pixels show
    for new, rects in ((br.blend_frame(bc.with_ec(oracle, fb, d), s2, d), bc.STALE_RECTS),
                       (br.blend_frame(bc.with_ec(oracle, fa, d), s2, d), bc.EXTEND_RECTS)):
        assert (bc.differing(old, new) & ~bc.union_mask(rects, *bc.IMAGE)).mean() > 0.5


def test_case_check_other_routes(oracle):
    from jxl_rs_amd import lib
    from test_gpu_blending import _oracle_colour
    # upsampled
    d, n = bc.UPS_DESC, bc.UPS_N
    fw, fh = bc.UPS_CODED[0] * n, bc.UPS_CODED[1] * n
    before, after = bc.ups_frames(oracle)
    refs = {2: bc.slot_planes(13, 3, (d.image_w, d.image_h))}
    rects = bc.frame_rects(d, fw, fh, lib.repaint_changed_rects(bc.frame_params(*bc.UPS_CODED, n=n), [bc.UPS_GROUP]))
    assert len(rects) == 1
    bc.check_case(d, fw, fh, br.blend_frame(before, refs, d), br.blend_frame(after, refs, d), rects, "upsampled")
    # Modular by cell
    d = bc.MOD_DESC
    before, after = bc.mod_frames(oracle)
    refs = {1: [p + np.float32(0.25) for p in bc.slot_planes(14, 3, (d.image_w, d.image_h))]}
    rects = bc.frame_rects(d, *bc.MOD_SIZE, lib.repaint_changed_rects(bc.frame_params(*bc.MOD_SIZE, modular=True), [bc.MOD_CELL]))
    assert len(rects) == 1
    bc.check_case(d, *bc.MOD_SIZE, br.blend_frame(before, refs, d), br.blend_frame(after, refs, d), rects, "Modular")
    # an alpha channel by rects
    d = bc.DESCS["blend_alpha"]
    fa, fab, _ = bc.frames(oracle)
    first, new = bc.ec_planes()
    refs = {0: bc.slot_planes(11, 4)}
    w, h = bc.FRAME
    rects = bc.frame_rects(d, w, h, lib.extra_channel_changed_rects(w, h, 1, w, h, [bc.EC_UPDATE]))
    bc.check_case(d, w, h, br.blend_frame(list(fa) + [oracle.modular_to_f32(first, 16, 0)], refs, d),
                  br.blend_frame(list(fa) + [oracle.modular_to_f32(new, 16, 0)], refs, d), rects, "alpha by rects")
    # a colour stage in front
    d = br.BlendDesc(*bc.ORIGIN, *bc.IMAGE, (br.ADD, 0, True, 0), [], [])
    refs = {0: bc.slot_planes(15, 3)}
    rects = bc.frame_rects(d, w, h, lib.changed_rects(bc.frame_params(w, h), [bc.GROUP]))
    bc.check_case(d, w, h, br.blend_frame(_oracle_colour(oracle, fa, "xyb", "srgb", 0.0), refs, d),
                  br.blend_frame(_oracle_colour(oracle, fab, "xyb", "srgb", 0.0), refs, d), rects, "sRGB in front")
