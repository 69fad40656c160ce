"""include/jxl_hip_extra_rects.h without a device: the header compiles as C in either include order and every symbol
it declares is exported and bound; both binding generators are current; the cap protocol and the statuses of
jxlh_extra_channel_changed_rects, and its rule against the oracle (replace a rect's samples, convert and upsample
before and after: no sample outside the returned rect differs); the statuses of the rects call that need no device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SYMBOLS = ["jxlh_frame_begin_extra_channel", "jxlh_frame_set_extra_channel_rects", "jxlh_frame_set_extra_channel_rects_async",
           "jxlh_extra_channel_changed_rects"]


def test_header_compiles_as_c_and_its_symbols_are_exported(tmp_path):
    import gen_rust_binding as g
    from jxl_rs_amd import _abi, lib
    header = open(g.EXTRA_RECTS_HEADER).read()
    declared = [f[0] for f in g.parse_header(header)[4]]
    assert declared == SYMBOLS == _abi.EXTRA_RECTS_SYMBOLS
    assert not set(SYMBOLS) & set(_abi.ABI_SYMBOLS + _abi.DEV_SYMBOLS + _abi.PREVIEW_SYMBOLS + _abi.SAVE_RECTS_SYMBOLS +
                                  _abi.PREVIEW_TILES_SYMBOLS)
    L = lib.load()
    for name, nargs in zip(SYMBOLS, (6, 6, 6, 10)):
        fn = getattr(L, name)  # AttributeError: declared but not exported
        assert fn.restype is C.c_int32 and len(fn.argtypes) == nargs, name
    assert '#include "jxl_hip_extra_rects.h"' in open(g.HEADER).read()
    assert lib.MAX_EC_RECTS == 4096 and lib.ABI_VERSION == 6
    for i, first in enumerate(("jxl_hip.h", "jxl_hip_extra_rects.h")):
        src = os.path.join(str(tmp_path), f"order{i}.c")
        with open(src, "w") as f:
            f.write(f'#include "{first}"\n#include "jxl_hip_extra_rects.h"\n#include "jxl_hip.h"\n#include <stddef.h>\n'
                    "jxlh_status (*begin)(jxlh_ctx*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) = jxlh_frame_begin_extra_channel;\n"
                    "jxlh_status (*rects)(jxlh_ctx*, const int32_t*, uint64_t, const jxlh_ec_rect*, uint32_t, uint32_t*) =\n"
                    "    jxlh_frame_set_extra_channel_rects;\n"
                    "jxlh_status (*rects_async)(jxlh_ctx*, const int32_t*, uint64_t, const jxlh_ec_rect*, uint32_t, uint32_t*) =\n"
                    "    jxlh_frame_set_extra_channel_rects_async;\n"
                    "jxlh_status (*changed)(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, const jxlh_rect*, uint32_t, jxlh_rect*,\n"
                    "                       uint32_t, uint32_t*) = jxlh_extra_channel_changed_rects;\n"
                    "_Static_assert(sizeof(jxlh_ec_rect) == 40 && offsetof(jxlh_ec_rect, offset) == 24 &&\n"
                    "               offsetof(jxlh_ec_rect, stride) == 32 && JXLH_MAX_EC_RECTS == 4096, \"jxlh_ec_rect\");\n"
                    "int main(void) { return 0; }\n")
        r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", src,
                            "-o", os.path.join(str(tmp_path), f"order{i}.o")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
    assert C.sizeof(lib.EcRect) == 40 == lib.EC_RECT_DTYPE.itemsize
    for name in ("ec", "x0", "y0", "w", "h", "offset", "stride"):
        assert getattr(lib.EcRect, name).offset == lib.EC_RECT_DTYPE.fields[name][1], name


def test_generators_are_current_and_name_the_header():
    import gen_py_binding
    import gen_rust_binding as g
    for tool in ("gen_py_binding.py", "gen_rust_binding.py"):
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--check"], check=True)
    assert open(gen_py_binding.OUT).read() == gen_py_binding.generate()
    rust = open(g.OUT_EXTRA_RECTS).read()
    assert rust == g.generate_extra_rects() and "pub mod extra_rects;" in open(g.OUT).read()
    for name in SYMBOLS:
        assert f"pub fn {name}(" in rust, name
    assert "pub struct jxlh_ec_rect" in rust and "pub offset: u64," in rust and "pub const JXLH_MAX_EC_RECTS: u32 = 4096;" in rust
    # the layers above name them too
    hpp = open(os.path.join(ROOT, "include", "jxl_hip.hpp")).read()
    pipe = open(os.path.join(ROOT, "include", "jxl_hip_pipeline.hpp")).read()
    safe = open(os.path.join(ROOT, "bindings", "rust", "jxl_hip", "src", "lib.rs")).read()
    for name in SYMBOLS[:3]:
        assert name + "(" in hpp, name
    assert "jxlh_extra_channel_changed_rects(" in pipe and "fn set_extra_channel_rects" in safe
    from jxl_rs_amd import lib
    for name in ("begin_extra_channel", "set_extra_channel_rects"):
        assert hasattr(lib.Context, name), name
    assert hasattr(lib, "extra_channel_changed_rects")


def test_changed_rects_cap_protocol_and_statuses():
    from jxl_rs_amd import lib
    INV = lib.ERR_INVALID_ARGUMENT
    L = lib.load()
    src = np.array([[0, 0, 1, 1], [30, 20, 3, 5], [9, 9, 0, 4]], dtype=np.uint32)
    want = [[0, 0, 6, 6], [56, 36, 9, 13], [0, 0, 0, 0]]   # (28..33) * 2 cut at 65; (18..25) * 2 cut at 49
    st, rects, n = lib.try_extra_channel_changed_rects(33, 25, 2, 65, 49, src)
    assert (st, n) == (lib.OK, 3) and rects.tolist() == want
    # the count alone; a cap that is too small sets *n and writes nothing; room to spare
    cnt = C.c_uint32(99)
    assert L.jxlh_extra_channel_changed_rects(33, 25, 2, 65, 49, src.ctypes.data, 3, None, 0, C.byref(cnt)) == INV and cnt.value == 3
    out = np.full((5, 4), 7, dtype=np.uint32)
    cnt = C.c_uint32(99)
    assert L.jxlh_extra_channel_changed_rects(33, 25, 2, 65, 49, src.ctypes.data, 3, out.ctypes.data, 2, C.byref(cnt)) == INV
    assert cnt.value == 3 and np.all(out == 7)
    assert L.jxlh_extra_channel_changed_rects(33, 25, 2, 65, 49, src.ctypes.data, 3, out.ctypes.data, 5, C.byref(cnt)) == lib.OK
    assert cnt.value == 3 and out[:3].tolist() == want and np.all(out[3:] == 7)
    assert L.jxlh_extra_channel_changed_rects(33, 25, 2, 65, 49, None, 0, None, 0, C.byref(cnt)) == lib.OK and cnt.value == 0
    # null pointers
    assert L.jxlh_extra_channel_changed_rects(33, 25, 2, 65, 49, src.ctypes.data, 3, out.ctypes.data, 5, None) == INV
    assert L.jxlh_extra_channel_changed_rects(33, 25, 2, 65, 49, None, 3, out.ctypes.data, 5, C.byref(cnt)) == INV
    assert L.jxlh_extra_channel_changed_rects(33, 25, 2, 65, 49, src.ctypes.data, 3, None, 5, C.byref(cnt)) == INV
    # sizes, factors, rects that leave the channel (the sums computed without wrapping)
    for args in ((0, 25, 2, 65, 49), (33, 0, 2, 65, 49), (33, 25, 2, 0, 49), (33, 25, 2, 65, 0), (33, 25, 0, 65, 49),
                 (33, 25, 3, 65, 49), (33, 25, 16, 65, 49)):
        assert lib.try_extra_channel_changed_rects(*args, src)[0] == INV, args
    for bad in ((33, 0, 1, 1), (0, 25, 1, 1), (31, 0, 3, 1), (0, 24, 1, 2), (0xffffffff, 0, 2, 1), (0, 0xffffffff, 1, 2),
                (1, 0, 0xffffffff, 1)):
        assert lib.try_extra_channel_changed_rects(33, 25, 2, 65, 49, [(0, 0, 1, 1), bad])[0] == INV, bad
    # factor 1: the rect itself, cut at the result
    assert lib.extra_channel_changed_rects(33, 25, 1, 33, 25, [(3, 4, 5, 6)]).tolist() == [[3, 4, 5, 6]]
    assert lib.extra_channel_changed_rects(33, 25, 1, 30, 20, [(28, 18, 5, 7), (31, 0, 2, 2)]).tolist() == [[28, 18, 2, 2], [0, 0, 0, 0]]
    with pytest.raises(lib.JxlHipError):
        lib.extra_channel_changed_rects(33, 25, 5, 33, 25, [(0, 0, 1, 1)])


def _rule_rects(w, h):
    """each corner, each edge, interior, 1 x 1 -- clipped to tiny channels"""
    rw, rh = min(3, w), min(2, h)
    cand = [(0, 0, rw, rh), (w - rw, 0, rw, rh), (0, h - rh, rw, rh), (w - rw, h - rh, rw, rh),          # corners
            (w // 2, 0, 1, rh), (w // 2, h - rh, 1, rh), (0, h // 2, rw, 1), (w - rw, h // 2, rw, 1),       # edges
            (w // 2, h // 2, 1, 1), (w // 3, h // 3, min(4, w - w // 3), min(3, h - h // 3)), (0, 0, 1, 1), (w - 1, h - 1, 1, 1)]
    return sorted(set(cand))


@pytest.mark.parametrize("up", [1, 2, 4, 8])
@pytest.mark.parametrize("size", [(33, 25), (7, 5), (1, 9), (9, 1)], ids=lambda s: "%dx%d" % s)
def test_changed_rects_rule_against_the_oracle(oracle, size, up):
    from jxl_rs_amd import lib
    w, h = size
    rng = np.random.default_rng(w * 100 + h * 10 + up)
    res_w, res_h = max(1, w * up - 1), max(1, h * up - 1)   # the result cuts one sample off the full size on each axis

    def finish(plane):
        f = oracle.modular_to_f32(plane, 12)
        return (oracle.upsample(up, f) if up > 1 else f)[:res_h, :res_w].copy()
    base = rng.integers(0, 1 << 12, size=(h, w)).astype(np.int32)
    before = finish(base)
    for x0, y0, rw, rh in _rule_rects(w, h):
        new = base.copy()
        new[y0:y0 + rh, x0:x0 + rw] = (base[y0:y0 + rh, x0:x0 + rw] + rng.integers(1, 4095, size=(rh, rw))) % 4096
        after = finish(new)
        (qx, qy, qw, qh), = lib.extra_channel_changed_rects(w, h, up, res_w, res_h, [(x0, y0, rw, rh)]).tolist()
        assert qx + qw <= res_w and qy + qh <= res_h
        outside = np.ones(before.shape, bool)
        outside[qy:qy + qh, qx:qx + qw] = False
        diff = before.view(np.uint32) != after.view(np.uint32)
        assert not np.any(diff & outside), (size, up, (x0, y0, rw, rh), (qx, qy, qw, qh), np.argwhere(diff & outside)[:4].tolist())
        # (a rect the result's crop cuts off entirely gives an empty rect, and changes nothing that is left)
        assert np.any(diff) == (qw * qh > 0), "the samples did change the channel"


def test_rects_call_statuses_that_need_no_device():
    from jxl_rs_amd import lib
    L = lib.load()
    INV = lib.ERR_INVALID_ARGUMENT
    block = np.zeros(16, np.int32)
    rect = np.zeros(1, dtype=lib.EC_RECT_DTYPE)
    rect[0] = (0, 0, 0, 2, 2, 0, 2)
    bad = C.c_uint32(99)
    for fn in (L.jxlh_frame_set_extra_channel_rects, L.jxlh_frame_set_extra_channel_rects_async):
        assert fn(None, block.ctypes.data, 16, rect.ctypes.data, 1, C.byref(bad)) == INV     # null context
        assert fn(None, block.ctypes.data, 16, None, 1, C.byref(bad)) == INV                 # ... and null rects
        assert fn(None, None, 0, None, 0, None) == INV
        assert bad.value == 99
    assert L.jxlh_frame_begin_extra_channel(None, 0, 4, 4, 8, 1) == INV
