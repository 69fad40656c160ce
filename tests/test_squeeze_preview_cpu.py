"""Progressive previews of a squeezed image, the host side (no GPU): jxlh_squeeze_preview_kinds -- the public face of
jxl_rs_amd/csrc/squeeze_preview_plan.h -- against the restatement of the reference's bookkeeping in
tests/squeeze_preview_ref.py; every refusal with its status; the bindings; and the planner header on its own through
tests/cpp/squeeze_preview_plan.cc, plain and under the host sanitizers."""
import os
import subprocess

import numpy as np
import pytest

from squeeze_preview_ref import explicit_steps, missing_flags, preview_kinds_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRESENT = 0x1000   # the host function only tests residual pointers for NULL


def default_steps(w, h):
    from jxl_rs_amd import synth
    return synth.default_squeeze_steps(w, h)


CHAINS = {
    "37x29": lambda: default_steps(37, 29),
    "64x64": lambda: default_steps(64, 64),
    "130x65": lambda: default_steps(130, 65),
    "1x40": lambda: default_steps(1, 40),
    "HHVV": lambda: explicit_steps(70, 50, [True, True, False, False]),
    "VHH": lambda: explicit_steps(33, 21, [False, True, True]),
    "allH": lambda: explicit_steps(200, 3, [True] * 5),
}


def levels_of(steps, missing, n_planes=1):
    return [(hz, ow, oh, [None if m else PRESENT] * n_planes, max(ow // 2 if hz else ow, 1))
            for (hz, ow, oh), m in zip(steps, missing)]


def check_against_ref(steps, base, missing, n_planes=1):
    from jxl_rs_amd import lib
    kinds, live = lib.squeeze_preview_kinds(levels_of(steps, missing, n_planes), base[0], base[1], n_planes=n_planes)
    want_kinds, _, want_live = preview_kinds_ref([hz for hz, _, _ in steps], missing_flags(steps, missing))
    assert list(kinds) == want_kinds, (steps, missing, list(kinds), want_kinds)
    assert [bool(v) for v in live] == want_live, (steps, missing, list(live), want_live)
    return list(kinds), [bool(v) for v in live]


@pytest.mark.parametrize("name", list(CHAINS))
def test_kinds_and_liveness_on_missing_suffixes(name):
    steps, base = CHAINS[name]()
    for k in range(0, 7):
        k = min(k, len(steps))
        check_against_ref(steps, base, [i >= len(steps) - k for i in range(len(steps))], n_planes=1 + k % 3)


@pytest.mark.parametrize("name", list(CHAINS))
def test_kinds_and_liveness_on_missing_sets_with_holes(name):
    steps, base = CHAINS[name]()
    rng = np.random.default_rng(len(name) * 1000 + len(steps))
    for _ in range(200):
        check_against_ref(steps, base, list(rng.random(len(steps)) < rng.choice([0.3, 0.5, 0.8])))


def test_known_answers():
    """the cases the rule is about, spelled out"""
    from jxl_rs_amd import lib
    R, S1, S2 = lib.PREVIEW_REGULAR, lib.PREVIEW_SMOOTH_1D, lib.PREVIEW_SMOOTH_2D
    steps, base = default_steps(64, 64)                 # V, H, V, H, V, H from 8 x 8 (squeeze.rs:71-105)
    assert [hz for hz, _, _ in steps] == [True, False] * 3 and base == (8, 8)
    n = len(steps)
    # five missing levels: 1-D, then 2-D four times; the final planes depend on every second level from the end
    kinds, live = check_against_ref(steps, base, [i >= 1 for i in range(n)])
    assert kinds == [R, S1, S2, S2, S2, S2] and live == [True, True, False, True, False, True]
    # four and three: the smooth 1-D level itself can be dead
    kinds, live = check_against_ref(steps, base, [i >= 2 for i in range(n)])
    assert kinds == [R, R, S1, S2, S2, S2] and live == [True, True, False, True, False, True]
    kinds, live = check_against_ref(steps, base, [i >= 3 for i in range(n)])
    assert kinds == [R, R, R, S1, S2, S2] and live == [True, True, True, True, False, True]
    # neighbours of one direction never pair up
    steps2, base2 = explicit_steps(70, 50, [True, True, False, False])
    kinds, live = check_against_ref(steps2, base2, [True] * 4)
    assert kinds == [S1, S1, S2, S1] and live == [True, False, True, True]
    # a hole: a present level behind a missing one is regular, and what it reads is live
    kinds, live = check_against_ref(steps, base, [False, True, True, False, True, True])
    assert kinds == [R, S1, S2, R, S1, S2] and live == [True, False, True, True, False, True]
    # a level without residual samples is regular whatever its pointers are
    steps3, base3 = default_steps(1, 40)
    assert all(not hz for hz, _, _ in steps3)
    steps4, base4 = explicit_steps(1, 9, [True, False])   # the horizontal level of a 1-wide channel has no residuals
    kinds, live = check_against_ref(steps4, base4, [True, True])
    assert kinds == [R, S1]


def test_refusals():
    from jxl_rs_amd import lib
    steps, base = default_steps(37, 29)
    n = len(steps)

    def status(levels, bw=base[0], bh=base[1], n_planes=1):
        try:
            lib.squeeze_preview_kinds(levels, bw, bh, n_planes=n_planes)
        except lib.JxlHipError as e:
            return e.status
        return lib.OK

    good = levels_of(steps, [False] * n, 3)
    assert status(good, n_planes=3) == lib.OK
    # some planes of a level named, others not
    for lost in ([0], [1], [2], [0, 2]):
        bad = [list(lv) for lv in good]
        bad[n - 1][3] = [None if p in lost else PRESENT for p in range(3)]
        assert status([tuple(lv) for lv in bad], n_planes=3) == lib.ERR_INVALID_ARGUMENT, lost
    # ... which one fewer plane does not see
    bad = [list(lv) for lv in good]
    bad[n - 1][3] = [PRESENT, PRESENT, None]
    assert status([tuple(lv) for lv in bad], n_planes=2) == lib.OK
    # geometry: a base that does not lead to the first level, a level that does not follow from the one before
    assert status(good, bw=base[0] + 1, n_planes=3) == lib.ERR_INVALID_ARGUMENT
    assert status(good, bh=0, n_planes=3) == lib.ERR_INVALID_ARGUMENT
    bad = list(good)
    hz, ow, oh, res, rs = bad[2]
    bad[2] = (hz, ow + 2, oh + 2, res, rs)
    assert status(bad, n_planes=3) == lib.ERR_INVALID_ARGUMENT
    # a present level's residual stride below its width; a missing level's stride is not looked at
    hz, ow, oh, res, rs = good[n - 1]
    assert status(good[:-1] + [(hz, ow, oh, res, 1)], n_planes=3) == lib.ERR_INVALID_ARGUMENT
    assert status(good[:-1] + [(hz, ow, oh, [None] * 3, 1)], n_planes=3) == lib.OK
    # plane and level counts
    assert status(good, n_planes=0) == lib.ERR_INVALID_ARGUMENT
    assert status(good, n_planes=4) == lib.ERR_INVALID_ARGUMENT
    assert status([], n_planes=1) == lib.ERR_INVALID_ARGUMENT
    L = lib._lib()
    assert L.jxlh_squeeze_preview_kinds(1, n, None, base[0], base[1], None, None) == lib.ERR_INVALID_ARGUMENT
    arr = lib._squeeze_levels(good, 3)
    assert L.jxlh_squeeze_preview_kinds(3, n, arr, base[0], base[1], None, None) == lib.ERR_INVALID_ARGUMENT   # no `kinds`
    kinds = np.full(n, 9, np.uint8)
    assert L.jxlh_squeeze_preview_kinds(3, n, arr, base[0], base[1], kinds.ctypes.data, None) == lib.OK       # `live` may be NULL
    assert (kinds == lib.PREVIEW_REGULAR).all()


def test_bindings_name_the_new_entry_points(tmp_path):
    """the entry points sit in include/jxl_hip_preview.h, which jxl_hip.h includes: the set jxl_hip.h itself declares is
    the one recorded for ABI version 6 and stays as it is; both generators read the new header too"""
    import ctypes as C
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_py_binding
    import gen_rust_binding
    from jxl_rs_amd import lib, _abi
    assert (lib.PREVIEW_REGULAR, lib.PREVIEW_SMOOTH_1D, lib.PREVIEW_SMOOTH_2D) == (0, 1, 2)
    assert lib.ABI_VERSION == 6
    L = lib._lib()
    assert _abi.PREVIEW_SYMBOLS == ["jxlh_squeeze_preview_kinds", "jxlh_unsqueeze_chain_preview"]
    assert not set(_abi.PREVIEW_SYMBOLS) & set(_abi.ABI_SYMBOLS + _abi.DEV_SYMBOLS)
    for name, nargs in (("jxlh_squeeze_preview_kinds", 7), ("jxlh_unsqueeze_chain_preview", 13)):
        fn = getattr(L, name)
        assert fn.restype is C.c_int32 and len(fn.argtypes) == nargs, name
    assert L.jxlh_unsqueeze_chain_preview.argtypes[-1] is C.c_uint32      # flags
    assert hasattr(lib.Context, "unsqueeze_chain_preview")
    from jxl_rs_amd.modular import ModularChain
    assert hasattr(ModularChain, "preview")
    # the committed bindings are what the generators produce now
    assert open(gen_py_binding.OUT).read() == gen_py_binding.generate()
    assert open(gen_rust_binding.OUT_PREVIEW).read() == gen_rust_binding.generate_preview()
    header = open(os.path.join(ROOT, "include", "jxl_hip_preview.h")).read()
    main_header = open(os.path.join(ROOT, "include", "jxl_hip.h")).read()
    rust = open(gen_rust_binding.OUT_PREVIEW).read()
    hpp = open(os.path.join(ROOT, "include", "jxl_hip.hpp")).read()
    assert '#include "jxl_hip_preview.h"' in main_header and "pub mod preview;" in open(gen_rust_binding.OUT).read()
    for name in ("jxlh_squeeze_preview_kinds", "jxlh_unsqueeze_chain_preview"):
        assert f"jxlh_status {name}(" in header and f"pub fn {name}(" in rust and name + "(" in hpp, name
    assert "flags: u32) -> jxlh_status;" in rust[rust.index("pub fn jxlh_unsqueeze_chain_preview("):][:600]
    for const in ("JXLH_PREVIEW_REGULAR", "JXLH_PREVIEW_SMOOTH_1D", "JXLH_PREVIEW_SMOOTH_2D"):
        assert const in header and f"pub const {const}: u32" in rust
    assert "#define JXLH_ABI_VERSION 6" in main_header
    # a C caller gets the whole interface from either header, in either order
    for i, first in enumerate(("jxl_hip.h", "jxl_hip_preview.h")):
        src = os.path.join(str(tmp_path), f"order{i}.c")
        with open(src, "w") as f:
            f.write(f'#include "{first}"\n#include "jxl_hip_preview.h"\n#include "jxl_hip.h"\n'
                    "jxlh_status (*kinds)(int32_t, int32_t, const jxlh_squeeze_level*, uint32_t, uint32_t, uint8_t*, uint8_t*) =\n"
                    "    jxlh_squeeze_preview_kinds;\nint flag = JXLH_PREVIEW_SMOOTH_2D | JXLH_SMOOTH_CVT_NEAREST_EVEN;\n")
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src,
                            "-o", src + ".o"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]


def _build_plan_program(tmp_path, name, extra):
    exe = os.path.join(str(tmp_path), name)
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "squeeze_preview_plan.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_planner_header_alone(tmp_path):
    """the header needs nothing but include/jxl_hip.h: no library, no device"""
    exe = _build_plan_program(tmp_path, "squeeze_preview_plan", ["-O2"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "squeeze preview plans: ok (100000 chains)" in r.stdout, (r.stdout + r.stderr)[-2000:]


def test_planner_header_alone_under_host_sanitizers(tmp_path):
    """the same stand-alone program, host compile with AddressSanitizer and UBSan: nothing is loaded into Python"""
    exe = _build_plan_program(tmp_path, "squeeze_preview_plan_san",
                              ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "squeeze preview plans: ok (100000 chains)" in r.stdout, (r.stdout + r.stderr)[-2000:]
