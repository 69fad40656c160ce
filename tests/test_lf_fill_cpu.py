"""Groups whose HF has not arrived, without a device: the expected-image builder (tests/lf_fill_ref.py) against a
line-by-line emulation of the reference's upsample_lf_group and against oracle.vardct_frame, and the new entry point in
every layer (header, Python binding, generated Rust, C++ wrappers)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from helpers import bit_equal, diff_report, oracle_params_from, run_oracle_frame
from lf_fill_ref import emulate_upsample_lf_group, expected_planes, group_rect, lf_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "jxlh_frame_set_groups_lf_only"


def make(w, h, **kw):
    from jxl_rs_amd import synth
    return synth.make_vardct(w, h, mix=synth.MIX_D1, seed=5, **kw)


def crop_of_whole_image(o, wl, lf, g, weights8=None):
    y0, y1, x0, x1 = group_rect(wl, g)
    return [o.upsample(8, a, weights8)[y0:y1, x0:x1] for a in lf]


# the reference's two scratch-row geometries (jxl_hip.h, "GROUPS WITHOUT HF"): (a) a frame one group wide, (b) the group
# column left of a one-block-wide last column (xblocks % 32 == 1)
def degenerate(wl, g):
    gx = g % wl.xgroups
    a = wl.xgroups == 1
    b = wl.xblocks % 32 == 1 and gx == wl.xgroups - 2
    return a or b


@pytest.mark.parametrize("size", [(300, 264), (520, 300), (200, 300)])
def test_the_contract_is_the_reference_function_except_in_its_two_scratch_row_geometries(oracle, size):
    """300 x 264 (38 x 33 blocks): every group equal.  520 x 300 (65 x 38): geometry (b) in group column 1.
    200 x 300 (25 x 38): geometry (a) in both groups.  The degenerate groups must DIFFER: the deviation stays pinned."""
    wl = make(*size)
    p = oracle_params_from(oracle, wl)
    lf = lf_image(oracle, wl, p)
    seen = {True: 0, False: 0}
    for g in range(wl.xgroups * wl.ygroups):
        ref = emulate_upsample_lf_group(oracle, lf, g, wl.xgroups)
        want = crop_of_whole_image(oracle, wl, lf, g)
        same = all(bit_equal(r, w) for r, w in zip(ref, want))
        assert same == (not degenerate(wl, g)), (size, g, [diff_report(r, w) for r, w in zip(ref, want)])
        seen[same] += 1
    assert seen[True] == {(300, 264): 4, (520, 300): 4, (200, 300): 0}[size]
    assert seen[False] == {(300, 264): 0, (520, 300): 2, (200, 300): 2}[size]


def test_custom_weights_reach_the_emulation_and_the_builder(oracle):
    wl = make(300, 264)
    p = oracle_params_from(oracle, wl)
    lf = lf_image(oracle, wl, p)
    w8 = np.random.default_rng(3).uniform(-0.05, 0.1, 210).astype(np.float32)
    ref = emulate_upsample_lf_group(oracle, lf, 3, wl.xgroups, w8)
    want = crop_of_whole_image(oracle, wl, lf, 3, w8)
    assert all(bit_equal(r, w) for r, w in zip(ref, want))
    assert not bit_equal(want[1], crop_of_whole_image(oracle, wl, lf, 3)[1])


@pytest.mark.parametrize("epf", [0, 2, 3])
def test_the_builder_with_no_group_marked_is_the_oracle_frame(oracle, epf):
    wl = make(300, 264, epf_iters=epf)
    want, _ = run_oracle_frame(oracle, wl)
    got = expected_planes(oracle, wl, [])
    for c in range(3):
        assert bit_equal(got[c], want[c]), (epf, c, diff_report(got[c], want[c]))


def test_marking_a_group_changes_the_frame_and_ignores_its_coefficients(oracle):
    wl = make(300, 264)
    plain = expected_planes(oracle, wl, [])
    one = expected_planes(oracle, wl, [1])
    changed = sum(int(np.count_nonzero(a.view(np.uint32) != b.view(np.uint32))) for a, b in zip(plain, one))
    assert changed > 5000, changed
    junk = wl.coeffs.copy()
    junk[1] = 12345
    again = expected_planes(oracle, wl, [1], coeffs=junk)
    assert all(bit_equal(a, b) for a, b in zip(one, again))


# ---------------------------------------------------------------- every layer carries the symbol
def test_header_binding_and_generated_rust_carry_the_symbol():
    from jxl_rs_amd import lib
    L = lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jxl_hip.h")).read(), flags=re.S)
    m = re.search(r"jxlh_status\s+" + NAME + r"\s*\(([^)]*)\)", src)
    assert m and [q.strip() for q in m.group(1).split(",")] == ["jxlh_ctx* ctx", "const uint32_t* group_ids", "uint32_t count"]
    assert re.search(r"#define\s+JXLH_ABI_VERSION\s+6\b", src) and L.jxlh_abi_version() == 6  # additions only
    assert hasattr(L, NAME) and NAME in lib.ABI_SYMBOLS
    assert list(getattr(L, NAME).argtypes) == [C.c_void_p, C.c_void_p, C.c_uint32]
    assert callable(lib.Context.set_groups_lf_only) and callable(lib.Context.try_set_groups_lf_only)
    assert getattr(L, NAME)(None, None, 0) == lib.ERR_INVALID_ARGUMENT  # refused before any device is touched
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "jxl_hip_sys", "src", "lib.rs")).read()
    assert "pub fn " + NAME + "(ctx: *mut jxlh_ctx, group_ids: *const u32, count: u32) -> jxlh_status;" in sys_rs
    safe_rs = open(os.path.join(ROOT, "bindings", "rust", "jxl_hip", "src", "lib.rs")).read()
    assert re.search(r"pub fn upsample_lf_group\(&self, group: u32\)", safe_rs) and "sys::" + NAME in safe_rs


def test_the_header_states_the_rules_and_what_is_out_of_scope():
    src = open(os.path.join(ROOT, "include", "jxl_hip.h")).read()
    doc = src[src.index("GROUPS WITHOUT HF"):src.index("jxlh_status " + NAME)]
    for needle in ("jxlh_frame_begin clears them", "clears that group's", "last call wins", "never read",
                   "JXLH_FRAME_STRIP", "chroma-subsampled", "comm_nranks > 1", "(a)", "(b)", "xblocks % 32 == 1",
                   "JXLH_ERR_BAD_STATE", "JXLH_ERR_UNSUPPORTED", "JXLH_ERR_INVALID_ARGUMENT", "count == 0"):
        assert needle in doc, needle


def test_the_cpp_wrappers_expose_it():
    hpp = open(os.path.join(ROOT, "include", "jxl_hip.hpp")).read()
    assert re.search(r"void upsample_lf_groups\(const uint32_t\* groups, uint32_t n\)", hpp) and NAME in hpp
    pipe = open(os.path.join(ROOT, "include", "jxl_hip_pipeline.hpp")).read()
    m = re.search(r"void set_lf_only_group\(uint32_t group_id\)\s*\{(.*?)\n  \}", pipe, flags=re.S)
    assert m and "upsample_lf_groups" in m.group(1) and "rerender_" in m.group(1)
    # beside set_buffer_for_group / mark_group_to_rerender, in the same class
    cls = pipe[pipe.index("class GpuRenderPipeline :"):pipe.index("class GpuModularFramePipeline :")]
    assert "set_lf_only_group" in cls and "set_buffer_for_group" in cls and "mark_group_to_rerender" in cls
