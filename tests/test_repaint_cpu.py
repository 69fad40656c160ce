"""include/jxl_hip_repaint.h without a device: the header compiles as C in either include order, both symbols are
exported and bound and both binding generators are current; the cap protocol and the statuses of
jxlh_repaint_changed_rects; its equality with jxlh_changed_rects wherever that call answers; and its soundness, tightness
and non-vacuity on the oracle: after the coefficients (samples) of the listed cells are replaced, no pixel of the oracle's
upsampled frame outside the returned rects differs, a reach one coded pixel smaller does leave one outside, and inside
every listed cell at least 5 % of the Y pixels do differ.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import repaint_ref as rr
from helpers import run_oracle_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SYMBOLS = ["jxlh_frame_repaint_groups", "jxlh_repaint_changed_rects"]
# (gab, epf_iters, the stage list's reach: Gaborish 1, EPF0 3, EPF1 2, EPF2 1)
STAGES = {"none": (False, 0, 0), "gab": (True, 0, 1), "gab_epf2": (True, 2, 4), "epf3": (False, 3, 6)}
SIZES = [(300, 600), (264, 520)]  # 2 x 3 groups; the one-block last column
LISTS = [[0], [3], [1, 4]]        # a corner group, an interior-edge group, two diagonal groups


def test_header_compiles_as_c_and_its_symbols_are_exported(tmp_path):
    import gen_rust_binding as g
    from jxl_rs_amd import _abi, lib
    declared = [f[0] for f in g.parse_header(open(g.REPAINT_HEADER).read())[4]]
    assert declared == SYMBOLS == _abi.REPAINT_SYMBOLS
    assert not set(SYMBOLS) & set(_abi.ABI_SYMBOLS + _abi.DEV_SYMBOLS + _abi.PREVIEW_SYMBOLS + _abi.SAVE_RECTS_SYMBOLS +
                                  _abi.PREVIEW_TILES_SYMBOLS + _abi.EXTRA_RECTS_SYMBOLS)
    L = lib.load()
    for name, nargs in zip(SYMBOLS, (3, 6)):
        fn = getattr(L, name)  # AttributeError: declared but not exported
        assert fn.restype is C.c_int32 and len(fn.argtypes) == nargs, name
    assert '#include "jxl_hip_repaint.h"' in open(g.HEADER).read() and lib.ABI_VERSION == 6
    for i, first in enumerate(("jxl_hip.h", "jxl_hip_repaint.h")):
        src = os.path.join(str(tmp_path), f"order{i}.c")
        with open(src, "w") as f:
            f.write(f'#include "{first}"\n#include "jxl_hip_repaint.h"\n#include "jxl_hip.h"\n'
                    "jxlh_status (*repaint)(jxlh_ctx*, const uint32_t*, uint32_t) = jxlh_frame_repaint_groups;\n"
                    "jxlh_status (*changed)(const jxlh_frame_params*, const uint32_t*, uint32_t, jxlh_rect*, uint32_t, uint32_t*) =\n"
                    "    jxlh_repaint_changed_rects;\n"
                    "int main(void) { return 0; }\n")
        r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", src,
                            "-o", os.path.join(str(tmp_path), f"order{i}.o")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]


def test_generators_are_current_and_the_layers_above_name_the_calls():
    import gen_py_binding
    import gen_rust_binding as g
    for tool in ("gen_py_binding.py", "gen_rust_binding.py"):
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--check"], check=True)
    assert open(gen_py_binding.OUT).read() == gen_py_binding.generate()
    rust = open(g.OUT_REPAINT).read()
    assert rust == g.generate_repaint() and "pub mod repaint;" in open(g.OUT).read()
    for name in SYMBOLS:
        assert f"pub fn {name}(" in rust, name
    hpp = open(os.path.join(ROOT, "include", "jxl_hip.hpp")).read()
    pipe = open(os.path.join(ROOT, "include", "jxl_hip_pipeline.hpp")).read()
    for name in SYMBOLS:
        assert name + "(" in hpp, name
    assert "repaint_changed_rects" in pipe and "repaint_groups" in pipe
    from jxl_rs_amd import lib
    for name in ("repaint_groups", "try_repaint_groups", "repaint_changed_rects"):
        assert hasattr(lib.Context, name), name
    assert callable(lib.repaint_changed_rects) and callable(lib.try_repaint_changed_rects)


def frame_params(w, h, gab=False, epf=0, n=1, modular=False, cut=None, shifts=None):
    from jxl_rs_amd import lib
    p = lib.FrameParams()
    assert lib.load().jxlh_default_frame_params(p, w, h) == lib.OK
    p.gab, p.epf_iters, p.upsampling = int(gab), int(epf), n
    if modular:
        p.flags |= lib.FRAME_MODULAR
    if cut:
        p.xsize_upsampled, p.ysize_upsampled = cut
    if shifts:
        for c in range(3):
            p.hshift[c], p.vshift[c] = shifts[0][c], shifts[1][c]
    return p


def rule_mask(w, h, n, reach_x, reach_y, ids, cut=None):
    """the rule, per pixel of the result: every listed cell, clipped to the frame, widened by the reach (the stage
    list's, plus the upsampling window's 2 coded pixels when n > 1), clipped, scaled by n, clipped to the result"""
    ow, oh = rr.result_size(w, h, n, cut)
    m = np.zeros((oh, ow), dtype=bool)
    for g in ids:
        x0, y0, x1, y1 = rr.cell(w, h, int(g))
        m[max(0, y0 - reach_y) * n:min(h, y1 + reach_y) * n, max(0, x0 - reach_x) * n:min(w, x1 + reach_x) * n] = True
    return m


def rect_mask(rects, ow, oh):
    cover = np.zeros((oh, ow), dtype=np.int32)
    for x0, y0, rw, rh in np.asarray(rects, dtype=np.int64).reshape(-1, 4):
        assert rw > 0 and rh > 0 and x0 + rw <= ow and y0 + rh <= oh, (x0, y0, rw, rh, ow, oh)
        cover[y0:y0 + rh, x0:x0 + rw] += 1
    return cover


def test_cap_protocol_and_statuses():
    from jxl_rs_amd import lib
    L = lib.load()
    p = frame_params(300, 600, True, 2, 2)
    ids = np.array([0, 3, 5], dtype=np.uint32)
    n = C.c_uint32(77)
    out = np.zeros((8, 4), dtype=np.uint32)

    def call(pp, i, count, o, cap, nn):
        return L.jxlh_repaint_changed_rects(pp, None if i is None else i.ctypes.data, count, None if o is None else o.ctypes.data,
                                            cap, nn)
    # the count comes back with cap 0; a cap that is too small is an argument error that still names the count
    assert call(p, ids, 3, None, 0, C.byref(n)) == lib.ERR_INVALID_ARGUMENT and n.value == 3
    assert call(p, ids, 3, out, 2, C.byref(n)) == lib.ERR_INVALID_ARGUMENT and n.value == 3 and not out.any()
    assert call(p, ids, 3, out, 3, C.byref(n)) == lib.OK and n.value == 3
    assert call(p, ids, 0, None, 0, C.byref(n)) == lib.OK and n.value == 0
    # null pointers
    for bad in ((None, ids, 3, out, 8, C.byref(n)), (p, None, 3, out, 8, C.byref(n)), (p, ids, 3, None, 8, C.byref(n)),
                (p, ids, 3, out, 8, None)):
        assert call(*bad) == lib.ERR_INVALID_ARGUMENT
    # parameters jxlh_frame_begin refuses, an id beyond the grid, a factor that is none
    for change in (dict(abi_version=5), dict(xsize=0), dict(ysize=(1 << 20) + 1), dict(epf_iters=4), dict(upsampling=3)):
        q = frame_params(300, 600, True, 2, 2)
        for k, v in change.items():
            setattr(q, k, v)
        assert call(q, ids, 3, out, 8, C.byref(n)) == lib.ERR_INVALID_ARGUMENT, change
    q = frame_params(300, 600, True, 2, 2)
    q.hshift[1] = 2
    assert call(q, ids, 3, out, 8, C.byref(n)) == lib.ERR_INVALID_ARGUMENT
    assert lib.try_repaint_changed_rects(p, [6])[0] == lib.ERR_INVALID_ARGUMENT
    assert lib.try_repaint_changed_rects(p, [5, 5, 0])[0] == lib.OK
    # never unsupported: every kind of frame jxlh_changed_rects refuses is answered
    for q in (frame_params(300, 600, n=8), frame_params(300, 600, modular=True), frame_params(300, 600, n=4, modular=True)):
        assert lib.try_changed_rects(q, [0])[0] == lib.ERR_UNSUPPORTED
        assert lib.try_repaint_changed_rects(q, [0])[0] == lib.OK


@pytest.mark.parametrize("w,h", [(600, 520), (264, 300), (8, 600), (256, 256)])
def test_equal_to_changed_rects_wherever_that_answers(w, h):
    from jxl_rs_amd import lib
    rng = np.random.default_rng(w + h)
    ng = ((w + 255) // 256) * ((h + 255) // 256)
    s420 = ((1, 0, 1), (1, 0, 1))
    for gab, epf, _ in STAGES.values():
        for shifts in (None, s420):
            p = frame_params(w, h, gab, epf, 1, shifts=shifts)
            for _ in range(6):
                ids = rng.integers(0, ng, size=int(rng.integers(1, 2 * ng + 1)))
                st, want, _ = lib.try_changed_rects(p, ids)
                assert st == lib.OK
                assert np.array_equal(lib.repaint_changed_rects(p, ids), want), (gab, epf, shifts, ids)
            p.upsampling = 0  # "not upsampled" as well
            assert np.array_equal(lib.repaint_changed_rects(p, [0, ng - 1]), lib.changed_rects(p, [0, ng - 1]))


@pytest.mark.parametrize("w,h", SIZES + [(8, 600), (700, 300)])
def test_rects_are_the_rule_and_disjoint(w, h):
    """against the per-pixel statement of the rule: exactly the widened, scaled cells, every pixel in one rect only"""
    from jxl_rs_amd import lib
    rng = np.random.default_rng(w * 3 + h)
    ng = ((w + 255) // 256) * ((h + 255) // 256)
    for n in (1, 2, 4):
        for modular in (False, True):
            if n == 1 and not modular:
                continue
            for gab, epf, reach in STAGES.values():
                for shifts in (None, ((1, 0, 1), (0, 0, 0))):
                    cut = (w * n - (n - 1), h * n - 1) if n > 1 and gab else None
                    p = frame_params(w, h, gab, epf, n, modular, cut, shifts)
                    ids = rng.integers(0, ng, size=int(rng.integers(1, ng + 2)))
                    rects = lib.repaint_changed_rects(p, ids)
                    ow, oh = rr.result_size(w, h, n, cut)
                    cover = rect_mask(rects, ow, oh)
                    border = 2 if n > 1 else 0
                    want = rule_mask(w, h, n, reach + border + (1 if shifts else 0), reach + border, ids, cut)
                    assert cover.max() <= 1, (n, modular, gab, epf, ids)
                    assert np.array_equal(cover > 0, want), (n, modular, gab, epf, shifts, ids)


# ---------------------------------------------------------------- on the oracle
_CODED = {}


def coded_frames(oracle, w, h, stage):
    """(A's coded-size planes, {list: the planes with the list's groups from another seed})"""
    from jxl_rs_amd import synth
    key = (w, h, stage)
    if key not in _CODED:
        gab, epf, _ = STAGES[stage]
        a = synth.make_vardct(w, h, mix=synth.MIX_D1, seed=61, epf_iters=epf, gab=gab)
        b = synth.make_vardct(w, h, mix=synth.MIX_D1, seed=62, epf_iters=epf, gab=gab)
        _CODED[key] = (run_oracle_frame(oracle, a)[0],
                       {tuple(ids): run_oracle_frame(oracle, rr.with_groups_from(a, b, ids))[0] for ids in LISTS})
    return _CODED[key]


def differing(before, after):
    d = np.zeros(before[0].shape, dtype=bool)
    for x, y in zip(before, after):
        d |= x.view(np.uint32) != y.view(np.uint32)
    return d


def check_sound(oracle, before, after, p, w, h, n, ids, cut, what):
    """non-vacuity first, then soundness; returns the map of differing pixels"""
    from jxl_rs_amd import lib
    up_b, up_a = rr.finish(oracle, before, n, False, cut), rr.finish(oracle, after, n, False, cut)
    ow, oh = rr.result_size(w, h, n, cut)
    y_diff = up_b[1].view(np.uint32) != up_a[1].view(np.uint32)
    for g in ids:
        x0, y0, x1, y1 = rr.cell(w, h, g)
        inside = y_diff[y0 * n:min(oh, y1 * n), x0 * n:min(ow, x1 * n)]
        assert inside.mean() >= 0.05, (what, g, float(inside.mean()))
    diff = differing(up_b, up_a)
    rects = lib.repaint_changed_rects(p, ids)
    out = rr.outside(rects, ow, oh)
    assert not np.any(diff & out), (what, ids, np.argwhere(diff & out)[:4].tolist())
    return diff


@pytest.mark.parametrize("stage", list(STAGES))
@pytest.mark.parametrize("w,h", SIZES, ids=["300x600", "264x520"])
def test_sound_on_the_oracle(oracle, w, h, stage):
    gab, epf, _ = STAGES[stage]
    before, afters = coded_frames(oracle, w, h, stage)
    cases = [(2, None), (4, None), (8, None)] if (w, h) == SIZES[0] else [(2, None), (4, (w * 4 - 3, h * 4 - 1))]
    for n, cut in cases:
        for ids in LISTS if n == 2 else LISTS[2:]:
            check_sound(oracle, before, afters[tuple(ids)], frame_params(w, h, gab, epf, n, cut=cut), w, h, n, ids, cut,
                        f"{stage} x{n} {cut}")


@pytest.mark.parametrize("n", [2, 4, 8])
def test_tight_on_the_oracle(oracle, n):
    """the same rule with a reach one coded pixel smaller leaves a differing pixel outside"""
    w, h = SIZES[0]
    for stage in ("none", "gab"):
        gab, epf, reach = STAGES[stage]
        before, afters = coded_frames(oracle, w, h, stage)
        ids = LISTS[1]
        diff = check_sound(oracle, before, afters[tuple(ids)], frame_params(w, h, gab, epf, n), w, h, n, ids, None, stage)
        smaller = rule_mask(w, h, n, reach + 1, reach + 1, ids)
        assert np.any(diff & ~smaller), (stage, n)


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("gab,epf,reach", [(0, 0, 0), (1, 2, 4)], ids=["unfiltered", "gab_epf2"])
def test_modular_sound_on_the_oracle(oracle, gab, epf, reach, n):
    w, h = SIZES[0]
    chans, other = rr.modular_samples(5, w, h), rr.modular_samples(6, w, h)
    p = frame_params(w, h, gab, epf, n, modular=True)

    def coded(c):
        return rr.modular_filters(oracle, [oracle.modular_to_f32(x, 8, 0) for x in c], gab, epf)
    before = coded(chans)
    for ids in LISTS:
        cur = [c.copy() for c in chans]
        for g in ids:
            x0, y0, x1, y1 = rr.cell(w, h, g)
            for c in range(3):
                cur[c][y0:y1, x0:x1] = other[c][y0:y1, x0:x1] + 64
        diff = check_sound(oracle, before, coded(cur), p, w, h, n, ids, None, f"modular gab{gab} epf{epf} x{n}")
        if ids == LISTS[1]:  # tight here as well
            border = 2 if n > 1 else 0
            if reach + border > 0:
                assert np.any(diff & ~rule_mask(w, h, n, reach + border - 1, reach + border - 1, ids))
