"""Group-local squeeze without a GPU: jxlh_modular_local_lower_squeeze and jxlh_modular_local_default_squeeze (pure host
code) against the restatement of squeeze.rs / meta_apply.rs (tests/modular_local_squeeze_ref.py), every refusal with its
status and first_bad, the unchanged ABI version and symbol lists, the bindings, the stand-alone lowering program (plain
and under sanitizers), and the proof on the oracle that the plane the GPU tests use reaches every tendency regime."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import modular_local_general_ref as gr
import modular_local_ref as mr
import modular_local_squeeze_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["jxlh_modular_local_default_squeeze", "jxlh_modular_local_lower_squeeze", "jxlh_modular_local_transforms_squeeze",
         "jxlh_frame_set_modular_groups_squeeze", "jxlh_frame_set_modular_groups_squeeze_async"]
# the lists in front of a squeeze: an RCT; a palette (its meta channel at position 0 is skipped by the default squeeze);
# both; a predicted palette
FRONTS = {
    "rct": (3, [mr.rct(0, 17)]),
    "palette_0_3": (3, [mr.palette(0, 3, mr.small_palette(3))]),
    "palette_2_1": (3, [mr.palette(2, 1, mr.small_palette(1))]),
    "rct_palette_1_1": (3, [mr.rct(0, 40), mr.palette(1, 1, mr.small_palette(1))]),
    "delta_palette_rct": (4, [gr.delta_palette(np.random.default_rng(3), 3, 1, 5), mr.rct(1, 10)]),
}


def _lib_steps(steps):
    from jxl_rs_amd import lib
    return [lib.local_rct(s["begin_c"], s["rct_type"]) if s["kind"] == mr.RCT else
            lib.local_palette(s["begin_c"], s["num_c"], s["table"], s["num_deltas"], s["predictor"]) for s in steps]


def _spec(n_channels, steps, squeeze, w, h, **over):
    shapes = sr.coded_shapes(n_channels, steps, squeeze, w, h)
    sp = {"x0": 0, "y0": 0, "w": w, "h": h, "n_channels": n_channels, "steps": _lib_steps(steps), "squeeze": squeeze,
          "coded": [np.zeros(s, np.int32) for s in shapes]}
    sp.update(over)
    return sp


def _check_program(p, n_channels, steps, squeeze, w, h):
    """p: a LocalSqueezeProgram"""
    (g_coded, g_slots, g_ops, g_phases), n_coded, chains = sr.expected_program(n_channels, steps, squeeze, w, h)
    assert p.n_coded == n_coded
    assert p.general.n_coded == g_coded and list(p.general.coded_slot)[:g_coded] == g_slots
    assert p.general.n_phases == g_phases and p.general.n_ops == len(g_ops)
    for got, want in zip(list(p.general.ops), g_ops):
        assert (got.kind, got.phase, got.num_colors, got.num_deltas, got.predictor) == \
            (want["kind"], want["phase"], want["num_colors"], want["num_deltas"], want["predictor"])
        assert list(got.out_slot)[:len(want["writes"])] == want["writes"] and got.in_slot[0] == want["reads"][0]
    for k, want in enumerate(chains):
        c = p.chains[k]
        assert (c.base, c.base_w, c.base_h, c.n_levels) == (want["base"], want["base_w"], want["base_h"], len(want["levels"])), (k, want)
        got = [(lv.horizontal, lv.out_w, lv.out_h, lv.res) for lv in list(c.levels)[:c.n_levels]]
        assert got == want["levels"], (k, got, want["levels"])


def _lower(specs, **kw):
    from jxl_rs_amd import lib
    arena, batch = lib.pack_local_squeeze_groups(specs)
    st, progs, bad = lib.modular_local_lower_squeeze(batch, 8, arena.size, wp=[gr.WP_DEFAULT] * len(specs), n=len(specs), **kw)
    return st, progs, bad, arena, batch


@pytest.mark.parametrize("n_channels", [1, 2, 3, 4])
@pytest.mark.parametrize("rect", sr.RECTS, ids=[f"{w}x{h}" for w, h in sr.RECTS])
def test_default_squeeze_lowering_agrees_with_the_restatement(rect, n_channels):
    from jxl_rs_amd import lib
    w, h = rect
    st, progs, bad, _, _ = _lower([_spec(n_channels, [], [], w, h)])
    assert st == lib.OK and bad is None
    _check_program(progs[0], n_channels, [], [], w, h)
    # ... and the public face of default_squeeze
    channels = [{"meta": False, "w": w, "h": h}] * n_channels
    assert lib.default_squeeze([(w, h)] * n_channels) == sr.default_squeeze(channels)
    assert lib.default_squeeze([(w, h)] * n_channels, n_meta=2) == sr.default_squeeze([{"meta": True, "w": 0, "h": 0}] * 2 + channels)


def test_what_the_default_lists_are():
    """the restatement itself where the issue names the outcome"""
    one = [{"meta": False, "w": 8, "h": 8}]
    assert sr.default_squeeze(one) == [] and sr.default_squeeze([{"meta": False, "w": 1, "h": 1}] * 3) == []
    # 8 x 8 with three equal channels: the preview branch alone
    assert sr.default_squeeze(one * 3) == [sr.params(1, 0, 1, 2), sr.params(0, 0, 1, 2)]
    _, _, chains = sr.expected_program(3, [], [], 1024, 1024)
    assert [len(c["levels"]) for c in chains] == [14, 16, 16]
    _, n_coded, chains = sr.expected_program(1, [], [], 1, 300)
    assert n_coded == 7 and all(lv[0] == 0 for lv in chains[0]["levels"])
    shapes = sr.coded_shapes(3, [], [], 300, 1)  # the preview's vertical step does not fire (h == 1); residuals of zero height: none
    assert all(s[0] == 1 for s in shapes)
    assert (1, 0) in sr.coded_shapes(3, [], [sr.params(1, 1, 0, 3)], 1, 1)  # (h, w): an explicit squeeze of a 1-sample axis leaves a zero side


@pytest.mark.parametrize("name", list(sr.EXPLICIT))
@pytest.mark.parametrize("rect", [(9, 9), (17, 130), (1, 5), (256, 256)], ids=lambda r: f"{r[0]}x{r[1]}")
def test_explicit_lists(name, rect):
    from jxl_rs_amd import lib
    n_channels, squeeze = sr.EXPLICIT[name]
    w, h = rect
    st, progs, bad, _, _ = _lower([_spec(n_channels, [], squeeze, w, h)])
    assert st == lib.OK and bad is None
    _check_program(progs[0], n_channels, [], squeeze, w, h)


@pytest.mark.parametrize("name", list(FRONTS))
def test_steps_in_front(name):
    """default and explicit squeezes behind an RCT / palettes: begin_c counts the meta channels, which the default list
    skips; the general program in front is the _general lowering's"""
    from jxl_rs_amd import lib
    n_channels, steps = FRONTS[name]
    n_meta = sum(s["kind"] == mr.PALETTE for s in steps)
    n_img = len([1 for _, m in gr.meta_apply(n_channels, steps)[0] if not m])
    explicit = [sr.params(1, 1, n_meta, n_img), sr.params(0, 0, n_meta + n_img - 1, 1)]
    specs = [_spec(n_channels, steps, [], 37, 53), _spec(n_channels, steps, explicit, 37, 53), _spec(n_channels, steps, None, 37, 53)]
    st, progs, bad, arena, _ = _lower(specs)
    assert st == lib.OK and bad is None
    for p, sq in zip(progs, ([], explicit, None)):
        _check_program(p, n_channels, steps, sq, 37, 53)
    assert all(progs[2].chains[k].n_levels == 0 for k in range(4))
    if n_meta:
        assert all(q[2] >= n_meta for q in sr.default_squeeze(
            [{"meta": True, "w": 0, "h": 0}] * n_meta + [{"meta": False, "w": 37, "h": 53}] * n_img))


def _refused(specs, want, bad_group=1, mutate=None, wp="default", arena_samples=None, **pack):
    from jxl_rs_amd import lib
    L = lib.load()
    arena, (groups, coded, params) = lib.pack_local_squeeze_groups(specs, **pack)
    if mutate:
        mutate(groups, coded, params)
    n = len(specs)
    progs = (lib.LocalSqueezeProgram * n)()
    C.memset(progs, 0x5a, C.sizeof(progs))
    before = bytes(progs)
    bad = C.c_size_t(77)
    hdr = lib.wp_headers([gr.WP_DEFAULT] * n) if wp == "default" else wp
    st = L.jxlh_modular_local_lower_squeeze(groups, n, coded, len(coded), params, len(params), hdr, 8,
                                            arena.size if arena_samples is None else arena_samples, progs, C.byref(bad))
    assert st == want, (st, want)
    if want != lib.OK:
        assert bad.value == bad_group, "the refusal names the group"
        assert bytes(progs) == before, "a refused batch leaves the programs untouched"
    return progs


def test_refusals():
    from jxl_rs_amd import lib
    INV, UNS, OK = lib.ERR_INVALID_ARGUMENT, lib.ERR_UNSUPPORTED, lib.OK
    good = _spec(3, [], [], 20, 12)

    def pair(second):
        return [good, second]

    assert lib.load().jxlh_modular_local_lower_squeeze(None, 1, None, 0, None, 0, None, 8, 0, None, None) == INV
    _refused(pair(_spec(3, [], [], 20, 12)), OK)
    # a channel range that leaves the list, an empty one
    for sq in ([(1, 1, 0, 4)], [(1, 1, 3, 1)], [(0, 0, 2 ** 32 - 1, 2)], [(1, 1, 0, 3), (0, 1, 0, 7)], [(1, 1, 1, 0)]):
        sp = _spec(3, [], [], 20, 12)
        sp["squeeze"] = sq
        _refused(pair(sp), INV)
    # a squeeze of a residual channel; a range that touches a palette meta channel
    sp = _spec(3, [], [], 20, 12)
    sp["squeeze"] = [(1, 1, 0, 1), (0, 1, 1, 1)]
    _refused(pair(sp), UNS)
    pal = [mr.palette(0, 3, mr.small_palette(3))]
    sp = _spec(3, pal, [], 20, 12)
    sp["squeeze"] = [(1, 1, 0, 2)]
    _refused(pair(sp), UNS)
    sp["squeeze"] = [(1, 1, 0, 1)]
    _refused(pair(sp), UNS)
    # more than 16 levels
    sp = _spec(1, [], [sr.params(1, 1, 0, 1)] * 16, 20, 12)
    _refused(pair(sp), OK)
    sp["squeeze"] = sp["squeeze"] + [sr.params(0, 1, 0, 1)]
    _refused(pair(sp), UNS)
    # a transform behind the squeeze, a second squeeze, a bad flag
    _refused(pair(_spec(3, [mr.rct(0, 3)], [], 20, 12, squeeze_pos=0)), UNS)
    _refused(pair(_spec(3, [mr.rct(0, 3)], [], 20, 12, squeeze_pos=2)), INV)
    _refused(pair(_spec(3, [mr.rct(0, 3)], [], 20, 12)), UNS, mutate=lambda g, c, p: setattr(g[1].steps[0], "kind", 2))
    _refused(pair(_spec(3, [], [], 20, 12)), INV, mutate=lambda g, c, p: setattr(g[1], "has_squeeze", 2))
    _refused(pair(_spec(3, [], [(1, 1, 0, 3)], 20, 12)), INV, mutate=lambda g, c, p: setattr(g[1], "has_squeeze", 0))
    # coded channels: missing (previews stay on the host), too many, a wrong size, stride < w, beyond the arena, ranges
    _refused(pair(_spec(3, [], [], 20, 12)), UNS, mutate=lambda g, c, p: setattr(g[1], "n_coded", g[1].n_coded - 1))
    _refused(pair(_spec(3, [], None, 20, 12)), UNS, mutate=lambda g, c, p: setattr(g[1], "n_coded", 2))
    _refused([good, _spec(3, [], [], 20, 12), good], INV, mutate=lambda g, c, p: setattr(g[1], "n_coded", g[1].n_coded + 1))
    _refused(pair(_spec(3, [], [], 20, 12)), INV, mutate=lambda g, c, p: setattr(c[g[1].coded_first + 2], "w", 21))
    _refused(pair(_spec(3, [], [], 20, 12)), INV, mutate=lambda g, c, p: setattr(c[g[1].coded_first + 2], "h", 0))
    _refused(pair(_spec(3, [], [], 20, 12)), INV, mutate=lambda g, c, p: setattr(c[g[1].coded_first], "stride", c[g[1].coded_first].w - 1))
    _refused(pair(_spec(3, [], [], 20, 12)), INV, mutate=lambda g, c, p: setattr(c[len(c) - 1], "offset", 2 ** 64 - 2))
    _refused(pair(_spec(3, [], [], 20, 12)), INV, mutate=lambda g, c, p: setattr(g[1], "coded_first", len(c) - 1))
    _refused(pair(_spec(3, [], [(1, 1, 0, 3)], 20, 12)), INV, mutate=lambda g, c, p: setattr(g[1], "params_first", 1))
    arena, _ = lib.pack_local_squeeze_groups(pair(_spec(3, [], [], 20, 12)), align=1)  # (no padding behind the last row)
    _refused(pair(_spec(3, [], [], 20, 12)), INV, arena_samples=arena.size - 1, align=1)  # the last channel's last sample
    _refused(pair(_spec(3, [], [], 20, 12)), OK, arena_samples=arena.size, align=1)
    # a zero-side channel's offset and stride are not read
    sp = _spec(1, [], [sr.params(1, 1, 0, 1)], 1, 5)
    assert (5, 0) in [c.shape for c in sp["coded"]]
    _refused(pair(sp), OK, mutate=lambda g, c, p: (setattr(c[len(c) - 1], "offset", 2 ** 64 - 1), setattr(c[len(c) - 1], "stride", 0)))
    # a group beyond 2^20 with a squeeze; without one it is the general lowering's business
    _refused(pair(_spec(1, [], [], 8, 8)), UNS, mutate=lambda g, c, p: setattr(g[1], "w", 2 ** 20 + 1))
    # everything the general lowering rejects
    _refused(pair(_spec(3, [mr.rct(0, 3)], [], 20, 12)), INV, mutate=lambda g, c, p: setattr(g[1].steps[0], "rct_type", 42))
    _refused(pair(_spec(3, [], [], 20, 12)), INV, mutate=lambda g, c, p: setattr(g[1], "n_channels", 5))
    wpal = [gr.delta_palette(np.random.default_rng(1), 0, 3, 6)]
    _refused(pair(_spec(3, wpal, [], 20, 12)), INV, wp=None)
    _refused(pair(_spec(3, wpal, [], 20, 12)), OK)


def test_the_existing_calls_still_refuse_a_squeeze():
    from jxl_rs_amd import lib
    L = lib.load()
    arena, groups = lib.pack_local_groups([{"x0": 0, "y0": 0, "n_channels": 3, "steps": [lib.local_rct(0, 1)],
                                           "coded": [np.zeros((4, 4), np.int32)] * 3}])
    groups[0].steps[0].kind = 2
    bad = C.c_size_t(9)
    assert L.jxlh_modular_local_lower(groups, 1, 8, arena.size, None, C.byref(bad)) == lib.ERR_UNSUPPORTED and bad.value == 0
    assert L.jxlh_modular_local_lower_general(groups, None, 1, 8, arena.size, None, C.byref(bad)) == lib.ERR_UNSUPPORTED


def test_calls_validate_before_touching_the_device():
    from jxl_rs_amd import lib
    L = lib.load()
    arena, (groups, coded, params) = lib.pack_local_squeeze_groups([_spec(3, [], [], 20, 12)])
    INV = lib.ERR_INVALID_ARGUMENT
    a = (arena.ctypes.data, arena.size, groups, 1, coded, len(coded), params, len(params), None)
    assert L.jxlh_frame_set_modular_groups_squeeze(None, *a, 8, None) == INV
    assert L.jxlh_frame_set_modular_groups_squeeze_async(None, *a, 8, None) == INV
    assert L.jxlh_modular_local_transforms_squeeze(None, *a, 8, None, 3, 32, 32, 32, None) == INV
    n = C.c_uint32(0)
    assert L.jxlh_modular_local_default_squeeze(None, None, 1, 0, None, 0, C.byref(n)) == INV
    w = (C.c_uint32 * 3)(300, 300, 300)
    assert L.jxlh_modular_local_default_squeeze(w, w, 3, 0, None, 0, C.byref(n)) == INV and n.value == 2 + 12  # counted, not written
    assert L.jxlh_modular_local_default_squeeze(w, w, 5, 0, None, 0, C.byref(n)) == INV


def test_symbols_bindings_and_abi_version():
    from jxl_rs_amd import lib
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_py_binding
    import gen_rust_binding as g
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jxl_hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+JXLH_ABI_VERSION\s+6\b", main), "additions only: the ABI version stays"
    raw = open(g.LOCAL_SQUEEZE_HEADER).read()
    assert '#include "jxl_hip_local_palette.h"' in raw
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    L = lib.load()
    assert L.jxlh_abi_version() == 6
    rust = open(g.OUT_LOCAL_SQUEEZE).read()
    assert "pub mod local_squeeze;" in open(g.OUT).read()
    assert lib.LOCAL_SQUEEZE_SYMBOLS == NAMES
    # the existing lists hold what they held
    assert lib.LOCAL_PALETTE_SYMBOLS == ["jxlh_modular_local_lower_general", "jxlh_modular_local_transforms_general",
                                         "jxlh_frame_set_modular_groups_general", "jxlh_frame_set_modular_groups_general_async"]
    palette_src = open(g.LOCAL_PALETTE_HEADER).read()
    for n in NAMES:
        assert n not in main and n not in palette_src, "declared in the header of its own only"
        assert re.search(r"jxlh_status\s+" + n + r"\s*\(", src), n
        for other in (lib.ABI_SYMBOLS, lib.DEV_SYMBOLS, lib.PREVIEW_SYMBOLS, lib.SAVE_RECTS_SYMBOLS, lib.PREVIEW_TILES_SYMBOLS,
                      lib.EXTRA_RECTS_SYMBOLS, lib.REPAINT_SYMBOLS, lib.LOCAL_PALETTE_SYMBOLS):
            assert n not in other
        assert hasattr(L, n) and getattr(L, n).argtypes is not None, n
        assert f"pub fn {n}(" in rust, n
    for struct, cls in (("jxlh_squeeze_params", lib.SqueezeParams), ("jxlh_local_coded_channel", lib.LocalCodedChannel),
                        ("jxlh_local_squeeze_group", lib.LocalSqueezeGroup), ("jxlh_local_squeeze_level", lib.LocalSqueezeLevel),
                        ("jxlh_local_squeeze_chain", lib.LocalSqueezeChain), ("jxlh_local_squeeze_program", lib.LocalSqueezeProgram)):
        m = re.search(r"pub struct " + struct + r" \{(.*?)\n\}", rust, flags=re.S)
        assert [f for f, _ in re.findall(r"pub (\w+): ([^,\n]+),", m.group(1))] == [f for f, _ in cls._fields_], struct
    assert lib.LOCAL_SQUEEZE_MAX_LEVELS == 16 and "pub const JXLH_LOCAL_SQUEEZE_MAX_LEVELS: u32 = 16;" in rust
    assert callable(lib.Context.set_modular_groups_squeeze) and callable(lib.Context.modular_local_transforms_squeeze)
    assert callable(lib.local_squeeze) and callable(lib.pack_local_squeeze_groups)
    # both generated files are what the generators write today
    assert open(gen_py_binding.OUT).read() == gen_py_binding.generate()
    assert rust == g.generate_local_squeeze()


def test_struct_layouts_match_the_c_compiler(tmp_path):
    from jxl_rs_amd import lib
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "jxl_hip_local_squeeze.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(jxlh_squeeze_params), sizeof(jxlh_local_coded_channel),\n'
                   "         offsetof(jxlh_local_coded_channel, h), sizeof(jxlh_local_squeeze_group),\n"
                   "         offsetof(jxlh_local_squeeze_group, has_squeeze), offsetof(jxlh_local_squeeze_group, n_coded),\n"
                   "         sizeof(jxlh_local_squeeze_chain), sizeof(jxlh_local_squeeze_program),\n"
                   "         offsetof(jxlh_local_squeeze_program, chains));\n  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(lib.SqueezeParams), C.sizeof(lib.LocalCodedChannel), lib.LocalCodedChannel.h.offset,
                   C.sizeof(lib.LocalSqueezeGroup), lib.LocalSqueezeGroup.has_squeeze.offset, lib.LocalSqueezeGroup.n_coded.offset,
                   C.sizeof(lib.LocalSqueezeChain), C.sizeof(lib.LocalSqueezeProgram), lib.LocalSqueezeProgram.chains.offset]


# ---------------------------------------------------------------- the stand-alone program
def _build(tmp_path, sanitize):
    exe = os.path.join(str(tmp_path), "modular_local_squeeze_lower" + ("_san" if sanitize else ""))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                "-static-libasan", "-static-libubsan"]  # the runtimes linked in: the child needs nothing from its environment
    cmd += ["-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "modular_local_squeeze_lower.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _all_cases():
    cases = [(n, [], [], w, h) for (w, h) in sr.RECTS for n in (1, 2, 3, 4)]
    cases += [(n, [], sq, w, h) for (n, sq) in sr.EXPLICIT.values() for (w, h) in ((9, 9), (17, 130), (1, 5))]
    for n, steps in FRONTS.values():
        cases += [(n, steps, [], 37, 53), (n, steps, None, 37, 53)]
    return cases


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitizers"])
def test_squeeze_lowering_stands_alone(tmp_path, sanitize):
    exe = _build(tmp_path, sanitize)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "modular local squeeze lowering: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    # ... and over the same lists as the library
    cases = _all_cases()
    path = tmp_path / "lists.txt"
    with open(path, "w") as f:
        for n_channels, steps, squeeze, w, h in cases:
            f.write(f"{w} {h} {n_channels} {len(steps)}")
            for s in steps:
                f.write(" %d %d %d %d %d %d %d" % (s["kind"], s["begin_c"], s.get("rct_type", 0), s.get("num_c", 0),
                                                    s.get("num_colors", 0), s.get("num_deltas", 0), s.get("predictor", 0)))
            f.write(" %d %d" % (squeeze is not None, len(squeeze or ())))
            for q in squeeze or ():
                f.write(" %d %d %d %d" % q)
            shapes = sr.coded_shapes(n_channels, steps, squeeze, w, h)
            f.write(" %d" % len(shapes) + "".join(" %d %d" % (sw, sh) for sh, sw in shapes) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(cases)
    for line, (n_channels, steps, squeeze, w, h) in zip(lines, cases):
        v = [int(x) for x in line.split()]
        (g_coded, g_slots, _, _), n_coded, chains = sr.expected_program(n_channels, steps, squeeze, w, h)
        assert v[:3] == [0, n_coded, g_coded], (line, n_channels, squeeze, w, h)
        at = 3
        for k, want in enumerate(chains):
            slot, base, bw, bh, nl = v[at:at + 5]
            at += 5
            assert (slot, base, bw, bh, nl) == (g_slots[k], want["base"], want["base_w"], want["base_h"], len(want["levels"]))
            got = [tuple(v[at + 4 * i:at + 4 * i + 4]) for i in range(nl)]
            at += 4 * nl
            assert got == want["levels"]
        assert at == len(v)


# ---------------------------------------------------------------- the test plane is not vacuous
@pytest.mark.parametrize("rect", [(129, 127), (256, 256)], ids=["129x127", "256x256"])
def test_the_plane_reaches_every_tendency_regime(oracle, rect):
    """On the oracle, for the plane the GPU tests use (forward-squeezed with tests/helpers.py under the default squeeze): at
    the finest level of each axis every tendency regime -- zero, positive, negative -- holds at least 5 % of the steps.
    The tendency of a step is what the oracle added to the residual: (a - b) - res of its two outputs."""
    w, h = rect
    rng = np.random.default_rng([129, w, h])
    plane = sr.recipe_plane(rng, h, w)
    coded = sr.forward(1, [], [], [plane])
    trace = []
    out = sr.local_apply(oracle, 1, [], [], w, h, coded, 8, trace=trace)
    assert np.array_equal(out[0], plane), "the forward squeeze of the helpers inverts"
    finest = {}
    for horizontal, avg, res, o in trace:  # the order the steps run in: the last of an axis is its finest
        finest[horizontal] = (res, o)
    assert set(finest) == {True, False}
    for horizontal, (res, o) in finest.items():
        o = o.astype(np.int64)
        if horizontal:
            a, b = o[:, 0:2 * res.shape[1]:2], o[:, 1:2 * res.shape[1]:2]
        else:
            a, b = o[0:2 * res.shape[0]:2, :], o[1:2 * res.shape[0]:2, :]
        t = (a - b) - res
        shares = {"zero": float((t == 0).mean()), "positive": float((t > 0).mean()), "negative": float((t < 0).mean())}
        print(rect, "horizontal" if horizontal else "vertical", shares)
        for regime, share in shares.items():
            assert share >= 0.05, (rect, horizontal, regime, shares)
