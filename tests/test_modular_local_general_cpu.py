"""Group-local palettes with delta entries and predictors, without a GPU: jxlh_modular_local_lower_general (pure host
code) against the extended restatement of meta_apply.rs / apply_local.rs (tests/modular_local_general_ref.py), every new
refusal with its status and first_bad, the old entry point's unchanged refusals, the bindings, the stand-alone lowering
program (plain and under sanitizers), and the proof on the oracle that the input recipe the GPU tests use exercises the
predictors."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import modular_local_general_ref as gr
import modular_local_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (5, 7)
ALL_LISTS = dict(mr.LISTS)
ALL_LISTS.update(gr.GENERAL_LISTS)


def _spec(n_channels, steps, shape=SHAPE):
    from jxl_rs_amd import lib
    try:
        n_coded = mr.expected_program(n_channels, steps)[0]
    except (IndexError, mr.InvalidChannelRange, mr.Unsupported):  # a list the tests expect to be refused
        n_coded = 3
    lsteps = [lib.local_rct(s["begin_c"], s["rct_type"]) if s["kind"] == mr.RCT else
              lib.local_palette(s["begin_c"], s["num_c"], s["table"], s["num_deltas"], s["predictor"]) for s in steps]
    return {"x0": 0, "y0": 0, "n_channels": n_channels, "steps": lsteps, "coded": [np.zeros(shape, np.int32)] * n_coded}


def _check_program(p, n_channels, steps):
    n_coded, coded_slot, ops, n_phases = gr.expected_general_program(n_channels, steps)
    assert p["n_coded"] == n_coded and p["coded_slot"][:n_coded] == coded_slot
    assert p["n_phases"] == n_phases and len(p["ops"]) == len(ops)
    for got, want in zip(p["ops"], ops):  # inverse order: the last step first
        for k in ("kind", "num_colors", "num_deltas", "predictor", "phase"):
            assert got[k] == want[k], (k, got, want)
        if want["kind"] == mr.RCT:
            assert got["rct_op"] == want["rct_op"] and got["n_slots"] == 3
            assert got["in_slot"] == want["reads"] and got["out_slot"][:3] == want["writes"]
        else:
            n = len(want["writes"])
            assert got["n_slots"] == n and got["in_slot"][0] == want["reads"][0] and got["out_slot"][:n] == want["writes"]


def _program_dict(p):
    return {"n_coded": p.n_coded, "coded_slot": list(p.coded_slot), "n_phases": p.n_phases,
            "ops": [{"kind": o.kind, "rct_op": o.rct_op, "n_slots": o.n_slots, "in_slot": list(o.in_slot),
                     "out_slot": list(o.out_slot), "num_colors": o.num_colors, "num_deltas": o.num_deltas,
                     "predictor": o.predictor, "phase": o.phase, "palette_offset": o.palette_offset}
                    for o in list(p.ops)[:p.n_ops]]}


@pytest.mark.parametrize("name", list(ALL_LISTS))
def test_general_lowering_agrees_with_the_restatement(name):
    from jxl_rs_amd import lib
    n_channels, steps = ALL_LISTS[name]
    arena, groups = lib.pack_local_groups([_spec(n_channels, steps)])
    st, progs, bad = lib.modular_local_lower_general(groups, 8, arena.size, wp=[gr.WP_DEFAULT], n=1)
    assert st == lib.OK and bad is None
    p = _program_dict(progs[0])
    _check_program(p, n_channels, steps)
    # the palettes' tables are where the packer put them, num_colors + num_deltas wide
    pal = [s for s in steps if s["kind"] == mr.PALETTE]
    got_pal = [o for o in p["ops"] if o["kind"] != mr.RCT]
    for s, o in zip(reversed(pal), got_pal):
        assert o["num_colors"] == s["table"].shape[1]
        assert np.array_equal(arena[o["palette_offset"]:o["palette_offset"] + s["table"].size], s["table"].reshape(-1))


def test_expected_general_programs_are_what_the_reference_order_implies():
    """the restatement itself on the lists that decide the phases"""
    g = gr.expected_general_program
    assert [(o["kind"], o["phase"]) for o in g(*gr.GENERAL_LISTS["rct_delta_rct"])[2]] == [(mr.RCT, 0), (2, 1), (mr.RCT, 2)]
    assert g(*gr.GENERAL_LISTS["rct_delta_rct"])[3] == 3
    assert [(o["kind"], o["phase"]) for o in g(*gr.GENERAL_LISTS["two_general"])[2]] == [(2, 1), (2, 3)]
    assert [(o["kind"], o["phase"]) for o in g(*gr.GENERAL_LISTS["lookup_and_delta"])[2]] == [(2, 1), (mr.PALETTE, 2)]
    o = g(*gr.GENERAL_LISTS["predictor0_deltas"])
    assert o[3] == 1 and [(x["kind"], x["num_colors"], x["num_deltas"], x["phase"]) for x in o[2]] == [(mr.PALETTE, 16, 0, 0)]
    o = g(*gr.GENERAL_LISTS["general_of_general"])[2]  # the second palette's output (slot 0) is the first one's index
    assert o[0]["writes"] == [0] and o[1]["reads"] == [0] and o[1]["writes"] == [0, 1, 2]


def test_predictors_without_deltas_are_general():
    """a negative index is < num_deltas == 0 and is predicted (palette.rs:239)"""
    from jxl_rs_amd import lib
    for predictor in range(1, 14):
        steps = [mr.palette(0, 3, mr.small_palette(3), 0, predictor)]
        arena, groups = lib.pack_local_groups([_spec(3, steps)])
        st, progs, _ = lib.modular_local_lower_general(groups, 8, arena.size, wp=[gr.WP_DEFAULT], n=1)
        assert st == lib.OK and progs[0].n_phases == 3
        o = progs[0].ops[0]
        assert (o.kind, o.predictor, o.num_deltas, o.num_colors, o.phase) == (lib.LOCAL_GENERAL_PALETTE, predictor, 0, 6, 1)


def _group(steps=(), **over):
    """two groups of three channels; `over` overwrites fields of the second one's first step"""
    from jxl_rs_amd import lib
    arena, groups = lib.pack_local_groups([_spec(3, []), _spec(3, list(steps))])
    for k, v in over.items():
        setattr(groups[1].steps[0], k, v)
    return arena, groups


def _refused(arena, groups, want, wp="default", general=True):
    from jxl_rs_amd import lib
    L = lib.load()
    progs = ((lib.LocalGeneralProgram if general else lib.LocalProgram) * 2)()
    C.memset(progs, 0x5a, C.sizeof(progs))
    before = bytes(progs)
    bad = C.c_size_t(77)
    if general:
        hdr = lib.wp_headers([gr.WP_DEFAULT] * 2) if wp == "default" else wp
        st = L.jxlh_modular_local_lower_general(groups, hdr, 2, 8, arena.size, progs, C.byref(bad))
    else:
        st = L.jxlh_modular_local_lower(groups, 2, 8, arena.size, progs, C.byref(bad))
    assert st == want, (st, want)
    assert bad.value == 1, "group 0 is fine: the refusal names group 1"
    assert bytes(progs) == before, "a refused call writes nothing"


def test_new_refusals():
    from jxl_rs_amd import lib
    L = lib.load()
    INV, UNS = lib.ERR_INVALID_ARGUMENT, lib.ERR_UNSUPPORTED
    rng = np.random.default_rng(1)
    delta = lambda predictor: [gr.delta_palette(rng, 0, 3, predictor)]  # noqa: E731  11 colours + 5 deltas
    assert L.jxlh_modular_local_lower_general(None, None, 1, 8, 0, None, None) == INV
    _refused(*_group(delta(5), predictor=14), INV)
    _refused(*_group(delta(5), predictor=2 ** 32 - 1), INV)
    _refused(*_group(delta(6)), INV, wp=None)                           # predictor 6 without headers
    for field, limit in (("p1c", 32), ("p2c", 32), ("p3ca", 32), ("p3cb", 32), ("p3cc", 32), ("p3cd", 32), ("p3ce", 32),
                         ("w0", 16), ("w1", 16), ("w2", 16), ("w3", 16)):
        hdr = lib.wp_headers([gr.WP_DEFAULT] * 2)
        setattr(hdr[1], field, limit)
        _refused(*_group(delta(6)), INV, wp=hdr)
        setattr(hdr[1], field, limit - 1)
        a, g = _group(delta(6))
        assert L.jxlh_modular_local_lower_general(g, hdr, 2, 8, a.size, None, None) == lib.OK
        setattr(hdr[0], field, limit)                                   # group 0 has no predictor-6 step: not read
        assert L.jxlh_modular_local_lower_general(g, hdr, 2, 8, a.size, None, None) == lib.OK
    a, g = _group(delta(5))
    assert L.jxlh_modular_local_lower_general(g, None, 2, 8, a.size, None, None) == lib.OK  # no step asks for a header
    # the meta channel's rows are num_colors + num_deltas wide
    g[1].steps[0].palette_offset = a.size - 3 * 16
    assert L.jxlh_modular_local_lower_general(g, None, 2, 8, a.size, None, None) == lib.OK
    g[1].steps[0].palette_offset = a.size - 3 * 16 + 1
    _refused(a, g, INV)
    a, g = _group(delta(0))                                             # ... also where it lowers to a look-up
    g[1].steps[0].palette_offset = a.size - 3 * 16 + 1
    _refused(a, g, INV)
    _refused(*_group(delta(5), num_colors=2 ** 31 - 5), INV)             # num_colors + num_deltas = 2^31
    _refused(*_group(delta(5), num_colors=2 ** 32 - 1, num_deltas=2 ** 32 - 1), INV)
    # still unsupported
    _refused(*_group(delta(5), kind=2), UNS)                            # squeeze
    _refused(*_group([gr.delta_palette(rng, 1, 1, 5), mr.rct(0, 0)]), UNS)  # touches the meta channel
    _refused(*_group([gr.delta_palette(rng, 1, 1, 5), gr.delta_palette(rng, 0, 2, 5)]), UNS)
    # still invalid, as in the default mode
    _refused(*_group(delta(5), num_c=0), INV)
    _refused(*_group(delta(5), num_c=4), INV)


@pytest.mark.parametrize("name", [n for n, (_, steps) in gr.GENERAL_LISTS.items()])
def test_the_old_entry_point_still_refuses(name):
    """jxlh_modular_local_lower refuses every list with a delta entry or a predictor, and lowers the others as before"""
    from jxl_rs_amd import lib
    n_channels, steps = gr.GENERAL_LISTS[name]
    arena, groups = lib.pack_local_groups([_spec(3, []), _spec(n_channels, steps)])
    assert any(s["kind"] == mr.PALETTE and (s["num_deltas"] or s["predictor"]) for s in steps)
    _refused(arena, groups, lib.ERR_UNSUPPORTED, general=False)


def test_calls_validate_before_touching_the_device():
    from jxl_rs_amd import lib
    L = lib.load()
    arena, groups = _group()
    INV = lib.ERR_INVALID_ARGUMENT
    assert L.jxlh_frame_set_modular_groups_general(None, arena.ctypes.data, arena.size, groups, None, 2, 8, None) == INV
    assert L.jxlh_frame_set_modular_groups_general_async(None, arena.ctypes.data, arena.size, groups, None, 2, 8, None) == INV
    assert L.jxlh_modular_local_transforms_general(None, arena.ctypes.data, arena.size, groups, None, 2, 8, None, 3, 8, 8, 8, None) == INV


def test_symbols_bindings_and_abi_version():
    from jxl_rs_amd import lib
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_py_binding
    import gen_rust_binding as g
    names = ["jxlh_modular_local_lower_general", "jxlh_modular_local_transforms_general",
             "jxlh_frame_set_modular_groups_general", "jxlh_frame_set_modular_groups_general_async"]
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jxl_hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+JXLH_ABI_VERSION\s+6\b", main), "additions only: the ABI version stays"
    src = re.sub(r"/\*.*?\*/", "", open(g.LOCAL_PALETTE_HEADER).read(), flags=re.S)
    L = lib.load()
    rust = open(g.OUT_LOCAL_PALETTE).read()
    assert "pub mod local_palette;" in open(g.OUT).read()
    assert lib.LOCAL_PALETTE_SYMBOLS == names
    for n in names:
        assert n not in main, "declared in the header of its own only"
        assert re.search(r"jxlh_status\s+" + n + r"\s*\(", src), n
        assert hasattr(L, n) and n not in lib.ABI_SYMBOLS and getattr(L, n).argtypes is not None, n
        assert f"pub fn {n}(" in rust, n
    for struct, cls in (("jxlh_local_general_op", lib.LocalGeneralOp), ("jxlh_local_general_program", lib.LocalGeneralProgram)):
        m = re.search(r"pub struct " + struct + r" \{(.*?)\n\}", rust, flags=re.S)
        assert [f for f, _ in re.findall(r"pub (\w+): ([^,\n]+),", m.group(1))] == [f for f, _ in cls._fields_], struct
    assert lib.LOCAL_GENERAL_PALETTE == 2 and "pub const JXLH_LOCAL_GENERAL_PALETTE: u32 = 2;" in rust
    assert callable(lib.Context.set_modular_groups_general) and callable(lib.Context.modular_local_transforms_general)
    # both generated files are what the generators write today
    assert open(gen_py_binding.OUT).read() == gen_py_binding.generate()
    assert rust == g.generate_local_palette()


def test_struct_layouts_match_the_c_compiler(tmp_path):
    from jxl_rs_amd import lib
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "jxl_hip_local_palette.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(jxlh_local_general_op), offsetof(jxlh_local_general_op, palette_offset),\n'
                   "         sizeof(jxlh_local_general_program), offsetof(jxlh_local_general_program, ops),\n"
                   "         offsetof(jxlh_local_general_op, phase));\n  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(lib.LocalGeneralOp), lib.LocalGeneralOp.palette_offset.offset, C.sizeof(lib.LocalGeneralProgram),
                   lib.LocalGeneralProgram.ops.offset, lib.LocalGeneralOp.phase.offset]


# ---------------------------------------------------------------- the stand-alone program
def _build(tmp_path, sanitize):
    exe = os.path.join(str(tmp_path), "modular_local_general_lower" + ("_san" if sanitize else ""))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                "-static-libasan", "-static-libubsan"]  # the runtimes linked in: the child needs nothing from its environment
    cmd += ["-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "modular_local_general_lower.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitizers"])
def test_general_lowering_stands_alone(tmp_path, sanitize):
    exe = _build(tmp_path, sanitize)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "modular local general lowering: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    # ... and over the same lists as the library
    path = tmp_path / "lists.txt"
    with open(path, "w") as f:
        for n_channels, steps in ALL_LISTS.values():
            f.write(f"{n_channels} {len(steps)}")
            for s in steps:
                f.write(" %d %d %d %d %d %d %d" % (s["kind"], s["begin_c"], s.get("rct_type", 0), s.get("num_c", 0),
                                                    s.get("num_colors", 0), s.get("num_deltas", 0), s.get("predictor", 0)))
            f.write("\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(ALL_LISTS)
    for line, (name, (n_channels, steps)) in zip(lines, ALL_LISTS.items()):
        v = [int(x) for x in line.split()]
        assert v[0] == 0, name
        p = {"n_coded": v[1], "coded_slot": v[2:6], "n_phases": v[6], "ops": []}
        for i in range(v[7]):
            o = v[8 + 14 * i:22 + 14 * i]
            p["ops"].append({"kind": o[0], "rct_op": o[1], "n_slots": o[2], "in_slot": o[3:6], "out_slot": o[6:10],
                             "num_colors": o[10], "num_deltas": o[11], "predictor": o[12], "phase": o[13]})
        _check_program(p, n_channels, steps)


# ---------------------------------------------------------------- the recipe is not vacuous
PROOF_SHAPES = [((37, 53), 0.20), ((300, 258), 0.20), ((1024, 1024), 0.20), ((257, 3), 0.10)]  # (h, w), pairwise bound


@pytest.mark.parametrize("shape,pairwise", PROOF_SHAPES, ids=[f"{h}x{w}" for (h, w), _ in PROOF_SHAPES])
def test_the_recipe_exercises_every_predictor(oracle, shape, pairwise):
    """On the oracle, for the recipe the GPU tests use: at least 40 % of the pixels are predicted (index < num_deltas);
    every predictor 1..13 and the weighted predictor under both non-default headers used on the GPU differ from the
    predictor-0 result on at least 30 % of the samples, and from each other on at least 20 % (257 x 3: 10 % -- on three
    columns several neighbours coincide; the one-row and one-column shapes are exempt for that reason)."""
    rng = np.random.default_rng([7, shape[0], shape[1]])
    num_colors, num_deltas = 11, 5
    table = gr.recipe_table(rng, 3, num_colors, num_deltas, 8)
    idx = gr.recipe_index(rng, shape, num_colors, num_deltas)
    assert (idx < num_deltas).mean() >= 0.40
    zero = oracle.palette_delta(idx, table, num_colors, num_deltas, 8, 0)
    results = {}
    for p in range(1, 14):
        if p == 6:
            continue
        results[f"p{p}"] = oracle.palette_delta(idx, table, num_colors, num_deltas, 8, p)
    for name, hdr in (("wp_default", gr.WP_DEFAULT), ("wp_a", gr.WP_A), ("wp_b", gr.WP_B)):
        results[name] = oracle.palette_delta_wp(idx, table, num_colors, num_deltas, 3, 8, hdr)
    for name, r in results.items():
        assert (r != zero).mean() >= 0.30, (name, float((r != zero).mean()))
    for (a, ra), (b, rb) in itertools.combinations(results.items(), 2):
        assert (ra != rb).mean() >= pairwise, (a, b, float((ra != rb).mean()))
