"""Group-local Modular transforms without a GPU: jxlh_modular_local_lower (pure host code) against the restatement of the
reference's channel-list bookkeeping (tests/modular_local_ref.py), every documented refusal with its status and
first_bad, and the bindings (ctypes, generated Rust crate, header)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import modular_local_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (5, 7)


_pal, LISTS = mr.small_palette, mr.LISTS


def _spec(n_channels, steps, x0=0, y0=0, shape=SHAPE):
    from jxl_rs_amd import lib
    try:
        n_coded = mr.expected_program(n_channels, steps)[0]
    except (IndexError, mr.InvalidChannelRange, mr.Unsupported):  # a list the tests expect to be refused
        n_coded = 3
    lsteps = [lib.local_rct(s["begin_c"], s["rct_type"]) if s["kind"] == mr.RCT else
              lib.local_palette(s["begin_c"], s["num_c"], s["table"], s["num_deltas"], s["predictor"]) for s in steps]
    return {"x0": x0, "y0": y0, "n_channels": n_channels, "steps": lsteps, "coded": [np.zeros(shape, np.int32)] * n_coded}


@pytest.mark.parametrize("name", list(LISTS))
def test_lowering_agrees_with_the_restatement(name):
    from jxl_rs_amd import lib
    n_channels, steps = LISTS[name]
    n_coded, coded_slot, ops = mr.expected_program(n_channels, steps)
    arena, groups = lib.pack_local_groups([_spec(n_channels, steps)])
    st, progs, bad = lib.modular_local_lower(groups, 8, arena.size, n=1)
    assert st == lib.OK and bad is None
    p = progs[0]
    assert p.n_coded == n_coded and list(p.coded_slot)[:n_coded] == coded_slot
    assert p.n_ops == len(ops)
    for got, (kind, op, reads, writes) in zip(p.ops, ops):  # inverse order: the last step first
        assert got.kind == kind
        if kind == mr.RCT:
            assert got.rct_op == op and got.n_slots == 3
            assert list(got.in_slot) == reads and list(got.out_slot)[:3] == writes
        else:
            assert got.n_slots == len(writes) and got.in_slot[0] == reads[0] and list(got.out_slot)[:len(writes)] == writes
    # the palettes' tables are where the packer put them
    pal = [s for s in steps if s["kind"] == mr.PALETTE]
    got_pal = [o for o in list(p.ops)[:p.n_ops] if o.kind == mr.PALETTE]
    for s, o in zip(reversed(pal), got_pal):
        assert o.num_colors == s["num_colors"]
        assert np.array_equal(arena[o.palette_offset:o.palette_offset + s["table"].size], s["table"].reshape(-1))


def test_expected_programs_are_what_the_reference_order_implies():
    """the restatement itself, on the case where the meta channel shifts the indices: [Palette(2,1), RCT(begin_c=1)]
    leaves [meta, c0', c1', idx'] -- the RCT runs first on slots 0, 1, 2 (perm 1: w0 -> 1, w1 -> 2, w2 -> 0), then the
    palette expands slot 2 in place"""
    n_coded, coded, ops = mr.expected_program(*LISTS["palette_2_1_rct_1"])
    assert (n_coded, coded) == (3, [0, 1, 2])
    assert ops == [(mr.RCT, 3, [0, 1, 2], [1, 2, 0]), (mr.PALETTE, 0, [2], [2])]
    assert mr.expected_program(*LISTS["palette_0_4"])[:2] == (1, [0])
    assert mr.expected_program(*LISTS["palette_1_1"])[:2] == (3, [0, 1, 2])


def _group(steps=(), **over):
    """two groups of three channels; `over` overwrites fields of the second one"""
    from jxl_rs_amd import lib
    arena, groups = lib.pack_local_groups([_spec(3, []), _spec(3, list(steps))])
    for k, v in over.items():
        setattr(groups[1], k, v)
    return arena, groups


def _refused(arena, groups, want, bit_depth=8, arena_samples=None):
    from jxl_rs_amd import lib
    L = lib.load()
    progs = (lib.LocalProgram * 2)()
    C.memset(progs, 0x5a, C.sizeof(progs))
    before = bytes(progs)
    bad = C.c_size_t(77)
    st = L.jxlh_modular_local_lower(groups, 2, bit_depth, arena.size if arena_samples is None else arena_samples, progs, C.byref(bad))
    assert st == want, (st, want)
    assert bad.value == 1, "group 0 is fine: the refusal names group 1"
    assert bytes(progs) == before, "a refused call writes nothing"


def test_invalid_arguments():
    from jxl_rs_amd import lib
    L = lib.load()
    INV = lib.ERR_INVALID_ARGUMENT
    assert L.jxlh_modular_local_lower(None, 1, 8, 0, None, None) == INV
    _refused(*_group(n_channels=0), INV)
    _refused(*_group(n_channels=5), INV)
    _refused(*_group(n_steps=5), INV)
    _refused(*_group(n_coded=0), INV)
    _refused(*_group(n_coded=5), INV)
    _refused(*_group(n_coded=2), INV)                                 # three channels, no step: three coded
    _refused(*_group(steps=[mr.palette(0, 3, _pal(3))], n_coded=3), INV)  # the palette leaves one
    _refused(*_group(steps=[mr.rct(0, 42)]), INV)
    _refused(*_group(steps=[mr.rct(1, 0)]), INV)                      # InvalidChannelRange: 1 + 3 > 3
    _refused(*_group(steps=[mr.palette(0, 3, _pal(3)), mr.rct(0, 0)]), INV)  # [meta, idx]: 0 + 3 > 2
    _refused(*_group(coded_stride=SHAPE[1] - 1), INV)
    a, g = _group()
    extent = (SHAPE[0] - 1) * g[1].coded_stride + SHAPE[1]
    g[1].coded_offset[2] = a.size - extent                             # the last row ends with the arena: fine
    assert L.jxlh_modular_local_lower(g, 2, 8, a.size, None, None) == lib.OK
    g[1].coded_offset[2] = a.size - extent + 1                         # ... one sample out
    _refused(a, g, INV)
    g[1].coded_offset[2] = 2 ** 64 - 1                                # offset + extent wraps
    _refused(a, g, INV)
    a, g = _group(steps=[mr.palette(0, 3, _pal(3))])
    g[1].steps[0].palette_offset = a.size - 3 * 6 + 1
    _refused(a, g, INV)
    a, g = _group(steps=[mr.palette(0, 3, _pal(3))])
    g[1].steps[0].num_colors = 0                                      # num_colors + num_deltas == 0
    _refused(a, g, INV)
    _refused(*_group(steps=[mr.palette(0, 3, _pal(3))]), INV, bit_depth=0)
    _refused(*_group(steps=[mr.palette(0, 3, _pal(3))]), INV, bit_depth=32)
    a, g = _group(steps=[mr.palette(0, 3, _pal(3))])
    g[1].steps[0].num_c = 0
    _refused(a, g, INV)
    a, g = _group(steps=[mr.palette(0, 3, _pal(3))])
    g[1].steps[0].num_c = 4                                           # 0 + 4 > 3
    _refused(a, g, INV)


def test_unsupported_groups():
    from jxl_rs_amd import lib
    UNS = lib.ERR_UNSUPPORTED
    _refused(*_group(steps=[mr.palette(0, 3, _pal(3), num_deltas=2)]), UNS)
    _refused(*_group(steps=[mr.palette(0, 3, _pal(3), predictor=5)]), UNS)
    _refused(*_group(steps=[mr.palette(1, 1, _pal(1)), mr.rct(0, 0)]), UNS)      # [meta, c0, idx, c2]: touches the meta channel
    _refused(*_group(steps=[mr.palette(1, 1, _pal(1)), mr.palette(0, 2, _pal(2))]), UNS)  # a palette of a palette
    a, g = _group(steps=[mr.rct(0, 0)])
    g[1].steps[0].kind = 2                                            # squeeze
    _refused(a, g, UNS)
    # ... and the restatement refuses the same lists
    with pytest.raises(mr.Unsupported):
        mr.meta_apply(3, [mr.palette(1, 1, _pal(1)), mr.rct(0, 0)])
    with pytest.raises(mr.InvalidChannelRange):
        mr.meta_apply(3, [mr.rct(1, 0)])


def test_accepted_without_programs_and_empty_batches():
    from jxl_rs_amd import lib
    L = lib.load()
    arena, groups = _group(steps=[mr.rct(0, 5)])
    assert L.jxlh_modular_local_lower(groups, 2, 0, arena.size, None, None) == lib.OK  # bit depth 0: no palette asks
    assert L.jxlh_modular_local_lower(None, 0, 8, 0, None, None) == lib.OK
    groups[1].w = 0  # an empty rect is skipped: its offsets are not read
    groups[1].coded_offset[0] = 2 ** 40
    assert L.jxlh_modular_local_lower(groups, 2, 8, arena.size, None, None) == lib.OK


def test_calls_validate_before_touching_the_device():
    from jxl_rs_amd import lib
    L = lib.load()
    arena, groups = _group()
    assert L.jxlh_frame_set_modular_groups(None, arena.ctypes.data, arena.size, groups, 2, 8, None) == lib.ERR_INVALID_ARGUMENT
    assert L.jxlh_frame_set_modular_groups_async(None, arena.ctypes.data, arena.size, groups, 2, 8, None) == lib.ERR_INVALID_ARGUMENT
    assert L.jxlh_modular_local_transforms(None, arena.ctypes.data, arena.size, groups, 2, 8, None, 3, 8, 8, 8, None) == lib.ERR_INVALID_ARGUMENT


def test_symbols_bindings_and_abi_version():
    from jxl_rs_amd import lib
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_binding as g
    names = ["jxlh_modular_local_lower", "jxlh_modular_local_transforms", "jxlh_frame_set_modular_groups",
             "jxlh_frame_set_modular_groups_async"]
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jxl_hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+JXLH_ABI_VERSION\s+6\b", src), "additions only: the ABI version stays"
    L = lib.load()
    rust = open(g.OUT).read()
    safe = open(os.path.join(ROOT, "bindings", "rust", "jxl_hip", "src", "lib.rs")).read()
    for n in names:
        assert re.search(r"jxlh_status\s+" + n + r"\s*\(", src), n
        assert hasattr(L, n) and n in lib.ABI_SYMBOLS and getattr(L, n).argtypes is not None, n
        assert f"pub fn {n}(" in rust, n
    assert "sys::jxlh_frame_set_modular_groups(" in safe and "sys::jxlh_modular_local_lower(" in safe
    for struct, cls in (("jxlh_local_step", lib.LocalStep), ("jxlh_local_group", lib.LocalGroup),
                        ("jxlh_local_op", lib.LocalOp), ("jxlh_local_program", lib.LocalProgram)):
        m = re.search(r"pub struct " + struct + r" \{(.*?)\n\}", rust, flags=re.S)
        assert [f for f, _ in re.findall(r"pub (\w+): ([^,\n]+),", m.group(1))] == [f for f, _ in cls._fields_], struct
    assert (lib.LOCAL_MAX_STEPS, lib.LOCAL_MAX_CHANNELS, lib.LOCAL_RCT, lib.LOCAL_PALETTE) == (4, 4, 0, 1)
    assert callable(lib.Context.set_modular_groups) and callable(lib.Context.modular_local_transforms)


def test_lowering_stands_alone(tmp_path):
    """tests/cpp/modular_local_lower.cc: the lowering header compiled as plain C++ without the library (the program a
    sanitizer build runs): known lists, refusals and a sweep of random descriptors"""
    import subprocess
    exe = str(tmp_path / "modular_local_lower")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "modular_local_lower.cc"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "modular local lowering: ok" in r.stdout, (r.stdout + r.stderr)[-2000:]
