"""Squeeze previews per grid cell, the host side (no GPU): tests/squeeze_tiles_ref.py against the oracle where the two
overlap (every cell present: the regular steps; masks uniform per level: squeeze_preview_ref.preview_reference);
jxlh_squeeze_tile_kinds -- the public face of jxl_rs_amd/csrc/squeeze_preview_plan.h -- against the restated rule; what
the GPU cases' masks exercise, as conditions on the reference alone; the bindings; the refusals that need no device."""
import functools
import os
import subprocess

import numpy as np
import pytest

import squeeze_tiles_ref as ref
from squeeze_preview_ref import REGULAR, SMOOTH_1D, SMOOTH_2D, explicit_steps, forward_chain, preview_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRESENT = 0x1000   # the host function only tests residual pointers for NULL


def default_steps(w, h):
    from jxl_rs_amd import synth
    return synth.default_squeeze_steps(w, h)[0]


@functools.lru_cache(maxsize=None)
def cases():
    return ref.case_list(default_steps)


@functools.lru_cache(maxsize=None)
def chain_of(w, h, nch=1, directions=None):
    rng = np.random.default_rng([w, h, nch, 7])
    image = [rng.integers(-4000, 4001, size=(h, w)).astype(np.int32) for _ in range(nch)]
    steps = default_steps(w, h) if directions is None else explicit_steps(w, h, directions)[0]
    base, residuals = forward_chain(image, steps)
    return image, steps, base, residuals


def levels_of(steps, level_missing, n_planes=1):
    return [(hz, ow, oh, [None if m else PRESENT] * n_planes, max(ow // 2 if hz else ow, 1))
            for (hz, ow, oh), m in zip(steps, level_missing)]


def base_of(steps):
    hz, ow, oh = steps[0]
    return ((ow + 1) // 2, oh) if hz else (ow, (oh + 1) // 2)


def lib_kinds(steps, tiles, level_missing, level, n_planes=1):
    from jxl_rs_amd import lib
    bw, bh = base_of(steps)
    return lib.squeeze_tile_kinds(levels_of(steps, level_missing, n_planes), tiles, bw, bh, level, n_planes=n_planes)


# ---------------------------------------------------------------- the reference against the oracle
@pytest.mark.parametrize("size,directions", [((40, 24), None), ((33, 29), None), ((70, 50), (True, True, False, False)),
                                             ((1, 40), None)], ids=["40x24", "33x29", "HHVV", "1x40"])
def test_every_cell_present_is_the_oracles_regular_step(oracle, size, directions):
    """level by level, for a few grids: pins the numpy regular step, its prev / next_avg across cell edges included"""
    image, steps, base, residuals = chain_of(*size, 2, directions)
    for finest in ((8, 8), (16, 2), (2, 16), (0, 0)):
        tiles = [(0, 0, None)] * len(steps)
        for k in range(len(steps)):
            tw, th = ref.level_tiles(steps, finest, k) if finest[0] else (0, 0)
            hz = steps[len(steps) - 1 - k][0]
            if tw and (tw % 2 if hz else th % 2):
                break                      # (a cell starts on a pair: coarser levels keep one cell)
            nx, ny = ref.grid_of(steps[len(steps) - 1 - k], (tw, th))[2:]
            tiles[len(steps) - 1 - k] = (tw, th, np.ones((ny, nx), np.uint8))
        final, outputs = ref.tiles_reference(oracle, base, residuals, steps, tiles)
        for level, (hz, ow, oh) in enumerate(steps):
            for c in range(2):
                res = residuals[level][c]
                want = oracle.unsqueeze_h(outputs[level - 1][c], res, ow) if hz else oracle.unsqueeze_v(outputs[level - 1][c], res, oh)
                assert np.array_equal(outputs[level][c], want), (size, finest, level, c)
        for c in range(2):
            assert np.array_equal(final[c], image[c])


def test_a_missing_cell_without_a_complete_pair_is_zero(oracle):
    """33 x 29, cells of 16 x 8, the finest (horizontal) level wholly missing: the last cell column is one sample wide.
    smooth_h_unsqueeze returns at once for such a rect (squeeze.rs:921-923) and the reference's output buffer is freshly
    allocated, so the column is zero -- where the whole-channel step of squeeze_preview_ref writes its samples.  The
    only difference between a uniform mask and the whole-level preview."""
    image, steps, base, residuals = chain_of(33, 29, 1)
    n = len(steps)
    assert steps[n - 1] == (True, 33, 29)
    tiles = [(0, 0, None)] * (n - 1) + [(16, 8, np.zeros((4, 3), np.uint8))]
    got, _ = ref.tiles_reference(oracle, base, residuals, steps, tiles)
    whole = preview_reference(oracle, base, residuals, steps, [False] * (n - 1) + [True])
    assert np.array_equal(got[0][:, :32], whole[0][:, :32])
    assert (got[0][:, 32] == 0).all() and (whole[0][:, 32] != 0).any()
    # present, the same cell copies the trailing average
    present = np.zeros((4, 3), np.uint8)
    present[:, 2] = 1
    tiles[n - 1] = (16, 8, present)
    got, outputs = ref.tiles_reference(oracle, base, residuals, steps, tiles)
    assert np.array_equal(got[0][:, 32], outputs[n - 2][0][:, 16])


@pytest.mark.parametrize("size", [(40, 24), (64, 48), (96, 80)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_uniform_masks_are_the_whole_level_preview(oracle, size):
    """(grids whose cells all hold a complete pair: see test_a_missing_cell_without_a_complete_pair_is_zero)"""
    image, steps, base, residuals = chain_of(*size, 1)
    n = len(steps)
    rng = np.random.default_rng(n)
    for trial in range(12):
        missing = [bool(rng.random() < 0.5) and i > 0 for i in range(n)]
        by_pointer = [bool(rng.random() < 0.5) for _ in range(n)]      # missing by res[] == NULL or by an all-zero mask
        tiles = []
        for k in range(n):
            level = n - 1 - k
            tw, th = ref.level_tiles(steps, (8, 8), k) if k < 3 else (0, 0)
            nx, ny = ref.grid_of(steps[level], (tw, th))[2:]
            tiles.insert(0, (tw, th, None if by_pointer[level] else np.full((ny, nx), 0 if missing[level] else 1, np.uint8)))
        level_missing = [m and p for m, p in zip(missing, by_pointer)]
        got, _ = ref.tiles_reference(oracle, base, residuals, steps, tiles, level_missing)
        want = preview_reference(oracle, base, residuals, steps, missing)
        assert np.array_equal(got[0], want[0]), (size, missing, by_pointer)


# ---------------------------------------------------------------- jxlh_squeeze_tile_kinds against the restated rule
def test_kinds_on_the_case_lists():
    for (g, name), (size, steps, tiles, level_missing, _) in cases().items():
        for level in range(len(steps)):
            want = ref.tile_kinds_ref(steps, tiles, level_missing, level)
            got = lib_kinds(steps, tiles, level_missing, level, n_planes=1 + level % 3)
            assert np.array_equal(got, want), (g, name, level, got, want)


def test_kinds_on_random_masks_and_geometries():
    rng = np.random.default_rng(2024)
    for trial in range(3000):
        w, h = int(rng.integers(1, 90)), int(rng.integers(1, 90))
        n = int(rng.integers(1, 6))
        steps = explicit_steps(w, h, [bool(rng.integers(2)) for _ in range(n)])[0]
        tiles, level_missing = [], []
        for hz, ow, oh in steps:
            if rng.random() < 0.2:
                tw = th = 0
            else:
                tw, th = int(rng.integers(1, 20)), int(rng.integers(1, 20))
                tw, th = (tw * 2, th) if hz else (tw, th * 2)          # a cell starts on a pair
            nx, ny = ref.grid_of((hz, ow, oh), (tw, th))[2:]
            present = None if rng.random() < 0.25 else (rng.random((ny, nx)) < rng.choice([0.2, 0.5, 0.8])).astype(np.uint8)
            tiles.append((tw, th, present))
            level_missing.append(bool(rng.random() < 0.2))
        level = int(rng.integers(n))
        want = ref.tile_kinds_ref(steps, tiles, level_missing, level)
        got = lib_kinds(steps, tiles, level_missing, level, n_planes=1 + trial % 3)
        assert np.array_equal(got, want), (steps, tiles, level_missing, level, got, want)


def test_known_answers():
    """the rule spelled out on 40 x 24, cells of 8 x 8: levels ... V (20 x 24, cells 4 x 8), H (40 x 24, cells 8 x 8)"""
    steps = default_steps(40, 24)
    n = len(steps)
    assert [s[0] for s in steps[-2:]] == [False, True]
    before = np.ones((3, 5), np.uint8)
    before[1, 2] = 0                                   # one missing cell of the vertical level ...
    tiles = [(0, 0, None)] * (n - 2) + [(4, 8, before), (8, 8, np.zeros((3, 5), np.uint8))]
    kinds = lib_kinds(steps, tiles, [False] * n, n - 1)
    want = np.full((3, 5), SMOOTH_1D, np.uint8)
    want[1, 2] = SMOOTH_2D                             # ... makes the horizontal cell above it 2-D, the others 1-D
    assert np.array_equal(kinds, want)
    assert np.array_equal(lib_kinds(steps, tiles, [False] * n, n - 2), np.where(before, REGULAR, SMOOTH_1D))
    # res[] == NULL: wholly missing whatever `present` says
    tiles[n - 1] = (8, 8, np.ones((3, 5), np.uint8))
    assert (lib_kinds(steps, tiles, [False] * (n - 1) + [True], n - 1) == want).all()
    # one cell for the level before: cell 0 decides for every cell
    tiles[n - 2] = (0, 0, np.zeros((1, 1), np.uint8))
    assert (lib_kinds(steps, tiles, [False] * (n - 1) + [True], n - 1) == SMOOTH_2D).all()
    # a level without residual samples is regular
    steps1 = explicit_steps(1, 9, [True, False])[0]
    assert (lib_kinds(steps1, [(0, 0, np.zeros((1, 1), np.uint8))] * 2, [True, True], 0) == REGULAR).all()


# ---------------------------------------------------------------- what the GPU cases exercise
def _runs(kinds, horizontal):
    """regular runs along the squeezed axis -> [(starts at the channel's first sample, smooth cell in front, smooth cell behind)]"""
    lines = kinds if horizontal else kinds.T
    out = []
    for line in lines:
        i = 0
        while i < len(line):
            if line[i] != REGULAR:
                i += 1
                continue
            j = i
            while j < len(line) and line[j] == REGULAR:
                j += 1
            out.append((i == 0, i > 0, j < len(line)))
            i = j
    return out


def _conditions(case_items):
    seen = set()
    for (g, name), (size, steps, tiles, level_missing, masks) in case_items:
        n = len(steps)
        finest = ref.tile_kinds_ref(steps, tiles, level_missing, n - 1)
        if {REGULAR, SMOOTH_1D, SMOOTH_2D} <= set(finest.ravel()):
            seen.add("three kinds on the finest level")
        for level in range(n - ref.N_MIXED, n):
            kinds = ref.tile_kinds_ref(steps, tiles, level_missing, level)
            axis = "H" if steps[level][0] else "V"
            for first, front, behind in _runs(kinds, steps[level][0]):
                if front:
                    seen.add(f"{axis}: a run starts behind a smooth cell")
                if behind:
                    seen.add(f"{axis}: a run ends in front of a smooth cell")
                if first:
                    seen.add("a run starts at the channel's first sample")
            for ty, tx in np.argwhere(kinds == SMOOTH_2D):
                near = {kinds[y, x] for y, x in ((ty - 1, tx), (ty + 1, tx), (ty, tx - 1), (ty, tx + 1))
                        if 0 <= y < kinds.shape[0] and 0 <= x < kinds.shape[1]}
                if {REGULAR, SMOOTH_1D} <= near:
                    seen.add("a 2-D cell touches a 1-D cell and a regular cell")
    return seen


ALL_CONDITIONS = {"three kinds on the finest level", "H: a run starts behind a smooth cell", "V: a run starts behind a smooth cell",
                  "H: a run ends in front of a smooth cell", "V: a run ends in front of a smooth cell",
                  "a 2-D cell touches a 1-D cell and a regular cell", "a run starts at the channel's first sample"}


def test_the_masks_exercise_what_they_claim():
    """Conditions on the reference's kind maps, not measurements.  A single mask cannot meet all of them (one missing
    cell has one kind), so they are held over each geometry's case list: the two geometries whose grids have several
    cells on both axes meet every one alone, the one-row and one-column grids every one their axis allows."""
    for g in ref.GEOMETRIES:
        seen = _conditions([(k, v) for k, v in cases().items() if k[0] == g])
        if g in ("40x24", "33x29"):
            assert seen == ALL_CONDITIONS, (g, ALL_CONDITIONS - seen)
        else:
            across = "V" if g != "24x600" else "H"       # the axis with one cell
            assert seen >= {c for c in ALL_CONDITIONS if not c.startswith(across + ":")} - {"a 2-D cell touches a 1-D cell and a regular cell"}, (g, seen)


@pytest.mark.parametrize("g", list(ref.GEOMETRIES))
def test_every_mask_byte_matters(oracle, g):
    """flipping any single byte of any mask of any GPU case changes a sample of the reference's final planes: the inputs
    are uniform noise, so a wrong cell mapping cannot hide"""
    size, _ = ref.GEOMETRIES[g]
    image, steps, base, residuals = chain_of(*size, 1)
    n = len(steps)
    plain = [(0, 0, None)] * n
    _, prefix = ref.tiles_reference(oracle, base, residuals, steps[:n - ref.N_MIXED], plain[:n - ref.N_MIXED])
    for (gg, name), (_, _, tiles, level_missing, masks) in cases().items():
        if gg != g:
            continue
        want, outputs = ref.tiles_reference(oracle, base, residuals, steps, tiles, level_missing, outputs=prefix, start=n - ref.N_MIXED)
        for level in range(n - ref.N_MIXED, n):
            present = tiles[level][2]
            if present is None:
                continue
            for ty, tx in np.ndindex(present.shape):
                flipped = present.copy()
                flipped[ty, tx] ^= 1
                t2 = list(tiles)
                t2[level] = (tiles[level][0], tiles[level][1], flipped)
                got, _ = ref.tiles_reference(oracle, base, residuals, steps, t2, level_missing, outputs=outputs, start=level)
                assert not np.array_equal(got[0], want[0]), (g, name, level, tx, ty)


# ---------------------------------------------------------------- bindings, refusals
def test_bindings_name_the_new_entry_points(tmp_path):
    import ctypes as C
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_py_binding
    import gen_rust_binding
    from jxl_rs_amd import lib, _abi
    assert lib.ABI_VERSION == 6
    assert _abi.PREVIEW_TILES_SYMBOLS == ["jxlh_squeeze_tile_kinds", "jxlh_unsqueeze_chain_preview_tiles"]
    assert not set(_abi.PREVIEW_TILES_SYMBOLS) & set(_abi.ABI_SYMBOLS + _abi.DEV_SYMBOLS + _abi.PREVIEW_SYMBOLS + _abi.SAVE_RECTS_SYMBOLS)
    L = lib._lib()
    for name, nargs in (("jxlh_squeeze_tile_kinds", 8), ("jxlh_unsqueeze_chain_preview_tiles", 14)):
        fn = getattr(L, name)
        assert fn.restype is C.c_int32 and len(fn.argtypes) == nargs, name
    assert C.sizeof(lib.SqueezeTiles) == 16 and lib.SqueezeTiles.present.offset == 8
    assert hasattr(lib.Context, "unsqueeze_chain_preview_tiles") and hasattr(lib, "squeeze_tile_kinds")
    from jxl_rs_amd.modular import ModularChain
    assert hasattr(ModularChain, "preview_tiles")
    assert open(gen_py_binding.OUT).read() == gen_py_binding.generate()
    assert open(gen_rust_binding.OUT_PREVIEW_TILES).read() == gen_rust_binding.generate_preview_tiles()
    header = open(os.path.join(ROOT, "include", "jxl_hip_preview_tiles.h")).read()
    main_header = open(os.path.join(ROOT, "include", "jxl_hip.h")).read()
    rust = open(gen_rust_binding.OUT_PREVIEW_TILES).read()
    hpp = open(os.path.join(ROOT, "include", "jxl_hip.hpp")).read()
    assert '#include "jxl_hip_preview_tiles.h"' in main_header and "pub mod preview_tiles;" in open(gen_rust_binding.OUT).read()
    for name in _abi.PREVIEW_TILES_SYMBOLS:
        assert f"jxlh_status {name}(" in header and f"pub fn {name}(" in rust and name + "(" in hpp, name
    assert "pub struct jxlh_squeeze_tiles" in rust and "pub present: *const u8," in rust
    assert "#define JXLH_ABI_VERSION 6" in main_header
    for i, first in enumerate(("jxl_hip.h", "jxl_hip_preview_tiles.h")):
        src = os.path.join(str(tmp_path), f"order{i}.c")
        with open(src, "w") as f:
            f.write(f'#include "{first}"\n#include "jxl_hip_preview_tiles.h"\n#include "jxl_hip.h"\n'
                    "jxlh_status (*kinds)(int32_t, int32_t, const jxlh_squeeze_level*, const jxlh_squeeze_tiles*, uint32_t, uint32_t,\n"
                    "                     int32_t, uint8_t*) = jxlh_squeeze_tile_kinds;\njxlh_squeeze_tiles t = {8, 8, 0};\n")
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src,
                            "-o", src + ".o"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]


def test_refusals():
    from jxl_rs_amd import lib
    steps = default_steps(40, 24)
    n = len(steps)
    bw, bh = base_of(steps)
    levels = levels_of(steps, [False] * n)

    def status(tiles, levels=levels, level=n - 1, bw_=bw):
        try:
            lib.squeeze_tile_kinds(levels, tiles, bw_, bh, level)
        except lib.JxlHipError as e:
            return e.status
        return lib.OK

    plain = [(0, 0, None)] * n
    assert status(plain) == lib.OK
    assert status(plain, bw_=bw + 1) == lib.ERR_INVALID_ARGUMENT                 # the chain's own rules come first
    assert status(plain[:-1] + [(8, 0, None)]) == lib.ERR_INVALID_ARGUMENT       # one of the two zero
    assert status(plain[:-1] + [(0, 8, None)]) == lib.ERR_INVALID_ARGUMENT
    assert status(plain[:-1] + [(7, 8, None)]) == lib.ERR_INVALID_ARGUMENT       # an odd tile_w on a horizontal level
    assert status(plain[:-1] + [(8, 7, None)]) == lib.OK                         # ... its tile_h may be odd
    assert status(plain[:-1] + [(41, 8, None)]) == lib.OK                        # ... and so may one cell column's width
    assert status(plain[:-2] + [(4, 7, None), (0, 0, None)]) == lib.ERR_INVALID_ARGUMENT   # an odd tile_h on a vertical level
    assert status(plain[:-2] + [(3, 8, None), (0, 0, None)]) == lib.OK
    assert status(plain[:-2] + [(4, 25, None), (0, 0, None)]) == lib.OK
    assert status(plain, level=n) == lib.ERR_INVALID_ARGUMENT
    assert status(plain, level=-1) == lib.ERR_INVALID_ARGUMENT
    # more than 2^20 cells in a level
    big = explicit_steps(4096, 2048, [True])[0]
    big_levels = levels_of(big, [False])
    assert status([(2, 2, None)], levels=big_levels, level=0, bw_=2048) == lib.ERR_INVALID_ARGUMENT     # 2^21 cells
    try:
        lib.squeeze_tile_kinds(big_levels, [(4, 2, None)], 2048, 2048, 0)                               # 2^20: allowed
    except lib.JxlHipError as e:
        raise AssertionError(e.status)
    L = lib._lib()
    arr = lib._squeeze_levels(levels, 1)
    kinds = np.zeros(64, np.uint8)
    assert L.jxlh_squeeze_tile_kinds(1, n, arr, None, bw, bh, n - 1, kinds.ctypes.data) == lib.ERR_INVALID_ARGUMENT   # no tiles
    tarr, keep = lib._squeeze_tiles(levels, plain)
    assert L.jxlh_squeeze_tile_kinds(1, n, arr, tarr, bw, bh, n - 1, None) == lib.ERR_INVALID_ARGUMENT               # no kinds
    assert L.jxlh_squeeze_tile_kinds(1, n, None, tarr, bw, bh, n - 1, kinds.ctypes.data) == lib.ERR_INVALID_ARGUMENT


# ---------------------------------------------------------------- the planner header on its own
def _build_plan_program(tmp_path, name, extra):
    exe = os.path.join(str(tmp_path), name)
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "squeeze_tiles_plan.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_planner_header_alone(tmp_path):
    """runs are maximal, disjoint and cover exactly the regular cells; every cell is in exactly one list; offsets stay
    inside the planes: on the case geometries and on random masks, without a library or a device"""
    exe = _build_plan_program(tmp_path, "squeeze_tiles_plan", ["-O2"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "squeeze tile plans: ok" in r.stdout, (r.stdout + r.stderr)[-2000:]


def test_planner_header_alone_under_host_sanitizers(tmp_path):
    """the same stand-alone program, host compile with AddressSanitizer and UBSan: nothing is loaded into Python"""
    exe = _build_plan_program(tmp_path, "squeeze_tiles_plan_san",
                              ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "squeeze tile plans: ok" in r.stdout, (r.stdout + r.stderr)[-2000:]
