"""tests/modular_local_ref.py extended to every local palette (TransformStep::Palette::local_apply ->
do_palette_step_general, apply_local.rs:260-294, palette.rs:165-262): the same channel-list bookkeeping, with each
palette step keeping its num_deltas and predictor; what jxlh_modular_local_lower_general must report (the look-up /
general split and the phases); local_apply with the committed oracle's palette_delta / palette_delta_wp run on the
group's own h x w arrays; and the input recipe the GPU tests and the CPU proof share."""
import numpy as np

import modular_local_ref as mr
from modular_local_ref import PALETTE, RCT, palette, rct, small_palette  # noqa: F401

GENERAL_PALETTE = 2
WP_DEFAULT = (16, 10, 7, 7, 7, 0, 0, 13, 12, 12, 12)  # WeightedHeader::default, headers/modular.rs
WP_A = (31, 0, 5, 19, 7, 3, 30, 15, 0, 1, 9)
WP_B = (0, 31, 31, 0, 0, 31, 1, 0, 15, 15, 0)


def meta_apply(n_channels, steps):
    """mr.meta_apply; the palette steps also carry num_deltas and predictor (the i-th recorded step is the i-th list
    entry: meta_apply_single_transform records exactly one per transform)"""
    channels, tsteps, n_buf = mr.meta_apply(n_channels, steps)
    for t, s in zip(tsteps, steps):
        if s["kind"] == PALETTE:
            t["num_deltas"], t["predictor"] = s["num_deltas"], s["predictor"]
    return channels, tsteps, n_buf


def expected_general_program(n_channels, steps):
    """-> (n_coded, coded_slot, ops, n_phases); ops, last step first: dicts with kind, rct_op, reads, writes and for
    palettes num_colors (= the step's num_colors + num_deltas), num_deltas, predictor; and the phase.  Predictor 0 is the
    look-up op whatever num_deltas is; every other predictor is a general palette, in an odd phase of its own."""
    n_coded, coded, ops = mr.expected_program(n_channels, steps)
    pal = [s for s in reversed(steps) if s["kind"] == PALETTE]
    out, phase, generals = [], 0, 0
    for kind, op, reads, writes in ops:
        d = {"kind": kind, "rct_op": op, "reads": reads, "writes": writes, "num_colors": 0, "num_deltas": 0, "predictor": 0}
        general = False
        if kind == PALETTE:
            s = pal.pop(0)
            d["num_colors"] = s["num_colors"] + s["num_deltas"]
            general = s["predictor"] != 0
            if general:
                d["kind"], d["num_deltas"], d["predictor"] = GENERAL_PALETTE, s["num_deltas"], s["predictor"]
        if general:
            phase += 2 if phase % 2 else 1
            generals += 1
        else:
            phase += phase % 2
        d["phase"] = phase
        out.append(d)
    return n_coded, coded, out, 1 + 2 * generals


def local_apply(oracle, n_channels, steps, coded, bit_depth, wp=None):
    """mr.local_apply with every palette by oracle.palette_delta (predictor 6: oracle.palette_delta_wp under `wp`, the
    group's header)"""
    channels, tsteps, _ = meta_apply(n_channels, steps)
    image = [b for b, meta in channels if not meta]
    assert len(image) == len(coded)
    buffers = {b: np.ascontiguousarray(c, dtype=np.int32) for b, c in zip(image, coded)}
    depth = min(bit_depth, 24)
    for s in reversed(tsteps):
        if s["kind"] == RCT:
            res = oracle.rct([buffers.pop(b) for b in s["buf_in"]], s["op"], s["perm"])
        else:
            idx, nb = buffers.pop(s["buf_in"]), len(s["buf_out"])
            if s["predictor"] == 6:
                res = oracle.palette_delta_wp(idx, s["table"], s["num_colors"], s["num_deltas"], nb, depth, wp)
            else:
                res = oracle.palette_delta(idx, s["table"], s["num_colors"], s["num_deltas"], depth, s["predictor"])
        for b, r in zip(s["buf_out"], res):
            buffers[b] = r
    return [buffers[c] for c in range(n_channels)]


# ---- the input recipe: test_delta_palette_bit_exact's, with per-pixel draws
def recipe_table(rng, num_c, num_colors, num_deltas, bit_depth):
    """[num_c, num_deltas + num_colors]: delta entries in [-12, 12] first, then entries in [0, 2^bit_depth)"""
    t = rng.integers(0, 1 << bit_depth, size=(num_c, num_deltas + num_colors), dtype=np.int64)
    t[:, :num_deltas] = rng.integers(-12, 13, size=(num_c, num_deltas))
    return t.astype(np.int32)


def recipe_index(rng, shape, num_colors, num_deltas):
    """indices in [-8, num_colors + num_deltas + 200), half of the pixels redrawn per pixel in [0, num_deltas)"""
    idx = rng.integers(-8, num_colors + num_deltas + 200, size=shape, dtype=np.int64)
    redraw = rng.random(shape) < 0.5
    if num_deltas > 0:
        idx[redraw] = rng.integers(0, num_deltas, size=int(redraw.sum()))
    return idx.astype(np.int32)


def delta_palette(rng, begin_c, num_c, predictor, num_colors=11, num_deltas=5, bit_depth=8):
    return palette(begin_c, num_c, recipe_table(rng, num_c, num_colors, num_deltas, bit_depth), num_deltas, predictor)


def coded_for(n_channels, steps, shape, rng, lo=0, hi=64):
    """coded channels for `steps`: a palette's index channel by recipe_index where the list's LAST palette reads a coded
    channel directly, random samples in [lo, hi) elsewhere (every i32 is a valid index)"""
    channels, tsteps, _ = meta_apply(n_channels, steps)
    index_of = {t["buf_in"]: t for t in tsteps if t["kind"] == PALETTE}
    out = []
    for b, meta in channels:
        if meta:
            continue
        if b in index_of:
            t = index_of[b]
            out.append(recipe_index(rng, shape, t["num_colors"], t["num_deltas"]))
        else:
            out.append(rng.integers(lo, hi, size=shape, dtype=np.int64).astype(np.int32))
    return out


_rng = np.random.default_rng(20)
# (n_channels, steps): the lists of the issue beyond mr.LISTS, in its order
GENERAL_LISTS = {
    "delta_0_3": (3, [delta_palette(_rng, 0, 3, 5)]),
    "delta_0_4": (4, [delta_palette(_rng, 0, 4, 4)]),
    "delta_grey": (1, [delta_palette(_rng, 0, 1, 1)]),
    "rct_delta": (3, [rct(0, 23), delta_palette(_rng, 0, 3, 13)]),
    "delta_2_1_rct_1": (3, [delta_palette(_rng, 2, 1, 3), rct(1, 10)]),  # [meta, c0, c1, idx]: the RCT on c0, c1, idx
    "delta_1_1_rct_rest": (4, [delta_palette(_rng, 3, 1, 2), rct(1, 31)]),  # the RCT on the three remaining channels
    "lookup_and_delta": (4, [palette(3, 1, small_palette(1)), delta_palette(_rng, 1, 3, 11)]),
    "two_general": (4, [delta_palette(_rng, 3, 1, 7), delta_palette(_rng, 1, 3, 12)]),
    "predictor0_deltas": (3, [delta_palette(_rng, 0, 3, 0)]),
    "weighted": (3, [delta_palette(_rng, 0, 3, 6)]),
    # [meta, idx, c1, c2]: the last RCT runs first and PRODUCES the index, the palette fills slot 0, the first RCT ends
    "rct_delta_rct": (3, [rct(0, 9), delta_palette(_rng, 0, 1, 5, num_colors=40), rct(1, 4)]),
    # [meta1, idx1] -> [meta2, meta1, idx2]: the second palette's output is the first one's index
    "general_of_general": (3, [delta_palette(_rng, 0, 3, 5), delta_palette(_rng, 1, 1, 2)]),
}
