"""The inputs of the tests of the group-local transforms with extra channels (jxl_hip_local_extra.h): the (layout, step
list) pairs tests/test_gpu_modular_local_extra.py runs, as group specs with their coded channels, built from seeds.
tests/test_modular_local_extra_cpu.py proves on the oracle that these inputs can tell mistakes apart (a plain copy, a
slot mix-up, a palette arm that is never taken); the GPU tests then use the same builders with the same seeds."""
import numpy as np

import modular_local_general_ref as gr
import modular_local_ref as mr
import modular_local_squeeze_ref as sr

PALETTE_COLORS, PALETTE_DELTAS = 40, 12


def table(rng, num_c, num_deltas):
    """[num_c, num_deltas + PALETTE_COLORS]: delta entries in [-12, 12] first, then 8-bit entries"""
    return gr.recipe_table(rng, num_c, PALETTE_COLORS, num_deltas, 8)


def index_plane(rng, shape, num_colors, num_deltas):
    """indices drawn per pixel from the palette's arms in equal shares: delta entries [0, num_deltas) when it has any,
    explicit entries [num_deltas, num_deltas + num_colors), implicit ones (behind the table, and small negatives)"""
    n = num_colors + num_deltas
    arms = [rng.integers(num_deltas, n, size=shape), np.where(rng.random(shape) < 0.25, rng.integers(-8, 0, size=shape),
                                                               rng.integers(n, n + 200, size=shape))]
    if num_deltas:
        arms.append(rng.integers(0, num_deltas, size=shape))
    pick = rng.integers(0, len(arms), size=shape)
    return np.choose(pick, arms).astype(np.int32)


def arm_shares(idx, num_colors, num_deltas):
    n = num_colors + num_deltas
    return {"delta": float(((idx >= 0) & (idx < num_deltas)).mean()), "explicit": float(((idx >= num_deltas) & (idx < n)).mean()),
            "implicit": float(((idx < 0) | (idx >= n)).mean())}


# name -> (steps(rng, n_channels), squeeze(n_channels)): the step lists of the issue.  RCTs are of op 6 (YCoCg: every
# output differs from every input; ops 0..5 pass a channel through), with the permutation varying.
def _pal(rng, begin_c, num_c, num_deltas=0, predictor=0):
    return mr.palette(begin_c, num_c, table(rng, num_c, num_deltas), num_deltas, predictor)


def _general(predictor):
    return lambda rng, n: [_pal(rng, 0, n, PALETTE_DELTAS, predictor)]


STEP_LISTS = {
    "none": (lambda rng, n: [], None),
    "rct": (lambda rng, n: [mr.rct(0, 6 + 7 * int(rng.integers(0, 6)))], None),
    "palette_all": (lambda rng, n: [_pal(rng, 0, n)], None),
    "palette_last": (lambda rng, n: [_pal(rng, n - 1, 1)], None),
    "rct_palette": (lambda rng, n: [mr.rct(0, 13), _pal(rng, n - 1, 1)], None),
    "general_p0": (_general(0), None),
    "general_p5": (_general(5), None),
    "general_p6": (_general(6), None),
    "general_p13": (_general(13), None),
    "squeeze": (lambda rng, n: [], lambda n: []),
    # a palette on the last channel, then explicit squeezes of the other image channels (list positions 1 .. n - 1: the
    # meta channel is position 0), in place and not
    "palette_squeeze": (lambda rng, n: [_pal(rng, n - 1, 1)],
                        lambda n: [sr.params(1, 1, 1, n - 1), sr.params(0, 0, 1, n - 1)] if n > 1 else []),
}
# lists that need three channels for their RCT
NEEDS_THREE = {"rct", "rct_palette"}
WP = {"general_p6": gr.WP_A}


def lists_for(n_channels):
    return [k for k in STEP_LISTS if (n_channels >= 3 or k not in NEEDS_THREE) and (n_channels >= 2 or k != "palette_squeeze")]


def _lib_steps(steps):
    from jxl_rs_amd import lib
    return [lib.local_rct(s["begin_c"], s["rct_type"]) if s["kind"] == mr.RCT else
            lib.local_palette(s["begin_c"], s["num_c"], s["table"], s["num_deltas"], s["predictor"]) for s in steps]


def spec(name, seed, x0, y0, w, h, n_channels, with_lib=True):
    """one group of step list `name`: its coded channels, such that the channels that reach the steps are distinct
    planes (recipe_plane scaled per channel) or, where a palette reads a coded channel, index_plane"""
    rng = np.random.default_rng([seed, x0, y0, w, h, n_channels] + [ord(c) for c in name])
    make_steps, make_squeeze = STEP_LISTS[name]
    steps = make_steps(rng, n_channels)
    squeeze = make_squeeze(n_channels) if make_squeeze else None
    channels, tsteps, _ = gr.meta_apply(n_channels, steps)
    index_of = {t["buf_in"]: t for t in tsteps if t["kind"] == mr.PALETTE}
    planes = []
    for b, meta in channels:
        if meta:
            continue
        if b in index_of:
            planes.append(index_plane(rng, (h, w), index_of[b]["num_colors"], index_of[b]["num_deltas"]))
        else:
            k = len(planes)
            planes.append(sr.recipe_plane(rng, h, w) * (k + 1) + 17 * k)
    coded = sr.forward(n_channels, steps, squeeze, planes) if squeeze is not None else planes
    sp = {"name": name, "x0": x0, "y0": y0, "w": w, "h": h, "n_channels": n_channels, "ref_steps": steps, "squeeze": squeeze,
          "coded": coded, "wp": WP.get(name, gr.WP_DEFAULT), "index_planes": [p for p, (b, m) in zip(planes, [c for c in channels if not c[1]]) if b in index_of]}
    if with_lib:
        sp["steps"] = _lib_steps(steps)
    return sp


_FINISHED = {}


def finished(oracle, sp, bit_depth=8):
    """a group's finished channels by the oracle; computed once per spec object and left unchanged"""
    key = id(sp)
    if key not in _FINISHED:
        _FINISHED[key] = (sp, sr.local_apply(oracle, sp["n_channels"], sp["ref_steps"], sp["squeeze"], sp["w"], sp["h"],
                                             sp["coded"], bit_depth, sp["wp"]))
    return _FINISHED[key][1]


def touched(sp):
    """the channels of the group some step or squeeze changes; the others are their coded channels as they are"""
    n = sp["n_channels"]
    t = set()
    for s in sp["ref_steps"]:
        t |= set(range(s["begin_c"], s["begin_c"] + (3 if s["kind"] == mr.RCT else s["num_c"])))
    if sp["squeeze"] is not None:
        n_meta = sum(s["kind"] == mr.PALETTE for s in sp["ref_steps"])
        if not sp["squeeze"]:
            t |= set(range(n))
        for q in sp["squeeze"]:
            # positions behind the meta channels are image channels in list order; with one palette on the last channel
            # (the lists above) image position i is channel i
            t |= set(range(q[2] - n_meta, q[2] - n_meta + q[3]))
    return t


def grid(w, h, cell):
    return [(x, y, min(cell, w - x), min(cell, h - y)) for y in range(0, h, cell) for x in range(0, w, cell)]


# the frames of the issue: (w, h, cell)
ALIGNED = (256, 128, 128)
RAGGED = (203, 137, 64)
GREY = (200, 136, 100)
LAYOUTS = {"rgba": (3, 1), "grey_alpha": (1, 1), "grey_three": (1, 3), "extra_1": (0, 1), "extra_2": (0, 2), "extra_4": (0, 4)}


def frame_specs(name, frame, n_channels, seed=1):
    w, h, cell = frame
    return [spec(name, seed, x0, y0, gw, gh, n_channels) for x0, y0, gw, gh in grid(w, h, cell)]
