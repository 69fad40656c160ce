"""Group-local squeeze restated for the tests, line by line: default_squeeze (frame/modular/transforms/squeeze.rs:39-105),
check_squeeze_params (:17-37) and the squeeze branch of meta_apply_single_transform (meta_apply.rs:90-180) on the
channel list tests/modular_local_general_ref.py leaves behind the steps in front, and the H/VSqueeze arms of
TransformStep::local_apply (apply_local.rs:295-348: in_next_avg and out_prev are None) with the committed oracle's
unsqueeze_h / unsqueeze_v as the arithmetic.  Buffers are ids as in the reference; expected_program maps them onto what
jxlh_modular_local_lower_squeeze must report."""
import numpy as np

import modular_local_general_ref as gr
import modular_local_ref as mr
from modular_local_ref import InvalidChannelRange, Unsupported  # noqa: F401
from helpers import forward_squeeze_h, forward_squeeze_v

SQUEEZE = 3  # a tstep kind of this module only
MAX_LEVELS = 16


def params(horizontal, in_place, begin_c, num_c):
    return (int(horizontal), int(in_place), int(begin_c), int(num_c))


def default_squeeze(channels):
    """squeeze.rs:39-105; channels: dicts with meta, w, h"""
    num_meta = 0
    while num_meta < len(channels) and channels[num_meta]["meta"]:  # take_while(is_meta)
        num_meta += 1
    w, h = channels[num_meta]["w"], channels[num_meta]["h"]
    nc = len(channels) - num_meta
    out = []
    if nc > 2 and (channels[num_meta + 1]["w"], channels[num_meta + 1]["h"]) == (w, h):  # 420 previews
        if w > 1:
            out.append(params(1, 0, num_meta + 1, 2))
        if h > 1:
            out.append(params(0, 0, num_meta + 1, 2))
    MAX_FIRST_PREVIEW_SIZE = 8
    if w <= h and h > MAX_FIRST_PREVIEW_SIZE:  # vertical first on tall images
        out.append(params(0, 1, num_meta, nc))
        h = -(-h // 2)
    while w > MAX_FIRST_PREVIEW_SIZE or h > MAX_FIRST_PREVIEW_SIZE:
        if w > MAX_FIRST_PREVIEW_SIZE:
            out.append(params(1, 1, num_meta, nc))
            w = -(-w // 2)
        if h > MAX_FIRST_PREVIEW_SIZE:
            out.append(params(0, 1, num_meta, nc))
            h = -(-h // 2)
    return out


def meta_apply(n_channels, steps, squeeze, w, h):
    """-> (channels, transform_steps).  steps: the RCT / palette steps in front (mr / gr dicts); squeeze: None (the group
    has none), [] (default_squeeze) or a list of params().  channels: the list after every transform, dicts with buf,
    meta, w, h, residual; transform_steps: gr.meta_apply's, then one {"kind": SQUEEZE, horizontal, buf_in: [avg, res],
    buf_out, out_w, out_h} per squeezed channel as the reference pushes them."""
    chans, tsteps, n_buf = gr.meta_apply(n_channels, steps)
    channels = [{"buf": b, "meta": m, "w": 0 if m else w, "h": 0 if m else h, "residual": False} for b, m in chans]
    if squeeze is None:
        return channels, tsteps
    levels = {}  # buffer of a running average -> levels recorded on its chain so far
    for horizontal, in_place, begin, num in (default_squeeze(channels) if len(squeeze) == 0 else squeeze):
        end = begin + num
        if end > len(channels) or num == 0:  # check_squeeze_params, squeeze.rs:21-28 (num == 0: channels[end - 1] of nothing)
            raise InvalidChannelRange((begin, num, len(channels)))
        if any(c["meta"] for c in channels[begin:end]):
            raise Unsupported("squeeze of a meta channel")
        if any(c["residual"] for c in channels[begin:end]):
            raise Unsupported("squeeze of a residual channel")
        new_chan_offset = end if in_place else len(channels)  # meta_apply.rs:104-108
        for ic in range(num):
            chan = channels[begin + ic]
            cw, ch = chan["w"], chan["h"]
            if horizontal:  # :125-129
                s0, s1 = (-(-cw // 2), ch), (cw - -(-cw // 2), ch)
            else:
                s0, s1 = (cw, -(-ch // 2)), (cw, ch - -(-ch // 2))
            buf_0, buf_1 = n_buf, n_buf + 1  # :136, :146
            n_buf += 2
            depth = levels.pop(chan["buf"], 0) + 1
            if depth > MAX_LEVELS:
                raise Unsupported("more than 16 levels")
            levels[buf_0] = depth
            tsteps.append({"kind": SQUEEZE, "horizontal": bool(horizontal), "buf_in": [buf_0, buf_1], "buf_out": chan["buf"],
                           "out_w": cw, "out_h": ch})  # :162-174
            channels[begin + ic] = {"buf": buf_0, "meta": False, "w": s0[0], "h": s0[1], "residual": False}  # :175
            channels.insert(new_chan_offset + ic, {"buf": buf_1, "meta": False, "w": s1[0], "h": s1[1], "residual": True})  # :176
    return channels, tsteps


def coded_shapes(n_channels, steps, squeeze, w, h):
    """(h, w) of every coded channel, in list order"""
    channels, _ = meta_apply(n_channels, steps, squeeze, w, h)
    return [(c["h"], c["w"]) for c in channels if not c["meta"]]


def expected_program(n_channels, steps, squeeze, w, h):
    """what jxlh_modular_local_lower_squeeze must report: (general, n_coded, chains).  general:
    gr.expected_general_program of the steps; chains[k], for the k-th channel that reaches the squeeze: base, base_w,
    base_h and levels -- (horizontal, out_w, out_h, res) in the order the inverse runs; base and res index the coded
    channels."""
    channels, tsteps = meta_apply(n_channels, steps, squeeze, w, h)
    image = [c for c in channels if not c["meta"]]
    coded_index = {c["buf"]: j for j, c in enumerate(image)}
    size = {c["buf"]: (c["w"], c["h"]) for c in image}
    by_out = {s["buf_out"]: s for s in tsteps if s["kind"] == SQUEEZE}
    before = [b for b, m in gr.meta_apply(n_channels, steps)[0] if not m]
    chains = []
    for b in before:
        levels = []
        while b in by_out:  # from the channel down to its base: the order the steps were recorded in
            s = by_out[b]
            levels.append((int(s["horizontal"]), s["out_w"], s["out_h"], coded_index[s["buf_in"][1]]))
            b = s["buf_in"][0]
        chains.append({"base": coded_index[b], "base_w": size[b][0], "base_h": size[b][1], "levels": levels[::-1]})
    return gr.expected_general_program(n_channels, steps), len(image), chains


def local_apply(oracle, n_channels, steps, squeeze, w, h, coded, bit_depth, wp=None, trace=None):
    """the group's n_channels finished channels from its coded channels (list order): gr.local_apply with the squeeze
    arms.  trace: a list that receives (horizontal, avg, res, out) of every squeeze step, in the order they run"""
    channels, tsteps = meta_apply(n_channels, steps, squeeze, w, h)
    image = [c for c in channels if not c["meta"]]
    assert len(image) == len(coded)
    buffers = {}
    for c, a in zip(image, coded):
        a = np.ascontiguousarray(a, dtype=np.int32)
        assert a.shape == (c["h"], c["w"]), (a.shape, c)
        buffers[c["buf"]] = a
    depth = min(bit_depth, 24)
    for s in reversed(tsteps):
        if s["kind"] == SQUEEZE:
            avg, res = buffers.pop(s["buf_in"][0]), buffers.pop(s["buf_in"][1])
            if s["horizontal"]:  # do_hsqueeze_step(in_avg, in_res, None, None, out)
                buffers[s["buf_out"]] = oracle.unsqueeze_h(avg, res, s["out_w"]) if s["out_h"] else np.zeros((0, s["out_w"]), np.int32)
            else:
                buffers[s["buf_out"]] = oracle.unsqueeze_v(avg, res, s["out_h"]) if s["out_w"] else np.zeros((s["out_h"], 0), np.int32)
            if trace is not None:
                trace.append((s["horizontal"], avg, res, buffers[s["buf_out"]]))
            continue
        if s["kind"] == mr.RCT:
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


# ---- inputs
def recipe_plane(rng, h, w):
    """5 * |x % 64 - 32| + 3 * |y % 48 - 24| plus uniform noise in [-6, 6]"""
    y, x = np.mgrid[0:h, 0:w]
    return (5 * np.abs(x % 64 - 32) + 3 * np.abs(y % 48 - 24) + rng.integers(-6, 7, size=(h, w))).astype(np.int32)


def forward(n_channels, steps, squeeze, planes):
    """the coded channels whose inverse squeeze gives `planes` (the channels that reach the squeeze, in list order):
    the encoder's side of meta_apply, with tests/helpers.py's forward squeeze"""
    h, w = planes[0].shape
    channels, tsteps = meta_apply(n_channels, steps, squeeze, w, h)
    before = [b for b, m in gr.meta_apply(n_channels, steps)[0] if not m]
    buffers = {b: np.ascontiguousarray(p, dtype=np.int32) for b, p in zip(before, planes)}
    for s in tsteps:
        if s["kind"] != SQUEEZE:
            continue
        img = buffers.pop(s["buf_out"])
        avg, res = forward_squeeze_h(img) if s["horizontal"] else forward_squeeze_v(img)
        buffers[s["buf_in"][0]], buffers[s["buf_in"][1]] = avg, res
    return [buffers[c["buf"]] for c in channels if not c["meta"]]


def random_coded(rng, n_channels, steps, squeeze, w, h, lo, hi):
    """coded channels of the right shapes with random samples in [lo, hi)"""
    return [rng.integers(lo, hi, size=s, dtype=np.int64).astype(np.int32) for s in coded_shapes(n_channels, steps, squeeze, w, h)]


# the rects of the issue (w, h), default squeeze on each
RECTS = [(1, 1), (8, 8), (9, 9), (9, 8), (1, 300), (300, 1), (17, 130), (129, 127), (255, 257), (256, 256), (1024, 1024)]
# explicit lists on three channels (and one on four): not in place, one axis only, a sub-range of channels
EXPLICIT = {
    "not_in_place": (3, [params(1, 0, 0, 3), params(0, 0, 0, 3)]),
    "horizontal_only": (3, [params(1, 1, 0, 3), params(1, 1, 0, 3), params(1, 1, 0, 3)]),
    "vertical_only": (3, [params(0, 1, 0, 3), params(0, 1, 0, 3)]),
    "sub_range": (4, [params(1, 1, 1, 2), params(0, 0, 1, 1), params(1, 1, 1, 2)]),
    "mixed_places": (3, [params(0, 0, 2, 1), params(1, 1, 0, 2), params(0, 1, 0, 1), params(1, 0, 2, 1)]),
}
