"""What the reference runs for the steps of a squeezed channel whose residual channels have partly not arrived, for
whole channels (ModularGridKind::None): a restatement of the bookkeeping in modular/transforms/meta_apply.rs:150-161
(which step gets a `buf_in_avg`) and transforms/step.rs:138-150 (SqueezeInfo::new: the kind from the two residual
buffers' DataStatus), kept apart from the library's planner; and preview_reference, which runs EVERY level the way the
reference does (dead ones included) through the oracle's step functions.

Levels are in the decoder's order throughout (smallest first), as in jxlh_squeeze_level lists."""
import numpy as np

REGULAR, SMOOTH_1D, SMOOTH_2D = 0, 1, 2
H, V, D2 = 0, 1, 2   # the oracle's smooth kinds


def has_res(horizontal, out_w, out_h):
    return (out_w // 2) * out_h > 0 if horizontal else out_w * (out_h // 2) > 0


def reference_steps(horizontal):
    """meta_apply.rs:100-178 for one channel: the transform names the squeezes finest first; each pushes a step whose
    inputs are two new buffers and whose output is the channel's current buffer.  -> steps in the order pushed, each
    {level, horizontal, buf_in: (avg, res), buf_out, buf_in_avg}; buffer 0 is the image channel."""
    n = len(horizontal)
    transform_steps, transform_step_for_buf = [], {}
    channel_buf, next_buf = 0, 1
    for level in reversed(range(n)):            # the decoder's last level is the transform's first squeeze
        hz = bool(horizontal[level])
        buf_0, buf_1 = next_buf, next_buf + 1   # add_transform_buffer: "Squeezed channel", "Squeeze residual"
        next_buf += 2
        transform_step_for_buf[buf_0] = (len(transform_steps), hz)          # :150
        buf_out = channel_buf                                              # :151
        t = transform_step_for_buf.get(buf_out)                            # :152
        if t is not None and t[1] != hz:                                   # :153
            transform_steps[t[0]]["buf_in_avg"] = (buf_0, buf_1)           # :155-160
        transform_steps.append({"level": level, "horizontal": hz, "buf_in": (buf_0, buf_1), "buf_out": buf_out,
                                "buf_in_avg": None})                       # :162-174
        channel_buf = buf_0                                                # :175
    return transform_steps


def preview_kinds_ref(horizontal, zero):
    """zero[level]: the level's residual buffer is DataStatus::Zero (not arrived).  -> (kinds, source, live): source[L]
    is the level whose OUTPUT level L reads as its average (-1: the base planes); live[L]: the last level's output
    depends on level L's."""
    n = len(horizontal)
    steps = reference_steps(horizontal)
    res_zero = {s["buf_in"][1]: bool(zero[s["level"]]) for s in steps}
    # a buffer is the output of the step that names it as buf_out; the last pushed step's average is the base
    producer = {s["buf_out"]: s["level"] for s in steps}
    avg_of_level = {s["buf_in"][0]: s["level"] - 1 for s in steps}
    assert all(producer.get(b, -1) == lv for b, lv in avg_of_level.items())
    kinds, source = [None] * n, [None] * n
    for s in steps:
        buf_in, buf_in_avg = s["buf_in"], s["buf_in_avg"]
        if not res_zero[buf_in[1]]:                          # step.rs:138
            kind, src = REGULAR, buf_in[0]
        elif buf_in_avg is not None:                         # :140
            avg2_buf, res2_buf = buf_in_avg
            if res_zero[res2_buf]:                           # :143
                kind, src = SMOOTH_2D, avg2_buf              # :144
            else:
                kind, src = SMOOTH_1D, buf_in[0]             # :146
        else:
            kind, src = SMOOTH_1D, buf_in[0]                 # :149
        kinds[s["level"]], source[s["level"]] = kind, avg_of_level[src]
    live = [False] * n
    todo = [n - 1] if n else []
    while todo:
        lv = todo.pop()
        if lv >= 0 and not live[lv]:
            live[lv] = True
            todo.append(source[lv])
    return kinds, source, live


def missing_flags(steps, missing):
    """a level that has no residual samples cannot be missing: it is regular whatever its pointers are"""
    return [bool(m) and has_res(hz, ow, oh) for (hz, ow, oh), m in zip(steps, missing)]


def forward_chain(planes, steps):
    """planes: the image's channels; steps: decoder-order [(horizontal, out_w, out_h)].  Squeezes finest first with
    helpers.forward_squeeze_h / _v -> (base planes, residuals[level][channel])"""
    from helpers import forward_squeeze_h, forward_squeeze_v
    cur = [np.ascontiguousarray(p, dtype=np.int32) for p in planes]
    residuals = [None] * len(steps)
    for level in reversed(range(len(steps))):
        hz, ow, oh = steps[level]
        assert cur[0].shape == (oh, ow)
        pairs = [forward_squeeze_h(p) if hz else forward_squeeze_v(p) for p in cur]
        cur = [a for a, _ in pairs]
        residuals[level] = [r for _, r in pairs]
    return cur, residuals


def explicit_steps(w, h, horizontal):
    """decoder-order steps of a w x h channel squeezed along the given decoder-order directions"""
    sizes, cw, ch = [], w, h
    for hz in reversed(horizontal):
        sizes.append((bool(hz), cw, ch))
        cw, ch = ((cw + 1) // 2, ch) if hz else (cw, (ch + 1) // 2)
    return list(reversed(sizes)), (cw, ch)


def preview_reference(oracle, base, residuals, steps, missing, rct=None, cvt_rne=False):
    """every level, dead ones included, the way the reference's step list runs: regular steps with the residuals,
    smooth steps from the buffer SqueezeInfo::new names; then the RCT.  -> final planes"""
    zero = missing_flags(steps, missing)
    kinds, source, _ = preview_kinds_ref([hz for hz, _, _ in steps], zero)
    nch = len(base)
    outputs = {-1: [np.ascontiguousarray(b, dtype=np.int32) for b in base]}
    for level, (hz, ow, oh) in enumerate(steps):
        src = outputs[source[level]]
        if kinds[level] == REGULAR:
            res = residuals[level]
            outputs[level] = [oracle.unsqueeze_h(src[c], res[c], ow) if hz else oracle.unsqueeze_v(src[c], res[c], oh)
                              for c in range(nch)]
        else:
            kind = D2 if kinds[level] == SMOOTH_2D else H if hz else V
            outputs[level] = [oracle.smooth_unsqueeze(kind, src[c], ow, oh, cvt_rne=cvt_rne) for c in range(nch)]
    final = outputs[len(steps) - 1]
    return oracle.rct(final, *rct) if rct is not None else final
