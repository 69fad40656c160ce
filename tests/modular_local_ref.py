"""Group-local Modular transforms restated for the tests: the channel-list bookkeeping of meta_apply_single_transform
(frame/modular/transforms/meta_apply.rs:49-230) as meta_apply_local_transforms drives it (apply_local.rs:69-104), and
TransformStep::local_apply (apply_local.rs:233-294) with the committed oracle's RCT and palette as the arithmetic.
Buffers are ids as in the reference; slot_of maps them onto the channel slots jxlh_modular_local_lower reports."""
import numpy as np

RCT, PALETTE = 0, 1
# do_rct_step's permutations, rct.rs:132-156: "out[PERM_OUT[p]] = in[0, 1, 2]"
PERM_OUT = [(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (1, 0, 2), (2, 1, 0)]


class InvalidChannelRange(Exception):
    """Error::InvalidChannelRange, meta_apply.rs:31-37"""


class Unsupported(Exception):
    """what the device path leaves on the host"""


def rct(begin_c, rct_type):
    return {"kind": RCT, "begin_c": begin_c, "rct_type": rct_type}


def palette(begin_c, num_c, table, num_deltas=0, predictor=0):
    t = np.ascontiguousarray(table, dtype=np.int32).reshape(num_c, -1)
    return {"kind": PALETTE, "begin_c": begin_c, "num_c": num_c, "table": t, "num_colors": t.shape[1] - num_deltas,
            "num_deltas": num_deltas, "predictor": predictor}


def meta_apply(n_channels, steps):
    """-> (channels, transform_steps, n_buffers).  channels: the list after every transform, (buffer id, is_meta);
    transform_steps: dicts with buf_in / buf_out (/ buf_pal) as the reference's TransformStep holds them."""
    channels = [(i, False) for i in range(n_channels)]  # apply_local.rs:77-81: buffer i = channel i
    n_buf = n_channels
    out = []
    for t in steps:
        b = t["begin_c"]
        if t["kind"] == RCT:
            if b + 3 > len(channels):  # check_equal_channels, meta_apply.rs:31
                raise InvalidChannelRange((b, b + 3, len(channels)))
            if any(m for _, m in channels[b:b + 3]):  # (sizes differ: MixingDifferentChannels in the reference)
                raise Unsupported("RCT on a meta channel")
            buf_out = [channels[b + i][0] for i in range(3)]  # :64-68
            buf_in = []
            for i in range(3):  # :69-81: each channel gets a fresh buffer
                channels[b + i] = (n_buf, False)
                buf_in.append(n_buf)
                n_buf += 1
            out.append({"kind": RCT, "buf_in": buf_in, "buf_out": buf_out, "op": t["rct_type"] % 7, "perm": t["rct_type"] // 7})  # :59-61
        elif t["kind"] == PALETTE:
            n = t["num_c"]
            if b + n > len(channels):  # :188
                raise InvalidChannelRange((b, b + n, len(channels)))
            if any(m for _, m in channels[b:b + n]):
                raise Unsupported("palette of a meta channel")
            pchan, inchan = n_buf, n_buf + 1  # :198, :207
            n_buf += 2
            out.append({"kind": PALETTE, "buf_in": inchan, "buf_pal": pchan, "buf_out": [c[0] for c in channels[b:b + n]],  # :214-225
                        "num_colors": t["num_colors"], "table": t["table"]})
            del channels[b + 1:b + n]       # :226
            channels[b] = (inchan, False)   # :227
            channels.insert(0, (pchan, True))  # :228
        else:
            raise Unsupported("squeeze")
    return channels, out, n_buf


def expected_program(n_channels, steps):
    """what jxlh_modular_local_lower must report: n_coded, coded_slot, and per inverse step (last first) the kind, the
    RCT op, the slots read and the slots written"""
    channels, tsteps, _ = meta_apply(n_channels, steps)
    slot_of = {i: i for i in range(n_channels)}
    for s in tsteps:
        if s["kind"] == RCT:
            for k in range(3):
                slot_of[s["buf_in"][k]] = slot_of[s["buf_out"][k]]
        else:
            slot_of[s["buf_in"]] = slot_of[s["buf_out"][0]]
    coded = [slot_of[b] for b, meta in channels if not meta]
    ops = []
    for s in reversed(tsteps):  # apply_local.rs: the steps run last to first
        if s["kind"] == RCT:
            reads = [slot_of[b] for b in s["buf_in"]]
            # bufs[k] of do_rct_step ends up as buffers[buf_out[k]] (apply_local.rs:256-258); w_j lands in bufs[PERM_OUT[j]]
            writes = [slot_of[s["buf_out"][PERM_OUT[s["perm"]][j]]] for j in range(3)]
            ops.append((RCT, s["op"], reads, writes))
        else:
            ops.append((PALETTE, 0, [slot_of[s["buf_in"]]], [slot_of[b] for b in s["buf_out"]]))
    return len(coded), coded, ops


def local_apply(oracle, n_channels, steps, coded, bit_depth):
    """the group's n_channels finished channels from its coded channels (list order), by the oracle's transforms"""
    channels, tsteps, _ = meta_apply(n_channels, steps)
    image = [b for b, meta in channels if not meta]
    assert len(image) == len(coded)
    buffers = {b: np.ascontiguousarray(c, dtype=np.int32) for b, c in zip(image, coded)}
    for s in reversed(tsteps):
        if s["kind"] == RCT:
            res = oracle.rct([buffers.pop(b) for b in s["buf_in"]], s["op"], s["perm"])  # do_rct_step, in place
            for b, r in zip(s["buf_out"], res):
                buffers[b] = r
        else:
            res = oracle.palette(buffers.pop(s["buf_in"]), s["table"], s["num_colors"], len(s["buf_out"]), min(bit_depth, 24))
            for b, r in zip(s["buf_out"], res):
                buffers[b] = r
    return [buffers[c] for c in range(n_channels)]


def coded_for_test(n_channels, steps, shape, rng, lo, hi):
    """coded channels of the right count and shape for `steps`: random samples in [lo, hi) (a palette's index channel
    too: every i32 is a valid index)"""
    channels, _, _ = meta_apply(n_channels, steps)
    return [rng.integers(lo, hi, size=shape, dtype=np.int64).astype(np.int32) for _, meta in channels if not meta]


def small_palette(n_c, n_colors=6):
    """n_c rows of n_colors distinct entries"""
    return np.arange(n_c * n_colors, dtype=np.int32).reshape(n_c, n_colors)


# (n_channels, steps): the lists of the issue, in its order
LISTS = {
    "none": (3, []),
    "rct": (3, [rct(0, 17)]),
    "rct_rct": (3, [rct(0, 6), rct(0, 29)]),
    "palette_0_3": (3, [palette(0, 3, small_palette(3))]),
    "palette_0_4": (4, [palette(0, 4, small_palette(4))]),
    "palette_1_1": (3, [palette(1, 1, small_palette(1))]),
    "rct_palette_0_3": (3, [rct(0, 40), palette(0, 3, small_palette(3))]),
    "palette_2_1_rct_1": (3, [palette(2, 1, small_palette(1)), rct(1, 10)]),
    "grey_palette_0_1": (1, [palette(0, 1, small_palette(1))]),
}
