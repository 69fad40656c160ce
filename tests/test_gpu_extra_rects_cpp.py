"""Extra channels by rect through the C++ layer on the device: tests/cpp/extra_rects.cc declares two extra channels
(factor 2 and factor 1) of a 264 x 200 frame through GpuFramePipeline, feeds them rect by rect, renders, replaces a
rect of each and re-renders a group; the finished channels it writes out are, byte for byte, those of the ctypes route
fed the same samples -- and the oracle's."""
import subprocess

import numpy as np
import pytest

from helpers import bit_equal, upload_frame
from test_cpp_host import _build

W, H = 264, 200


def _lcg_planes():
    """the program's samples: one LCG stream, alpha (8 bits, half resolution) then depth (16 bits)"""
    aw, ah = (W + 1) // 2, (H + 1) // 2
    n = aw * ah + W * H
    state, vals = 12345, np.empty(n, dtype=np.uint32)
    for i in range(n):
        state = (state * 1664525 + 1013904223) & 0xffffffff
        vals[i] = state
    alpha = (vals[:aw * ah] >> 24).astype(np.int32).reshape(ah, aw)
    depth = (vals[aw * ah:] >> 16).astype(np.int32).reshape(H, W)
    for p in (alpha, depth):
        p[13:20, 60:69] ^= 0x55  # the program's update
    return alpha, depth


@pytest.mark.gpu
def test_pipeline_route_equals_the_ctypes_route(tmp_path, oracle):
    import jxl_rs_amd
    from jxl_rs_amd import synth
    exe = _build(tmp_path, "extra_rects")
    out = str(tmp_path / "channels.f32")
    r = subprocess.run([exe, str(W), str(H), out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "rects equal, not-rendered read refused, second begin refused" in r.stdout and "extra rects: ok" in r.stdout
    got = np.fromfile(out, dtype=np.float32).reshape(2, H, W)
    alpha, depth = _lcg_planes()
    ctx = jxl_rs_amd.Context(0, 1)
    try:
        upload_frame(ctx, synth.make_vardct(W, H, mix=synth.MIX_DCT8, seed=1, epf_iters=1))
        ctx.begin_extra_channel(0, alpha.shape[1], alpha.shape[0], 8, 2)
        ctx.begin_extra_channel(1, W, H, 16, 1)
        ctx.set_extra_channel_rects([(0, 0, 0, alpha[:40]), (0, 0, 40, alpha[40:]), (1, 0, 0, depth[:, :100]), (1, 100, 0, depth[:, 100:])])
        ctx.frame_run()
        ctx.sync()
        for ec, (plane, bits, up) in enumerate(((alpha, 8, 2), (depth, 16, 1))):
            mine = ctx.read_extra_channel(ec, W, H)
            assert bit_equal(got[ec], mine), ec
            f = oracle.modular_to_f32(plane, bits)
            assert bit_equal(mine, oracle.upsample(up, f)[:H, :W] if up > 1 else f), ec
    finally:
        ctx.close()
