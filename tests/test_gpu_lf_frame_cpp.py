"""The C++ layer of LF frames held to the C calls: tests/cpp/lf_frame.cc compiles every new member of include/jxl_hip.hpp
and GpuFramePipeline::save_lf; on the device it runs a Modular XYB LF frame through RenderPipelineBuilder::
build_modular_frame, saves it into an LF slot and previews the slot, and the image is byte-compared with the one this
side makes from the same samples through the C ABI (ctypes)."""
import subprocess

import numpy as np
import pytest

import lf_preview_ref as lp
from test_cpp_host import _build

IW, IH = 70, 37  # slot 9 x 5


def test_lf_frame_program_compiles_and_links(tmp_path):
    """no GPU needed: the new wrappers and the pipeline's forwarder build against the library"""
    import os
    assert os.path.exists(_build(tmp_path, "lf_frame"))


@pytest.mark.gpu
def test_pipeline_save_lf_and_preview_equal_c_calls(tmp_path):
    import jxl_rs_amd
    from jxl_rs_amd import lib
    sw, sh = lp.slot_size(IW, IH)
    chans = lp.modular_xyb(np.random.default_rng(2028), sw, sh)
    xyb = np.float32([1.0 if i % 4 == 0 else 0.01 * i for i in range(9)] + [0.1] * 3 + [0.001] * 3 + [1.0])
    ctx = jxl_rs_amd.Context(0, 1)
    try:
        lp.render_modular_xyb(ctx, chans)
        ctx.save_lf(0)
        want = ctx.lf_preview(0, IW, IH, lib.save_desc([0, 1, 2], lib.SAVE_U8, fill_opaque_alpha=True),
                              ctx.output_desc(lib.COLOR_XYB, "srgb", xyb))
        ctx.clear_lf_frame(0)
    finally:
        ctx.close()
    assert want.shape == (IH, IW * 4) and len(np.unique(want)) > 32
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.int32([IW, IH]).tobytes() + xyb.tobytes() + np.float32(lp.XYB_FACTORS).tobytes())
        for a in chans:
            f.write(np.ascontiguousarray(a).tobytes())
    (tmp_path / "want.bin").write_bytes(want.tobytes())
    exe = _build(tmp_path, "lf_frame")
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "want.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "pipeline save_lf + lf_preview vs ctypes: 0 differing bytes" in r.stdout and "lf frame: ok" in r.stdout
