"""The save tail in the C++ mirror of the reference's RenderPipelineBuilder (include/jxl_hip_lowering.hpp): the RGBA,
gray + alpha, BGRA-premultiplied, spot-colour, f16-with-clamp, 10-bit-u16 and several-buffer lists of frame/render.rs
lower to the expected jxlh_save_desc entries, lists out of the reference's order fail naming the stage, and lists without
these stages lower to what they did -- through tests/cpp/save_lowering.cc.  Host-only, no GPU."""
import subprocess

from test_cpp_host import _build


def test_save_stage_lowering(tmp_path):
    exe = _build(tmp_path, "save_lowering")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "save lowering: ok" in r.stdout, (r.stdout + r.stderr)[-2000:]
