"""BlendingStage and ExtendToImageDimensionsStage in the C++ mirror of the reference's RenderPipelineBuilder
(include/jxl_hip_lowering.hpp): where a stage list may hold them and what they lower to, through
tests/cpp/blending_lowering.cc.  Host-only, no GPU."""
import subprocess

from test_cpp_host import _build


def test_blending_stage_lowering(tmp_path):
    exe = _build(tmp_path, "blending_lowering")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "blending lowering: ok" in r.stdout, (r.stdout + r.stderr)[-2000:]
