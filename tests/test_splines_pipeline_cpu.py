"""SplinesStage in the C++ mirror of the reference's RenderPipelineBuilder (include/jxl_hip_lowering.hpp): where a
stage list may hold it and what it lowers to, through tests/cpp/splines_lowering.cc.  Host-only, no GPU."""
import subprocess

from test_cpp_host import _build


def test_splines_stage_lowering(tmp_path):
    exe = _build(tmp_path, "splines_lowering")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "splines lowering: ok" in r.stdout, (r.stdout + r.stderr)[-2000:]
