"""The C++ layers held to the C calls on the device: tests/cpp/splines_frame.cc runs one synthetic frame with the
reference's consistency-test spline through VarDctFrame::decode_splines, through GpuRenderPipeline with a stage list that
holds SplinesStage, and through jxlh_stage_splines on the plain frame's planes; the three results are bit-identical."""
import subprocess

import pytest

from test_cpp_host import _build


@pytest.mark.gpu
@pytest.mark.parametrize("args", [("300", "270", "2"), ("515", "133", "0")])
def test_decode_splines_and_builder_equal_c_calls(tmp_path, args):
    exe = _build(tmp_path, "splines_frame")
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "decode_splines vs stage hook: 0 differing rows; builder vs decode_splines: 0 differing rows" in r.stdout
    assert "splines frame: ok" in r.stdout
