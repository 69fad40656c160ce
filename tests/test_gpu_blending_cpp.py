"""The builder layer held to the C calls on the device: tests/cpp/blending_frame.cc runs one synthetic frame through
GpuRenderPipeline with a stage list that holds BlendingStage + the extend stage, and through jxlh_frame_run +
jxlh_frame_blend; both results are image-sized and bit-identical."""
import subprocess

import pytest

from test_cpp_host import _build


@pytest.mark.gpu
@pytest.mark.parametrize("args", [("300", "270", "2"), ("515", "133", "3")])
def test_builder_blend_equals_c_calls(tmp_path, args):
    exe = _build(tmp_path, "blending_frame")
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "builder vs C calls: 0 differing rows" in r.stdout and "blending frame: ok" in r.stdout
