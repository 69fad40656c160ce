"""The builder layer held to the C calls on the device: tests/cpp/save_frame.cc runs one synthetic frame with an alpha
channel through GpuRenderPipeline with a stage list that ends in premultiply + U8 conversions + an RGBA save in
orientation 6 (and a second buffer with the alpha alone), and through jxlh_frame_run + jxlh_frame_save in bands; both
results are bit-identical."""
import subprocess

import pytest

from test_cpp_host import _build


@pytest.mark.gpu
@pytest.mark.parametrize("args", [("300", "270", "2"), ("515", "133", "3")])
def test_builder_save_equals_c_calls(tmp_path, args):
    exe = _build(tmp_path, "save_frame")
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "builder vs C calls: 0 differing rows" in r.stdout and "save frame: ok" in r.stdout
