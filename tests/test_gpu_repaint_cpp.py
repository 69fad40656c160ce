"""jxlh_frame_repaint_groups through the C++ layer on the device: tests/cpp/repaint.cc repaints the late groups of an
upsampled VarDCT frame through VarDctFrame::repaint_groups and two replaced cells of a Modular frame through
GpuModularFramePipeline::repaint_groups; the planes are, byte for byte, those of the C call on a second context, of a
third context's whole run and of the oracle, and the three ways to ask for the changed rects give one list."""
import subprocess

import pytest

from test_cpp_host import _build


@pytest.mark.gpu
@pytest.mark.parametrize("args", [("300", "600", "2", "2"), ("264", "520", "1", "4")])
def test_repaint_through_the_cpp_layer(tmp_path, args):
    exe = _build(tmp_path, "repaint")
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "repaint: ok" in r.stdout and "first pass stale" in r.stdout and "rects equal" in r.stdout
    assert r.stdout.count("repaint vs oracle: 0 differing planes, vs the C call: 0, vs a whole run: 0") == 2
