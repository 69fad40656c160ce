"""The repaint through the C++ layer on the device: tests/cpp/save_rects_frame.cc renders a synthetic frame through
GpuRenderPipeline in two passes, saves the first pass whole (opaque RGBA8, orientation 6), and after the second pass
repaints only GpuRenderPipeline::changed_rects' rectangles with save_rects; the buffer is then, row for row, the oracle's
frame through the oracle's output stage -- also through jxlh::changed_rects, VarDctFrame::save_rects_async and the C
call."""
import subprocess

import pytest

from test_cpp_host import _build


@pytest.mark.gpu
@pytest.mark.parametrize("args", [("600", "520", "2"), ("515", "270", "3")])
def test_repaint_through_the_builder_equals_the_oracle(tmp_path, args):
    exe = _build(tmp_path, "save_rects_frame")
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "repaint vs oracle: 0 differing rows, wrappers: 0 differing rows" in r.stdout and "save rects frame: ok" in r.stdout
    assert "first pass stale" in r.stdout and "rects equal" in r.stdout and "error path ok" in r.stdout
