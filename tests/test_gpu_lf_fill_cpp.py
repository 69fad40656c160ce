"""The C++ layers of the LF fill held to the C calls: tests/cpp/lf_fill.cc runs the streaming sequence (every group
marked and painted from the LF, two groups arrive, the rest arrive) through the plain C calls, through
VarDctFrame::upsample_lf_groups and through GpuRenderPipeline::set_lf_only_group; the three agree bit for bit at every
step and end at the oracle's frame."""
import subprocess

import pytest

from test_cpp_host import _build


def test_lf_fill_program_compiles_and_links(tmp_path):
    """no GPU needed: the new wrappers build against the library"""
    import os
    assert os.path.exists(_build(tmp_path, "lf_fill"))


@pytest.mark.gpu
@pytest.mark.parametrize("args", [("520", "300", "2"), ("300", "520", "0")])
def test_streaming_sequence_through_the_cpp_layers(tmp_path, args):
    exe = _build(tmp_path, "lf_fill")
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "first paint: 0 differing rows; two groups: 0; all groups: 0; final vs oracle: 0;" in r.stdout
    assert "lf fill: ok" in r.stdout
