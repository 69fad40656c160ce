"""Blend rectangles through the C++ layer: tests/cpp/blend_rects.cc compiles VarDctFrame::blend_rects,
jxlh::blend_image_rects and the new pipeline methods (without a device), and on a device runs
GpuRenderPipeline::do_render_rects() over two passes of a blended stage list: byte for byte the existing do_render() and
the plain C calls, the first render one whole-image rect, the second only the changed rects."""
import os
import subprocess

import pytest

from test_cpp_host import ROOT, _build


def test_cpp_members_and_pipeline_methods_compile(tmp_path):
    """no GPU needed: the program builds against the two shared libraries, and a translation unit that instantiates
    every new pipeline method compiles"""
    assert os.path.exists(_build(tmp_path, "blend_rects"))
    src = tmp_path / "methods.cc"
    src.write_text('#include "jxl_hip_pipeline.hpp"\n'
                   "using namespace jxlh;\n"
                   "std::vector<jxlh_rect> a(GpuRenderPipeline& p) { return p.do_render_rects(); }\n"
                   "std::vector<jxlh_rect> b(GpuRenderPipeline& p, const std::vector<jxlh_rect>& r) { return p.repaint_rects(r); }\n"
                   "std::vector<jxlh_rect> c(GpuModularFramePipeline& p) { return p.repaint_groups_rects({0u, 3u}); }\n"
                   "std::vector<jxlh_rect> d(const jxlh_blend_desc& x) { return blend_image_rects(x, 8, 8, {jxlh_rect{0, 0, 8, 8}}); }\n"
                   "void e(VarDctFrame& f, const jxlh_blend_desc& x) { f.blend_rects(x, {jxlh_rect{0, 0, 1, 1}}); }\n")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I",
                        os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "methods.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("args", [("600", "520", "2"), ("515", "270", "3")])
def test_do_render_rects_equals_do_render_and_the_c_calls(tmp_path, args):
    exe = _build(tmp_path, "blend_rects")
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "blend rects frame: ok" in r.stdout
    assert "do_render_rects vs do_render: equal, C calls vs do_render: equal" in r.stdout
    assert "first pass stale" in r.stdout and "one whole rect" in r.stdout and "rects equal" in r.stdout and "wrappers ok" in r.stdout
