"""The plan of the rectangle-list save (jxl_rs_amd/csrc/save_rects_plan.h) through tests/cpp/save_rects_plan.cc: over
all 8 orientations, pixels of 1 to 16 bytes, results of 1 x 1, 5 x 3, 1030 x 9 and 70 x 130 and lists with empty,
clipped, overlapping, duplicate, 1 x 1, whole-image, odd-origin and 4096 rects, walking the work list the way the
kernels do and copying the staged blocks out the way the host does leaves exactly the bytes a per-pixel membership scan
with a per-pixel display_pixel asks for; every refusal; the geometry of jxlh_changed_rects.  Host-only, no GPU."""
import os
import subprocess

from test_cpp_host import CPP, ROOT, _build


def test_save_rects_plan(tmp_path):
    exe = _build(tmp_path, "save_rects_plan")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "save rects plan: ok" in r.stdout, (r.stdout + r.stderr)[-2000:]


def test_save_rects_plan_under_sanitizers(tmp_path):
    """the same program as a stand-alone host binary with AddressSanitizer and UBSan: the plan indexes nothing out of
    bounds and overflows nowhere on the same cases"""
    exe = os.path.join(str(tmp_path), "save_rects_plan_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "include"), os.path.join(CPP, "save_rects_plan.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "save rects plan: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
