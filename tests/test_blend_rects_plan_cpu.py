"""The plan of the rectangle-list blend (jxl_rs_amd/csrc/blend_rects_plan.h) through tests/cpp/blend_rects_plan.cc: over
images of 1 x 1, 5 x 3, 517 x 11, 1030 x 9 and 70 x 130 and lists with empty, clipped, overlapping, duplicate, 1 x 1,
whole-image, odd-origin, random and 4096 rects, walking the work list the way k_blend_rects does stores exactly the
pixels of the union (every one by a lane of some piece, none outside a rect, no piece wholly outside its rect), `first`
ascends and the group count is the walk's; every refusal, the 2^31-workgroup limit to the group; the frame-to-image
mapping of jxlh_blend_image_rects against a per-pixel restatement over negative and large origins.  Host-only, no GPU."""
import os
import subprocess

from test_cpp_host import CPP, ROOT, _build


def test_blend_rects_plan(tmp_path):
    exe = _build(tmp_path, "blend_rects_plan")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "blend rects plan: ok" in r.stdout, (r.stdout + r.stderr)[-2000:]


def test_blend_rects_plan_under_sanitizers(tmp_path):
    """the same program as a stand-alone host binary with AddressSanitizer and UBSan: the plan indexes nothing out of
    bounds and overflows nowhere on the same cases"""
    exe = os.path.join(str(tmp_path), "blend_rects_plan_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "include"), os.path.join(CPP, "blend_rects_plan.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "blend rects plan: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
