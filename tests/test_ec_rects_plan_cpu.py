"""The host plan of the extra channels' rect form (jxl_rs_amd/csrc/ec_rects_plan.h) through tests/cpp/ec_rects_plan.cc:
over more than 100 000 random channel sizes (1, and both sides of every tile and piece seam), factors and rect lists
(1 x 1, on the edges, overlapping, empty), the dirty tiles, the item list of a run, the scatter layout walked the way
the kernel walks it and the changed-rects rule against a brute-force per-sample model; every argument error with its
status and first_bad, at the wrap of 32 and 64 bits too.  Host-only, no GPU."""
import os
import subprocess

from test_cpp_host import CPP, ROOT


def _compile(tmp_path, name, flags):
    exe = os.path.join(str(tmp_path), name)
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "include"),
           os.path.join(CPP, "ec_rects_plan.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_ec_rects_plan(tmp_path):
    """plain C++ with the public headers alone: no HIP, no library"""
    exe = _compile(tmp_path, "ec_rects_plan", ["-O2"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ec rects plan: ok" in r.stdout, (r.stdout + r.stderr)[-2000:]


def test_ec_rects_plan_under_sanitizers(tmp_path):
    """the same program as a stand-alone host binary with AddressSanitizer and UBSan: the plan indexes nothing out of
    bounds and overflows nowhere on the same cases"""
    exe = _compile(tmp_path, "ec_rects_plan_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ec rects plan: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
