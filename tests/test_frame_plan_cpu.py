"""The frame planner (jxl_rs_amd/csrc/frame_plan.h) through tests/cpp/frame_plan.cc: over frame sizes from 0 to beyond
2^20 on each axis and both sides of the two bounds that keep the kernels' 32-bit offsets in range, every shift triple,
the upsampling factors and upsampled sizes, zero divisors, epf_iters, the ABI version, Modular frames against
epf_sigma_for_modular and the rank count, and the quantisation biases that decide the direct entries path, the plan
equals field for field what the top of jxlh_frame_begin and modular_frame_begin computed (transcribed in the program),
and the invariants of an accepted plan hold.  Host-only, no GPU.  The same program also runs as a stand-alone binary
under the address and undefined-behaviour sanitizers."""
import os
import subprocess

from test_cpp_host import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_frame_plans(tmp_path):
    exe = _build(tmp_path, "frame_plan")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "frame plans: ok" in r.stdout, (r.stdout + r.stderr)[-2000:]


def test_frame_plans_under_sanitizers(tmp_path):
    exe = os.path.join(str(tmp_path), "frame_plan_san")
    src = os.path.join(ROOT, "tests", "cpp", "frame_plan.cc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",  # the runtimes linked in: the child needs nothing from its environment
           "-I", os.path.join(ROOT, "include"), src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "frame plans: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
