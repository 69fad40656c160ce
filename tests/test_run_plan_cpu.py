"""The frame run's planner (jxl_rs_amd/csrc/run_plan.h) through tests/cpp/run_plan.cc: over every stage list, frame
kind, flag, band and set of re-rendered group rows, the plan equals what the expressions it replaced gave (transcribed
in the program, one function per place they stood), and the invariants that tie those places together hold.  Host-only,
no GPU."""
import subprocess

from test_cpp_host import _build


def test_run_plans(tmp_path):
    exe = _build(tmp_path, "run_plan")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "run plans: ok" in r.stdout, (r.stdout + r.stderr)[-2000:]
