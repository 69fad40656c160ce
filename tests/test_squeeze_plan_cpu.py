"""The squeeze chain's planner (jxl_rs_amd/csrc/squeeze_plan.h) through tests/cpp/squeeze_plan.cc: over final sizes with
their default chains, plane counts, an RCT or none, strides, plane addresses, both environment switches and spans next to
2^30 and 2^31 samples, the plan equals what the expressions it replaced gave (transcribed in the program, one function
per place they stood), and the invariants of a plan hold.  Host-only, no GPU."""
import subprocess

from test_cpp_host import _build


def test_squeeze_plans(tmp_path):
    exe = _build(tmp_path, "squeeze_plan")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "squeeze plans: ok" in r.stdout, (r.stdout + r.stderr)[-2000:]
