"""K1's launch planner (jxl_rs_amd/csrc/k1_plan.h) through tests/cpp/k1_plan.cc: over every coefficient form, 4:4:4 and
sub-sampled frames, the density hints, the three environment overrides, special / large varblocks, routed groups, a dense
slab or none, the strip flag, listed groups and row ranges, and group counts from 1 to beyond every grid cap, the plan
equals step for step what the decision code it replaced gave (launch_vardct_groups and launch_vardct_large, transcribed
in the program), and the invariants of a plan hold.  Host-only, no GPU."""
import subprocess

from test_cpp_host import _build


def test_k1_plans(tmp_path):
    exe = _build(tmp_path, "k1_plan")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "k1 plans: ok" in r.stdout, (r.stdout + r.stderr)[-2000:]
