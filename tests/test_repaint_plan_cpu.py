"""The repaint planner (jxl_rs_amd/csrc/repaint_plan.h) through tests/cpp/repaint_plan.cc: over sizes around the 256
grid, every stage list, VarDCT / Modular, upsampling 1 / 2 / 4 / 8, noise, draws_in_place, chroma subsampling and random
group lists the plan equals plan_rerender's / plan_run's where it is built on them, its centre and noise rows are the
rule's, and the changed rects are disjoint, inside the result and exactly the widened cells.  Host-only, no GPU."""
import subprocess

from test_cpp_host import _build


def test_repaint_plans(tmp_path):
    exe = _build(tmp_path, "repaint_plan")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "repaint plans: ok" in r.stdout, (r.stdout + r.stderr)[-2000:]
