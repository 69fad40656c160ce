"""The coefficient-epoch planner (jxl_rs_amd/csrc/coeff_epoch.h) through tests/cpp/coeff_epoch_plan.cc: for a table of
submission histories, the resident form after the run, the routes, the groups rebuilt from the old resident form or
widened into pair words, the descriptors uploaded, the sort and the density hint.  Host-only, no GPU."""
import subprocess

from test_cpp_host import _build


def test_coeff_epoch_plans(tmp_path):
    exe = _build(tmp_path, "coeff_epoch_plan")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "coeff epoch plans: ok" in r.stdout, (r.stdout + r.stderr)[-2000:]
