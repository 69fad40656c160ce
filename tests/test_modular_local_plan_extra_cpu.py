"""The destination table of the group-local transforms with extra channels without a GPU:
jxl_rs_amd/csrc/modular_local_plan.h compiled into the stand-alone program tests/cpp/modular_local_plan_extra.cc (plain
and under sanitizers), which checks the table of every layout, every refusal, the per-plane alignment rule and walks
100 000 random batches on the host."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, sanitize):
    exe = os.path.join(str(tmp_path), "modular_local_plan_extra" + ("_san" if sanitize else ""))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                "-static-libasan", "-static-libubsan"]  # the runtimes linked in: the child needs nothing from its environment
    cmd += ["-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "modular_local_plan_extra.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitizers"])
def test_plan_extra_stands_alone(tmp_path, sanitize):
    exe = _build(tmp_path, sanitize)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "modular local plan extra: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
