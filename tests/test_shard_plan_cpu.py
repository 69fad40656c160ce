"""The shard plan without a GPU: jxl_rs_amd/csrc/shard_plan.h compiled into the stand-alone program
tests/cpp/shard_plan.cc (plain and under sanitizers), which plans every rank of every world of 1..8 ranks over 1..9 group
rows and checks itself that each plan equals the index arithmetic comm.hip carried inline, that the ranks' sends pair
with their neighbours' receives, that the exchange and both forms of the gather move the right rows of a model frame,
and that everything stays inside what the frame plan sized; and its dump of the bands against jxl_rs_amd.shard, the
Python mirror test_sharding.py and the hosts that distribute coefficient groups rely on."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, sanitize):
    exe = os.path.join(str(tmp_path), "shard_plan" + ("_san" if sanitize else ""))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                "-static-libasan", "-static-libubsan"]  # the runtimes linked in: the child needs nothing from its environment
    cmd += ["-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shard_plan.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitizers"])
def test_plan_stands_alone(tmp_path, sanitize):
    exe = _build(tmp_path, sanitize)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "shard plan: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_python_mirror_cuts_the_same_bands(tmp_path):
    from jxl_rs_amd.shard import band_for_rank, band_pixel_rows
    r = subprocess.run([_build(tmp_path, False), "dump"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:] + r.stderr)[-3000:]
    seen = set()
    for line in r.stdout.split("\n"):
        v = line.split()
        if not v:
            continue
        assert v[0] == "band" and len(v) == 10, line
        ygroups, nranks, ysize, rank, r0, r1, y0, y1, per = map(int, v[1:])
        assert band_for_rank(ygroups, rank, nranks) == (r0, r1, per), line
        assert band_pixel_rows(r0, r1, ysize) == (y0, y1), line
        seen.add((ygroups, nranks, ysize, rank))
    want = {(yg, n, ys, rank) for yg in range(1, 10) for n in range(1, 9) for ys in ((yg - 1) * 256 + 100, yg * 256)
            for rank in range(n)}
    assert seen == want
