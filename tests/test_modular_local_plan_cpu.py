"""The batch plan of the group-local transforms without a GPU: jxl_rs_amd/csrc/modular_local_plan.h compiled into the
stand-alone program tests/cpp/modular_local_plan.cc (plain and under sanitizers), which plans its named batches and
checks routes, launch lists, slot placement, chains and scratch, the block's layout and bytes and every refusal itself;
and its dump of the launch lists against what the GPU tests count after the fact (test_launch_accounting)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, sanitize):
    exe = os.path.join(str(tmp_path), "modular_local_plan" + ("_san" if sanitize else ""))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                "-static-libasan", "-static-libubsan"]  # the runtimes linked in: the child needs nothing from its environment
    cmd += ["-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "modular_local_plan.cc"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _dump(exe):
    """-> {batch: {"status", "first_bad", "scratch", "total", "steps": [{kernel, n_items, ...}], "block": bytes}}"""
    r = subprocess.run([exe, "dump"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:] + r.stderr)[-3000:]
    out, cur = {}, None
    for line in r.stdout.split("\n"):
        v = line.split()
        if not v:
            continue
        if v[0] == "batch":
            cur = out[v[1]] = {"status": int(v[2]), "first_bad": int(v[3]), "scratch": int(v[5]), "total": int(v[7]), "steps": []}
        elif v[0] == "step":
            st = {"kernel": v[1], "desc": (int(v[3]), int(v[4])), "items": (int(v[6]), int(v[7]))}
            st.update({v[i]: int(v[i + 1]) for i in range(8, len(v), 2)})
            cur["steps"].append(st)
        elif v[0] == "block":
            cur["block"] = bytes.fromhex(v[1]) if len(v) > 1 else b""
    return out


def _counts(batch):
    n = {}
    for st in batch["steps"]:
        n[st["kernel"]] = n.get(st["kernel"], 0) + 1
    return n


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitizers"])
def test_plan_stands_alone(tmp_path, sanitize):
    exe = _build(tmp_path, sanitize)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "modular local plan: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    d = _dump(exe)
    # the launches test_gpu_modular_local_squeeze.py::test_launch_accounting counts on the device, from the plan alone
    one, many = d["accounting_one"], d["accounting_many"]
    assert _counts(one) == _counts(many) == {"k_modular_local_squeeze_lds": 1, "k_modular_local_squeeze_level": 2}
    assert [st["kernel"] for st in one["steps"]] == [st["kernel"] for st in many["steps"]]
    assert [st["n_items"] for st in many["steps"]] == [40 * st["n_items"] for st in one["steps"]]
    assert _counts(d["accounting_deep_plain_many"]) == {"k_modular_local": 1, "k_modular_local_squeeze_lds": 1,
                                                       "k_modular_local_squeeze_level": 2, "k_modular_local_phase": 1}
    a, b = d["no_squeeze"], d["no_squeeze_general"]
    assert a["steps"] == b["steps"] and a["block"] == b["block"] and a["scratch"] == b["scratch"]
    assert "k_modular_local" in _counts(a) and not any("squeeze" in k for k in _counts(a))
    for name, batch in d.items():
        assert batch["status"] == 0 and len(batch["block"]) == batch["total"], name
        # the order of launches: the plain one, the LDS launch, the streamed levels ascending, the phases ascending
        rank = {"k_modular_local": 0, "k_modular_local_squeeze_lds": 1, "k_modular_local_squeeze_level": 2}
        keys = []
        for st in batch["steps"]:
            assert st["n_items"] > 0 and st["items"][1] == 8 * st["n_items"] and st["items"][0] % 16 == 0 and st["desc"][0] % 16 == 0
            keys.append((rank.get(st["kernel"], 3), st["step"] if st["kernel"].endswith("level") else st["items"][0]))
        assert keys == sorted(keys) and len(set(keys)) == len(keys), (name, keys)
        # alignment of the caller's pointers decides the vector path and nothing else
        if not name.endswith("_unaligned"):
            u = d[name + "_unaligned"]
            assert u["steps"] == batch["steps"] and u["total"] == batch["total"] and u["scratch"] == batch["scratch"]
