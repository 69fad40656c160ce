#!/usr/bin/env python3
"""Records what every case of tests/run_plan_cases.py enqueues and leaves in the planes -- timer scope names with launch
counts, SHA-256 of read_planes() -- as tests/golden/run_plan_launches.json, which tests/test_gpu_run_plan.py compares
against exactly.  Run it on the commit whose behaviour is to be pinned (an MI355X), twice: with --check the second run
compares itself against the file instead of writing it, and names every case that does not reproduce.

  python tools/record_run_launches.py [--check] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare against the file instead of writing it")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "run_plan_launches.json"))
    a = ap.parse_args()
    import jxl_rs_amd
    from run_plan_cases import CASES, run_case
    ctx = jxl_rs_amd.Context(0, 1)
    got = {c["name"]: run_case(ctx, c) for c in CASES}
    ctx.close()
    if a.check:
        want = json.load(open(a.out))
        bad = [n for n in got if got[n] != want.get(n)]
        for n in bad:
            print(f"{n}: recorded {want.get(n)}\n{' ' * len(n)}  now      {got[n]}")
        print(f"{len(got) - len(bad)} of {len(got)} cases reproduce {a.out}")
        return 1 if bad or set(want) != set(got) else 0
    with open(a.out, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(got)} cases -> {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
