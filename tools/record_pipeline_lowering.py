#!/usr/bin/env python3
"""Records what every stage list of tests/cpp/lowering_corpus.h lowers to or is rejected with -- per family of lists, their
number, the number accepted and the SHA-256 of the lines tests/cpp/lowering_dump.cc prints for them, beside the revision
whose header was recorded -- as tests/golden/pipeline_lowering.json, which tests/test_pipeline_lowering_corpus_cpu.py
compares against exactly.  Needs no GPU, only the built libjxl_hip.so to link against.  Run it on the commit whose
behaviour is to be pinned, or from a later one with --rev: the dump program is then built against that revision's
include/ (the corpus and the program themselves are the working tree's).  Run it twice: with --check the second run
compares itself against the file instead of writing it.  --dump FILE keeps the program's whole output, e.g. to diff two
revisions line by line.

  python tools/record_pipeline_lowering.py [--rev REVISION | --include DIR] [--check] [--out FILE] [--dump FILE]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def family_digests(dump):
    """{family: {"lists", "accepted", "sha256"}} of the dump program's output: a list counts once per entry point it
    went through (one line each), a family's lines are digested in order"""
    out = {}
    for line in dump.splitlines(keepends=True):
        f = out.setdefault(line.split(" ", 1)[0], {"lists": 0, "accepted": 0, "sha256": hashlib.sha256()})
        f["lists"] += 1
        f["accepted"] += " -> ok " in line
        f["sha256"].update(line.encode())
    for f in out.values():
        f["sha256"] = f["sha256"].hexdigest()
    return out


def build_dump(include, exe):
    lib = os.path.join(ROOT, "jxl_rs_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
                    "-I", include, "-I", CPP, os.path.join(CPP, "lowering_dump.cc"), "-o", exe, "-L", lib, "-ljxl_hip",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-lpthread", "-lm"],
                   check=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rev", help="build against include/ of this git revision")
    ap.add_argument("--include", default=os.path.join(ROOT, "include"), help="build against this include directory")
    ap.add_argument("--check", action="store_true", help="compare against the file instead of writing it")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pipeline_lowering.json"))
    ap.add_argument("--dump", help="also write the dump program's output here")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        include = a.include
        if a.rev:
            tar = subprocess.run(["git", "-C", ROOT, "archive", a.rev, "include"], check=True, capture_output=True).stdout
            subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
            include = os.path.join(tmp, "include")
        exe = os.path.join(tmp, "lowering_dump")
        build_dump(include, exe)
        dump = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    if a.dump:
        with open(a.dump, "w") as f:
            f.write(dump)
    got = family_digests(dump)
    # the corpus pins acceptance and rejection alike: a family with only one of them says nothing about the other
    lopsided = [n for n, f in got.items() if not 0 < f["accepted"] < f["lists"]]
    if lopsided:
        print("families without both accepted and rejected lists:", ", ".join(lopsided))
        return 1
    total = sum(f["lists"] for f in got.values())
    if a.check:
        want = json.load(open(a.out))["families"]
        bad = [n for n in sorted(set(got) | set(want)) if got.get(n) != want.get(n)]
        for n in bad:
            print(f"{n}: recorded {want.get(n)}\n{' ' * len(n)}  now      {got.get(n)}")
        print(f"{len(got) - len(bad)} of {len(got)} families ({total} lines) reproduce {a.out}")
        return 1 if bad else 0
    with open(a.out, "w") as f:
        rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", a.rev or "HEAD"], check=True, capture_output=True, text=True)
        json.dump({"revision": rev.stdout.strip(), "families": got}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(got)} families, {total} lines -> {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
