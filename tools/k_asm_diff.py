#!/usr/bin/env python3
"""Compare the kernels of device-only assembly files (hipcc ... --cuda-device-only -S) kernel by kernel.

    tools/k_asm_diff.py --old a.s [b.s ...] --new c.s [d.s ...]

A kernel is everything from its entry label to the end of its `; Kernel info` block: the instructions, the
.amdhsa_ descriptor (VGPRs, SGPRs, scratch, LDS) and the spill / occupancy figures.  Only what depends on the
kernel's position in its file is normalised: the function number in local labels (.LBB<n>_, .Lfunc_end<n>, .Ltmp<n>)
and in the comments that name them, and the column the comments start in.
Prints one line per kernel and exits 1 unless both sides hold the same kernels with identical text."""
import argparse
import re
import subprocess
import sys


def kernels(path):
    lines = open(path).read().split("\n")
    names = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m]
    out = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = start
        while not lines[end].startswith("; Kernel info"):
            end += 1
        while lines[end].startswith(";"):
            end += 1
        text = "\n".join(lines[start:end])
        text = re.sub(r"(\.L|\b)BB\d+_", r"\1BB_", text)  # labels and the loop comments that name them
        text = re.sub(r"\.L(func_end|func_begin|tmp)\d+", r".L\1", text)
        text = re.sub(r" +;", " ;", text)  # comment columns move with the label's length
        out[name] = text
    return out


def figures(text):
    def f(pat):
        m = re.search(pat, text)
        return m.group(1) if m else "?"
    n_ins = sum(1 for l in text.split("\n") if l.startswith("\t") and not l.startswith("\t.") and not l.startswith("\t;"))
    return (n_ins, f(r"; NumVgprs: (\d+)"), f(r"; TotalNumSgprs: (\d+)"), f(r"; ScratchSize: (\d+)"),
            f(r"\.amdhsa_group_segment_fixed_size (\d+)"), f(r"; codeLenInByte = (\d+)"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    a = ap.parse_args()
    old, new = {}, {}
    for p in a.old:
        old.update(kernels(p))
    for p in a.new:
        new.update(kernels(p))
    bad = 0
    print(f"{'instr':>7} {'VGPR':>5} {'SGPR':>5} {'scratch':>7} {'LDS':>6} {'bytes':>7}  verdict    kernel")
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            verdict = "only old" if name in old else "only new"
        else:
            verdict = "identical" if old[name] == new[name] else "DIFFERS"
        bad += verdict != "identical"
        fig = figures(new.get(name) or old[name])
        short = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
        short = short.replace("jxlh::(anonymous namespace)::", "").split("(")[0].replace("void ", "")
        print(f"{fig[0]:>7} {fig[1]:>5} {fig[2]:>5} {fig[3]:>7} {fig[4]:>6} {fig[5]:>7}  {verdict:<10} {short}")
    print(f"{len(set(old) | set(new))} kernels, {bad} not identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
