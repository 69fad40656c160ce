"""What RenderPipelineBuilder::lower() and lower_modular_frame() (include/jxl_hip_lowering.hpp) make of every stage list
of tests/cpp/lowering_corpus.h -- each lowered field, or the status and message of the rejection -- against
tests/golden/pipeline_lowering.json, recorded by tools/record_pipeline_lowering.py before the lowering was restructured.
A family's digest covers its lines in order, so which check wins on a list that breaks two rules is pinned too.
Host-only, no GPU."""
import json
import os
import subprocess
import sys

from test_cpp_host import ROOT, _build

sys.path.insert(0, os.path.join(ROOT, "tools"))
RECORDER = os.path.join(ROOT, "tools", "record_pipeline_lowering.py")


def _first_differing_lines(tmp_path, revision, dump, families):
    """the golden file holds digests; the lines themselves come from the recorded revision's header, where git has it"""
    rec = os.path.join(str(tmp_path), "recorded.txt")
    subprocess.run([sys.executable, RECORDER, "--rev", revision, "--dump", rec, "--out", rec + ".json"], capture_output=True)
    if not os.path.exists(rec):
        return f"(no lines to compare: revision {revision} is not at hand)"
    old, out = open(rec).read().splitlines(), []
    for n in families:
        pairs = zip([x for x in dump.splitlines() if x.startswith(n + " ")], [x for x in old if x.startswith(n + " ")])
        now, then = next(((a, b) for a, b in pairs if a != b), ("(the family's length changed)", ""))
        out.append(f"{n}: first differing line\n  now:      {now[:800]}\n  recorded: {then[:800]}")
    return "\n".join(out)


def test_every_list_lowers_as_recorded(tmp_path):
    from record_pipeline_lowering import family_digests
    exe = _build(tmp_path, "lowering_dump")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "pipeline_lowering.json")))
    got, want = family_digests(r.stdout), golden["families"]
    assert sorted(got) == sorted(want)
    bad = [n for n in sorted(want) if got[n] != want[n]]
    for n in bad:
        print(f"{n}: recorded {want[n]}\n{' ' * len(n)}  now      {got[n]}")
    if bad:
        print(_first_differing_lines(tmp_path, golden["revision"], r.stdout, bad))
    assert not bad, bad
