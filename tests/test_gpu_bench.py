"""bench.py's plain run end to end on a small frame: one result line with the contract fields, exactly --steps timed
steps, nothing measured beside the headline, and --dump-outputs writing the planes of the last timed step -- which
must be the oracle's planes of the same synthetic frame, bit for bit (whole, or at the dump's sampled positions)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import bit_equal, run_oracle_frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_THREADS = max(1, min(16, len(os.sched_getaffinity(0))))


def _run_bench(out_dir, size, steps, warmup):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size", str(size),
                        "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("size", [1024, 2560])
def test_plain_run_line_and_dumped_planes_match_the_oracle(tmp_path, oracle, size):
    from jxl_rs_amd import synth
    line = _run_bench(tmp_path, size, steps=4, warmup=1)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert line.get(k) is not None, k
    assert line["unit"] == "MP/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 4 and line["warmup"] == 1 and line["repetitions"]["n"] == 1
    assert line["ms_per_step"] > 0 and abs(line["value"] - size * size / 1e3 / line["ms_per_step"]) < 0.02 * line["value"]
    for k in ("roofline", "cpu_baseline", "e2e_pcie_inclusive", "secondary", "strong_scaling"):
        assert line[k] is None, k

    files = sorted(os.listdir(tmp_path))
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= 64_000_000
    # the frame bench.py times (default --seed 3, d1 mix, EPF x2)
    wl = synth.make_vardct(size, size, mix=synth.MIX_D1, seed=3, unique_groups=24, epf_iters=2, gab=True,
                           lf_smoothing=True)
    want, _ = run_oracle_frame(oracle, wl, num_threads=ORACLE_THREADS)
    if files == ["planes.npy"]:
        got = np.load(tmp_path / "planes.npy")
        assert got.dtype == np.float32 and got.shape == (3, size, size)
        for c in range(3):
            assert bit_equal(got[c], want[c]), f"plane {c}"
    else:
        assert files == ["planes_sample.npy", "planes_sample_index.npy"], files
        got = np.load(tmp_path / "planes_sample.npy")
        idx = np.load(tmp_path / "planes_sample_index.npy")
        assert got.dtype == np.float32 and idx.dtype == np.float64 and got.shape == (3, idx.size)
        pos = idx.astype(np.int64)
        assert np.array_equal(pos, idx) and pos.min() >= 0 and pos.max() < size * size
        for c in range(3):
            assert bit_equal(got[c], want[c].reshape(-1)[pos]), f"plane {c}"
