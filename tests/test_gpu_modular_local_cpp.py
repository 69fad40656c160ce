"""The builder layer held to the C calls on the device: tests/cpp/modular_local.cc feeds one 300 x 200 Modular frame --
RCT and palette groups on a 128 grid -- through GpuModularFramePipeline::set_groups and compares the rendered planes bit
for bit with the ones this side renders from the same arena and descriptors through the C ABI (ctypes)."""
import subprocess

import numpy as np
import pytest

from test_cpp_host import _build
from test_gpu_modular_local import _frame_specs


@pytest.mark.gpu
def test_builder_batched_intake_equals_c_calls(tmp_path, oracle):
    import jxl_rs_amd
    from jxl_rs_amd import lib
    w, h = 300, 200
    specs = _frame_specs(oracle, w, h, np.random.default_rng(2028))
    arena, groups = lib.pack_local_groups(specs)
    ctx = jxl_rs_amd.Context(0, 1)
    try:
        p = ctx.default_params(w, h)
        p.gab, p.epf_iters = 0, 0
        ctx.modular_frame_begin(p)
        ctx.set_modular_groups(arena, groups, 8, n=len(specs))
        ctx.frame_run()
        ctx.sync()
        want = ctx.read_planes()
    finally:
        ctx.close()
    assert all(len(np.unique(p)) > 50 for p in want)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.uint64([w, h, len(specs), arena.size]).tobytes() + bytes(groups)[:len(specs) * 232] + arena.tobytes())
    with open(tmp_path / "want.bin", "wb") as f:
        for p in want:
            f.write(np.ascontiguousarray(p, dtype=np.float32).tobytes())
    exe = _build(tmp_path, "modular_local")
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "want.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "builder vs ctypes: 0 differing planes" in r.stdout and "modular local: ok" in r.stdout
