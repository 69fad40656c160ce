"""The builder layer held to the C calls on the device: tests/cpp/modular_local_general.cc feeds one 300 x 200 Modular
frame -- RCT groups and delta palettes under neighbour and weighted predictors on a 128 grid -- through
GpuModularFramePipeline::set_groups_general and compares the rendered planes byte for byte with the ones this side
renders from the same arena, descriptors and wp headers through the C ABI (ctypes); the stage-level wrapper is compared
with its C call inside the program."""
import subprocess

import numpy as np
import pytest

from test_cpp_host import _build
from test_gpu_modular_local_general import _frame_specs


def test_cpp_program_compiles_and_links(tmp_path):
    """no GPU needed: the headers and the program build against the library"""
    _build(tmp_path, "modular_local_general")


@pytest.mark.gpu
def test_builder_general_intake_equals_c_calls(tmp_path):
    import jxl_rs_amd
    from jxl_rs_amd import lib
    w, h = 300, 200
    specs = _frame_specs(w, h, np.random.default_rng(2029))
    arena, groups = lib.pack_local_groups(specs)
    wp = lib.wp_headers([sp["wp"] for sp in specs])
    ctx = jxl_rs_amd.Context(0, 1)
    try:
        p = ctx.default_params(w, h)
        p.gab, p.epf_iters = 0, 0
        ctx.modular_frame_begin(p)
        ctx.set_modular_groups_general(arena, groups, 8, wp=wp, n=len(specs))
        ctx.frame_run()
        ctx.sync()
        want = ctx.read_planes()
    finally:
        ctx.close()
    assert all(len(np.unique(p)) > 50 for p in want)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.uint64([w, h, len(specs), arena.size]).tobytes() + bytes(groups)[:len(specs) * 232] +
                bytes(wp)[:len(specs) * 44] + arena.tobytes())
    with open(tmp_path / "want.bin", "wb") as f:
        for p in want:
            f.write(np.ascontiguousarray(p, dtype=np.float32).tobytes())
    exe = _build(tmp_path, "modular_local_general")
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "want.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "builder vs ctypes: 0 differing planes" in r.stdout and "stage wrapper vs C call: 0 differing planes" in r.stdout
    assert "modular local general: ok" in r.stdout
