"""The builder layer held to the C calls on the device: tests/cpp/modular_local_squeeze.cc feeds one 600 x 420 Modular
frame -- default squeezes, squeezes behind an RCT and behind predicted palettes, and RCT groups without one, on a 200
grid -- through GpuModularFramePipeline::set_groups and compares the rendered planes byte for byte with the ones this
side renders from the same arena and descriptors through the C ABI (ctypes); the stage-level wrapper is compared with
its C call inside the program."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from test_cpp_host import _build
from test_gpu_modular_local_squeeze import _frame_specs


def test_cpp_program_compiles_and_links(tmp_path):
    """no GPU needed: the headers and the program build against the library"""
    _build(tmp_path, "modular_local_squeeze")


@pytest.mark.gpu
def test_builder_squeeze_intake_equals_c_calls(tmp_path):
    import jxl_rs_amd
    from jxl_rs_amd import lib
    w, h = 600, 420
    specs = _frame_specs(w, h, np.random.default_rng(2030))
    arena, (groups, coded, params) = lib.pack_local_squeeze_groups(specs)
    n_coded, n_params = sum(len(sp["coded"]) for sp in specs), sum(len(sp["squeeze"] or ()) for sp in specs)
    wp = lib.wp_headers([sp["wp"] for sp in specs])
    ctx = jxl_rs_amd.Context(0, 1)
    try:
        p = ctx.default_params(w, h)
        p.gab, p.epf_iters = 0, 0
        ctx.modular_frame_begin(p)
        ctx.set_modular_groups_squeeze(arena, (groups, coded, params), 8, wp=wp, n=len(specs))
        ctx.frame_run()
        ctx.sync()
        want = ctx.read_planes()
    finally:
        ctx.close()
    assert all(len(np.unique(p)) > 50 for p in want)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.uint64([w, h, len(specs), n_coded, n_params, arena.size]).tobytes() +
                bytes(groups)[:len(specs) * C.sizeof(lib.LocalSqueezeGroup)] + bytes(coded)[:n_coded * C.sizeof(lib.LocalCodedChannel)] +
                bytes(params)[:n_params * C.sizeof(lib.SqueezeParams)] + bytes(wp)[:len(specs) * C.sizeof(lib.WpHeader)] + arena.tobytes())
    with open(tmp_path / "want.bin", "wb") as f:
        for p in want:
            f.write(np.ascontiguousarray(p, dtype=np.float32).tobytes())
    exe = _build(tmp_path, "modular_local_squeeze")
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "want.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "builder vs ctypes: 0 differing planes" in r.stdout and "stage wrapper vs C call: 0 differing planes" in r.stdout
    assert "modular local squeeze: ok" in r.stdout
