"""The builder layer held to the C calls on the device: tests/cpp/modular_local_extra.cc feeds one 203 x 137 RGBA Modular
frame -- cells of 64 with every step list of tests/modular_local_extra_cases.py in turn -- through
GpuModularFramePipeline::set_groups(..., dest), and a second extra channel through GpuFramePipeline::set_extra_groups,
and compares the rendered colour planes and both extra channels byte for byte with the ones this side renders from the
same arena and descriptors through the C ABI (ctypes)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import modular_local_extra_cases as ec
from test_cpp_host import _build


def test_cpp_program_compiles_and_links(tmp_path):
    """no GPU needed: the headers and the program build against the library"""
    _build(tmp_path, "modular_local_extra")


@pytest.mark.gpu
def test_builder_extra_intake_equals_c_calls(tmp_path):
    import jxl_rs_amd
    from jxl_rs_amd import lib
    w, h, cell = ec.RAGGED
    names = ec.lists_for(4)
    rgba = [ec.spec(names[i % len(names)], 7, x0, y0, gw, gh, 4) for i, (x0, y0, gw, gh) in enumerate(ec.grid(w, h, cell))]
    one = [ec.spec("palette_all", 8, x0, y0, gw, gh, 1) for x0, y0, gw, gh in ec.grid(w, h, 128)]
    arena, (groups, coded, params) = lib.pack_local_squeeze_groups(rgba + one)
    n, n1 = len(rgba), len(one)
    n_coded = sum(len(sp["coded"]) for sp in rgba + one)
    n_params = sum(len(sp["squeeze"] or ()) for sp in rgba + one)
    wp = lib.wp_headers([sp["wp"] for sp in rgba])
    G = C.sizeof(lib.LocalSqueezeGroup)
    one_groups = (lib.LocalSqueezeGroup * n1).from_buffer_copy(bytes(groups)[n * G:(n + n1) * G])
    ctx = jxl_rs_amd.Context(0, 1)
    try:
        p = ctx.default_params(w, h)
        p.gab, p.epf_iters = 0, 0
        ctx.modular_frame_begin(p)
        ctx.begin_extra_channel(0, w, h, 8, 1)
        ctx.begin_extra_channel(1, w, h, 8, 1)
        ctx.set_modular_groups_extra(arena, (groups, coded, params), 8, lib.local_dest(3, [0]), wp=wp, n=n)
        ctx.set_modular_groups_extra(arena, (one_groups, coded, params), 0, lib.local_dest(0, [1], bit_depth=8), n=n1)
        ctx.frame_run()
        ctx.sync()
        want = ctx.read_planes() + [ctx.read_extra_channel(0, w, h), ctx.read_extra_channel(1, w, h)]
    finally:
        ctx.close()
    assert all(len(np.unique(q)) > 50 for q in want)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.uint64([w, h, n, n_coded, n_params, arena.size, n1, n_coded]).tobytes() +
                bytes(groups)[:n * G] + bytes(coded)[:n_coded * C.sizeof(lib.LocalCodedChannel)] +
                bytes(params)[:n_params * C.sizeof(lib.SqueezeParams)] + bytes(wp)[:n * C.sizeof(lib.WpHeader)] +
                bytes(one_groups) + bytes(coded)[:n_coded * C.sizeof(lib.LocalCodedChannel)] + arena.tobytes())
    with open(tmp_path / "want.bin", "wb") as f:
        for q in want:
            f.write(np.ascontiguousarray(q, dtype=np.float32).tobytes())
    exe = _build(tmp_path, "modular_local_extra")
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "want.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "builder vs ctypes: 0 differing planes" in r.stdout and "not-rendered read refused" in r.stdout
    assert "refusals: 3 of 3" in r.stdout and "modular local extra: ok" in r.stdout
