"""The builder layer held to the C calls on the device: tests/cpp/modular_frame.cc runs one 70 x 37 Modular frame with an
alpha channel through RenderPipelineBuilder::build_modular_frame -- conversions, Gaborish, EPF1, patches, the XYB + sRGB
colour stages, an RGBA8 save -- and byte-compares the image with the one this side makes from the same samples through
the C ABI (ctypes)."""
import subprocess

import numpy as np
import pytest

from test_cpp_host import _build

W, H, REF_W, REF_H = 70, 37, 80, 48


@pytest.mark.gpu
def test_builder_modular_frame_equals_c_calls(tmp_path):
    import jxl_rs_amd
    from jxl_rs_amd import lib
    rng = np.random.default_rng(2027)
    chans = [rng.integers(0, 256, size=(H, W)).astype(np.int32) for _ in range(3)]
    alpha = rng.integers(0, 256, size=(H, W)).astype(np.int32)
    alpha[:8, :16] = 0
    refs = [rng.uniform(-0.5, 1.5, (REF_H, REF_W)).astype(np.float32) for _ in range(4)]
    xyb = np.float32([1.0 if i % 4 == 0 else 0.01 * i for i in range(9)] + [0.1] * 3 + [0.001] * 3 + [1.0])
    ctx = jxl_rs_amd.Context(0, 1)
    try:
        ctx.set_reference(0, refs)
        p = ctx.default_params(W, H)
        p.gab, p.epf_iters = 1, 1
        ctx.modular_frame_begin(p)
        ctx.set_modular_channels(*chans, 8)
        ctx.set_extra_channel(0, alpha, 8)
        ctx.set_patches([(3, 2, 0, 5, 4, 40, 20), (50, 20, 0, 0, 0, 20, 17)],
                        [(lib.PATCH_REPLACE, 0, 0), (lib.PATCH_REPLACE, 0, 0), (lib.PATCH_BLEND_ABOVE, 0, 1),
                         (lib.PATCH_BLEND_ABOVE, 0, 0)], [lib.EC_ALPHA])
        ctx.frame_run()
        want = ctx.frame_save(lib.save_desc([0, 1, 2, 3], lib.SAVE_U8), ctx.output_desc(lib.COLOR_XYB, "srgb", xyb))
        ctx.clear_reference(0)
    finally:
        ctx.close()
    assert want.shape == (H, W * 4) and len(np.unique(want)) > 32
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.int32([W, H, REF_W, REF_H]).tobytes() + xyb.tobytes())
        for a in chans + [alpha] + refs:
            f.write(np.ascontiguousarray(a).tobytes())
    (tmp_path / "want.bin").write_bytes(want.tobytes())
    exe = _build(tmp_path, "modular_frame")
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "want.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "builder vs ctypes: 0 differing bytes" in r.stdout and "modular frame: ok" in r.stdout
