"""The C++ wrappers of the preview calls (include/jxl_hip.hpp) through tests/cpp/squeeze_preview.cc: the planes a
compiled caller gets are, byte for byte, those of the ctypes route on the same chain."""
import os
import subprocess

import numpy as np
import pytest

from test_cpp_host import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_wrapper_compiles_and_links(tmp_path):
    """no GPU needed: the header's new wrappers build against the library"""
    assert os.path.exists(_build(tmp_path, "squeeze_preview"))


@pytest.mark.gpu
@pytest.mark.parametrize("size,nch,n_missing,rct,rne", [((130, 65), 3, 4, (6, 0), 0), ((37, 29), 1, 2, None, 1),
                                                        ((64, 64), 3, 1, (0, 5), 1)])
def test_cpp_wrapper_equals_the_ctypes_route(tmp_path, size, nch, n_missing, rct, rne):
    from jxl_rs_amd import Context, lib
    from test_gpu_squeeze_preview import DeviceChain, chain_of
    chain = chain_of(*size, nch)
    bh, bw = chain.base[0].shape
    words = [nch, chain.n, n_missing, rct[0] if rct else -1, rct[1] if rct else 0, rne, bw, bh]
    for hz, ow, oh in chain.steps:
        words += [int(hz), ow, oh]
    parts = [np.asarray(words, np.int32)] + [b.ravel() for b in chain.base] + [r.ravel() for lvl in chain.residuals for r in lvl]
    src, dst = os.path.join(str(tmp_path), "chain.i32"), os.path.join(str(tmp_path), "planes.i32")
    np.concatenate(parts).astype(np.int32).tofile(src)
    exe = _build(tmp_path, "squeeze_preview")
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "error path ok" in r.stdout, (r.stdout + r.stderr)[-2000:]
    got = np.fromfile(dst, np.int32)
    ctx = Context(0)
    dev = DeviceChain(chain)
    try:
        missing = chain.suffix(n_missing)
        want = dev.run(ctx, missing, rct=rct, cvt_rne=bool(rne))
        kinds, live = lib.squeeze_preview_kinds(dev.levels(missing), bw, bh, n_planes=nch)
    finally:
        dev.free()
        ctx.close()
    assert np.array_equal(got[:chain.n], kinds) and np.array_equal(got[chain.n:2 * chain.n], live)
    planes = got[2 * chain.n:].reshape(nch, chain.h, chain.w)
    for c in range(nch):
        assert planes[c].tobytes() == want[c].tobytes(), c
