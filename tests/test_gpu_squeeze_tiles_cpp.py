"""The C++ wrappers of the per-cell preview calls (include/jxl_hip.hpp) through tests/cpp/squeeze_tiles.cc: a download
painted after every group -- the streaming sequence -- gives a compiled caller, byte for byte, the planes of the ctypes
route on the same chain."""
import os
import subprocess

import numpy as np
import pytest

import squeeze_tiles_ref as ref
from test_cpp_host import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_wrapper_compiles_and_links(tmp_path):
    """no GPU needed: the header's new wrappers build against the library"""
    assert os.path.exists(_build(tmp_path, "squeeze_tiles"))


@pytest.mark.gpu
@pytest.mark.parametrize("g,nch,rct,rne", [("40x24", 3, (6, 0), 0), ("33x29", 1, None, 1)])
def test_cpp_streaming_sequence_equals_the_ctypes_route(tmp_path, g, nch, rct, rne):
    from jxl_rs_amd import Context, lib
    from test_gpu_squeeze_preview import DeviceChain, chain_of
    size, finest = ref.GEOMETRIES[g]
    chain = chain_of(*size, nch)
    n = chain.n
    bh, bw = chain.base[0].shape
    shapes = [ref.grid_of(chain.steps[n - 1 - k], ref.level_tiles(chain.steps, finest, k))[3:1:-1] for k in range(2)]
    masks = {k: np.zeros(shapes[k], np.uint8) for k in range(2)}
    paints = []
    for i, at in enumerate([None] + list(np.ndindex(shapes[0]))):
        if at is not None:
            masks[0][at] = masks[1][at] = 1 + i % 200
        paints.append(ref.build_tiles(chain.steps, finest, {k: m.copy() for k, m in masks.items()})[0])
    words = [nch, n, rct[0] if rct else -1, rct[1] if rct else 0, rne, bw, bh, len(paints)]
    for (hz, ow, oh), (tw, th, _) in zip(chain.steps, paints[0]):
        words += [int(hz), ow, oh, tw, th]
    parts = [np.asarray(words, np.int32)] + [b.ravel() for b in chain.base] + [r.ravel() for lvl in chain.residuals for r in lvl]
    for tiles in paints:
        for _, _, present in tiles:
            parts.append(np.asarray([0] if present is None else [present.size] + list(present.ravel()), np.int32))
    src, dst = os.path.join(str(tmp_path), "chain.i32"), os.path.join(str(tmp_path), "planes.i32")
    np.concatenate(parts).astype(np.int32).tofile(src)
    exe = _build(tmp_path, "squeeze_tiles")
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "error path ok" in r.stdout, (r.stdout + r.stderr)[-2000:]
    got = np.fromfile(dst, np.int32)
    n_cells = shapes[0][0] * shapes[0][1]
    per_paint = n_cells + nch * chain.h * chain.w
    assert got.size == per_paint * len(paints)
    ctx = Context(0)
    dev = DeviceChain(chain)
    try:
        for i, tiles in enumerate(paints):
            ctx.unsqueeze_chain_preview_tiles(dev.levels([False] * n), tiles, dev.base, bw, bw, bh, dev.out_ptr, dev.out_stride,
                                              rct=rct, cvt_rne=bool(rne))
            ctx.sync()
            want = dev.result()
            dev.poison()
            kinds = lib.squeeze_tile_kinds(dev.levels([False] * n), tiles, bw, bh, n - 1, n_planes=nch)
            part = got[i * per_paint:(i + 1) * per_paint]
            assert np.array_equal(part[:n_cells], kinds.ravel()), i
            planes = part[n_cells:].reshape(nch, chain.h, chain.w)
            for c in range(nch):
                assert planes[c].tobytes() == want[c].tobytes(), (i, c)
    finally:
        dev.free()
        ctx.close()
