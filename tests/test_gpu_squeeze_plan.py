"""The default squeeze chain, one call, at the final sizes that sit on the planner's thresholds (squeeze_plan.h): lines
of 255 / 256 / 257 output samples on each axis (a level is streamed from 256), sides of 128 / 129 (the LDS-resident
prefix ends at 128), chains of exactly one and two levels, a chain whose only streamed level is the last one with the
RCT behind it, and one with a dataflow run.  Three planes with and without the RCT and one plane, on tight aligned
output planes and on planes with an odd stride that start 4 bytes off a 16-byte boundary; bit-exact against the oracle's
step-by-step result, padding untouched."""
import functools

import numpy as np
import pytest

from helpers import DeviceArray
from jxl_rs_amd import synth

SIZES = [(255, 40), (256, 40), (257, 40), (40, 255), (40, 256), (40, 257), (128, 128), (129, 128), (128, 129),
         (9, 8), (9, 9), (200, 256), (300, 600)]
SENTINEL = -777


def test_the_sizes_are_what_they_are_meant_to_be():
    steps = {s: synth.default_squeeze_steps(*s)[0] for s in SIZES}
    streamed = lambda st: (st[1] if st[0] else st[2]) // 2 >= 128
    assert len(steps[(9, 8)]) == 1 and len(steps[(9, 9)]) == 2
    assert [streamed(st) for st in steps[(200, 256)]][-3:] == [False, False, True]
    assert sum(streamed(st) for st in steps[(300, 600)]) >= 3 and max(max(s) for s in SIZES) <= 600
    for a, b in [((255, 40), (256, 40)), ((40, 255), (40, 256))]:
        assert not any(streamed(st) for st in steps[a]) and streamed(steps[b][-1])


@pytest.fixture(scope="module")
def ctx():
    from jxl_rs_amd import Context
    c = Context(0, n_slots=1)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _planes(size):
    return synth.make_modular_planes(*size, seed=size[0] * 1000 + size[1])


_want = {}


def _reference(oracle, size):
    if size not in _want:
        base, residuals, steps = _planes(size)
        cur = [b.copy() for b in base]
        for (hz, ow, oh), res in zip(steps, residuals):
            cur = [oracle.unsqueeze_h(cur[c], res[c], ow) if hz else oracle.unsqueeze_v(cur[c], res[c], oh) for c in range(3)]
        _want[size] = (cur, oracle.rct(cur, 6, 0))
    return _want[size]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["tight", "odd_stride_4_bytes_off"])
@pytest.mark.parametrize("planes_rct", [(3, (6, 0)), (3, None), (1, None)], ids=["3_rct", "3", "1"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_default_chain_on_the_planner_thresholds(ctx, oracle, size, planes_rct, layout):
    w, h = size
    n_planes, rct = planes_rct
    base, residuals, steps = _planes(size)
    plain, with_rct = _reference(oracle, size)
    want = with_rct if rct is not None else plain
    stride, off = (w, 0) if layout == "tight" else (w + 1 + w % 2, 1)   # odd, and above w
    bufs = []

    def dev(a):
        bufs.append(DeviceArray(np.ascontiguousarray(a, dtype=np.int32)))
        return bufs[-1]

    try:
        d_base = [dev(base[c]) for c in range(n_planes)]
        levels = [(hz, ow, oh, [dev(res[c]).ptr for c in range(n_planes)], res[0].shape[1])
                  for (hz, ow, oh), res in zip(steps, residuals)]
        n_out = off + h * stride + 7
        d_out = [dev(np.full(n_out, SENTINEL, np.int32)) for _ in range(n_planes)]
        ctx.unsqueeze_chain(levels, [d.ptr for d in d_base], base[0].shape[1], base[0].shape[1], base[0].shape[0],
                            [d.ptr + 4 * off for d in d_out], stride, rct=rct)
        ctx.sync()
        for c in range(n_planes):
            raw = d_out[c].download(np.int32, n_out)
            got = raw[off:off + h * stride].reshape(h, stride)
            assert np.array_equal(got[:, :w], want[c]), (size, planes_rct, layout, c, np.argwhere(got[:, :w] != want[c])[:5])
            assert (got[:, w:] == SENTINEL).all() and (raw[:off] == SENTINEL).all() and (raw[off + h * stride:] == SENTINEL).all()
    finally:
        for d in bufs:
            d.free()
