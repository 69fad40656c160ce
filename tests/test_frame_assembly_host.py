"""Host side of the rect-by-rect frame assembly tests (tests/test_gpu_frame_assembly.py): the rect generators cover the
frame, and the binding turns numpy views into the (pointer, stride) pairs the C ABI takes without copying what it need
not copy.  No GPU."""
import numpy as np
import pytest

from helpers import (LF_GROUP_BLOCKS, lf_group_rects, lf_piece, ragged_lf_rects, ragged_map_rects, rects_cover,
                     subsampled_corner_mask, _padded)

# blocks; includes sizes that are not multiples of 8 or of 256, a single block, and more than one LF group each way
SIZES = [(1, 1), (9, 5), (65, 38), (98, 65), (64, 64), (263, 5), (5, 263), (288, 265), (512, 256), (513, 257)]


@pytest.mark.parametrize("xb,yb", SIZES)
def test_lf_group_grid_tiles_the_frame_exactly(xb, yb):
    rects = lf_group_rects(xb, yb)
    assert (rects_cover(rects, xb, yb) == 1).all()
    assert len(rects) == -(-xb // LF_GROUP_BLOCKS) * -(-yb // LF_GROUP_BLOCKS)
    assert all(x0 % LF_GROUP_BLOCKS == 0 and y0 % LF_GROUP_BLOCKS == 0 and 0 < w <= LF_GROUP_BLOCKS and
               0 < h <= LF_GROUP_BLOCKS for x0, y0, w, h in rects)


@pytest.mark.parametrize("xb,yb", SIZES)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_ragged_lf_tiling_covers_every_block_once(xb, yb, seed):
    rects = ragged_lf_rects(xb, yb, seed)
    assert (rects_cover(rects, xb, yb) == 1).all()   # raises if a rect leaves the frame
    assert all(w > 0 and h > 0 for _, _, w, h in rects)
    if xb > 2 and yb > 2:
        assert any(w == 1 for _, _, w, _ in rects) and any(h == 1 for _, _, _, h in rects)
        assert any(x0 % 2 for x0, _, _, _ in rects) and any(y0 % 2 for _, y0, _, _ in rects)
        assert len({(w, h) for _, _, w, h in rects}) > 1


@pytest.mark.parametrize("xb,yb", SIZES)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_ragged_map_tiling_covers_every_block_from_aligned_origins(xb, yb, seed):
    rects = ragged_map_rects(xb, yb, seed)
    assert (rects_cover(rects, xb, yb) >= 1).all()
    assert all(x0 % 8 == 0 and y0 % 8 == 0 and w > 0 and h > 0 for x0, y0, w, h in rects)
    # a rect that does not end at the frame's edge ends inside a colour tile, which its neighbour also delivers
    for x0, y0, w, h in rects:
        assert x0 + w == xb or (x0 + w) % 8
        assert y0 + h == yb or (y0 + h) % 8
    if xb > 16 or yb > 16:
        assert (rects_cover(rects, xb, yb) > 1).any()


def test_ragged_tilings_are_seeded():
    assert ragged_lf_rects(98, 65, 4) == ragged_lf_rects(98, 65, 4) != ragged_lf_rects(98, 65, 5)
    assert ragged_map_rects(98, 65, 4) == ragged_map_rects(98, 65, 4) != ragged_map_rects(98, 65, 5)


def test_rects_cover_rejects_a_rect_outside_the_frame():
    with pytest.raises(ValueError):
        rects_cover([(0, 0, 9, 4)], 8, 4)


def test_corner_mask_follows_the_lf_group_grid():
    class W:  # geometry only
        opts = dict(hshift=(1, 0, 0), vshift=(1, 0, 1))
        xblocks, yblocks = 264, 260
    m = subsampled_corner_mask(W, 0)
    assert m[:128, :128].all() and not m[:256, 128:256].any() and not m[128:256, :].any()
    assert m[256:258, 256:260].all() and not m[258:, :].any() and not m[256:, 260:].any() and m[256:258, :128].all()
    assert subsampled_corner_mask(W, 1).all()
    b = subsampled_corner_mask(W, 2)
    assert b[:128, :256].all() and b[256:258, :].all() and not b[128:256, :].any()


def test_lf_piece_scales_by_the_rects_precision():
    class W:
        lf_q = [np.arange(48, dtype=np.int32).reshape(6, 8) - 20 + 100 * c for c in range(3)]
    got = lf_piece(W, (3, 1, 4, 2), ep=3)
    for c in range(3):
        assert np.array_equal(got[c], W.lf_q[c][1:3, 3:7] * 8) and got[c].dtype == np.int32
    low = lf_piece(W, (3, 1, 4, 2), ep=2, low_bits=np.random.default_rng(0))
    for c in range(3):
        assert np.array_equal(low[c] >> 2, W.lf_q[c][1:3, 3:7]) and (low[c] & 3).any()


# ---------------------------------------------------------------- the binding's stride handling
def test_binding_passes_a_slice_of_a_wider_array_as_it_is():
    from jxl_rs_amd.lib import _rect_planes
    big = [np.arange(40 * 50, dtype=np.int32).reshape(40, 50) + c for c in range(3)]
    views = [b[3:20, 7:30] for b in big]
    arrs, w, h, stride = _rect_planes(views, np.int32, None, None, None)
    assert (w, h, stride) == (23, 17, 50)
    assert all(a.ctypes.data == v.ctypes.data for a, v in zip(arrs, views))  # no copy
    # rows read through (pointer, stride) are the slice's rows
    flat = np.frombuffer(big[1], dtype=np.int32)
    first = (arrs[1].ctypes.data - big[1].ctypes.data) // 4
    for y in range(h):
        assert np.array_equal(flat[first + y * stride:first + y * stride + w], views[1][y])


def test_binding_copies_into_one_pitch_only_when_pitches_differ():
    from jxl_rs_amd.lib import _rect_planes
    a = np.zeros((10, 30), dtype=np.float32)[:, 2:12]
    b = np.ones((10, 31), dtype=np.float32)[:, 2:12]
    c = np.full((10, 30), 2, dtype=np.float32)[:, 5:15]
    arrs, w, h, stride = _rect_planes((a, a, c), np.float32, None, None, None)
    assert stride == 30 and arrs[2].ctypes.data == c.ctypes.data
    arrs, w, h, stride = _rect_planes((a, b, c), np.float32, None, None, None)
    assert (w, h, stride) == (10, 10, 10) and all(x.flags.c_contiguous for x in arrs)
    assert np.array_equal(arrs[1], b) and np.array_equal(arrs[2], c)


def test_binding_copies_what_the_abi_cannot_address():
    from jxl_rs_amd.lib import _rect_planes
    base = np.arange(20 * 20, dtype=np.int32).reshape(20, 20)
    for v in (base[:, ::2], base[::-1, :], base.T, base.astype(np.int64), base.astype(">i4")):
        arrs, w, h, stride = _rect_planes((v, v, v), np.int32, None, None, None)
        assert stride == w == v.shape[1] and h == v.shape[0]
        assert arrs[0].dtype == np.int32 and arrs[0].flags.c_contiguous and np.array_equal(arrs[0], v)
    # every other row: rows contiguous, pitch 40 -> passed as it is
    arrs, w, h, stride = _rect_planes((base[::2],) * 3, np.int32, None, None, None)
    assert stride == 40 and arrs[0].ctypes.data == base.ctypes.data


def test_binding_block_maps_share_a_pitch_in_elements_not_bytes():
    from jxl_rs_amd.lib import _rect_planes_mixed
    tm = _padded(np.ones((9, 13), dtype=np.uint8), 6)
    rq = _padded(np.ones((9, 13), dtype=np.int32), 6)
    em = _padded(np.ones((9, 13), dtype=np.uint8), 6)
    assert tm.strides[0] == 19 and rq.strides[0] == 76
    arrs, w, h, stride = _rect_planes_mixed((tm, rq, em), (np.uint8, np.int32, np.uint8))
    assert (w, h, stride) == (13, 9, 19) and [a.ctypes.data for a in arrs] == [tm.ctypes.data, rq.ctypes.data, em.ctypes.data]
    em2 = _padded(np.ones((9, 13), dtype=np.uint8), 2)
    arrs, w, h, stride = _rect_planes_mixed((tm, rq, em2), (np.uint8, np.int32, np.uint8))
    assert stride == 13 and all(a.flags.c_contiguous for a in arrs)


def test_binding_single_rows_and_empty_rects():
    from jxl_rs_amd.lib import _rect_planes
    big = np.arange(100, dtype=np.int32).reshape(10, 10)
    arrs, w, h, stride = _rect_planes((big[4:5, 2:9],) * 3, np.int32, None, None, None)
    assert (w, h) == (7, 1) and stride >= w and arrs[0].ctypes.data == big[4:5, 2:9].ctypes.data
    for v in (big[3:3, 2:9], big[2:6, 4:4]):
        arrs, w, h, stride = _rect_planes((v,) * 3, np.int32, None, None, None)
        assert (h, w) == v.shape and stride >= max(w, 1)


def test_binding_device_pointers_need_their_geometry():
    from jxl_rs_amd.lib import _rect_planes
    assert _rect_planes((4096, 8192, 12288), np.int32, 5, 6, 9) == ([4096, 8192, 12288], 5, 6, 9)
    with pytest.raises(ValueError):
        _rect_planes((4096, 8192, 12288), np.int32, 5, 6, None)
    with pytest.raises(ValueError):
        _rect_planes((4096, np.zeros((6, 5), np.int32), 12288), np.int32, 5, 6, 9)
    with pytest.raises(ValueError):
        _rect_planes((np.zeros((6, 5), np.int32),) * 3, np.int32, 5, 6, 9)
    with pytest.raises(ValueError):
        _rect_planes((np.zeros((6, 5), np.int32), np.zeros((6, 4), np.int32), np.zeros((6, 5), np.int32)), np.int32,
                     None, None, None)


def test_padding_is_poisoned_on_both_sides():
    v = _padded(np.zeros((3, 4), dtype=np.float32), 5)
    assert np.isnan(v.base[:, :2]).all() and np.isnan(v.base[:, 6:]).all() and not np.isnan(v).any()
    q = _padded(np.zeros((3, 4), dtype=np.int32), 5)
    assert (q.base[:, :2] == 0x7fffffff).all() and (q.base[:, 6:] == 0x7fffffff).all()
    assert (_padded(np.zeros((3, 4), dtype=np.uint8), 3).base[:, 5:] == 0xff).all()
