"""The transform stage's work-list memory (k_vardct_scan.hip, vardct_worklist_layout): one layout gives both the bytes
jxlh_frame_begin allocates and the regions launch_vardct_groups carves from them.  Swept over every frame of
1..512 x 1..512 blocks through the host-only jxlh_worklist_layout (jxl_hip_dev.h): each region holds the worst case
a frame of that size can put in it, the regions follow each other without overlap and the last one ends inside the
allocation.  No GPU needed."""
import numpy as np

# class order of the work lists (k_vardct_common.h): DCT8, 16x8, 8x16, 16x16, 32x8, 8x32, 32x16, 16x32, 32x32, special,
# large.  MIN_AREA: the fewest 8x8 blocks a varblock of the class covers (worst case = one varblock per MIN_AREA blocks);
# BATCH: varblocks per batch of the DCT classes (Shape::NB, k_vardct.hip) -- one fallback flag word per batch.
MIN_AREA = np.array([1, 2, 2, 4, 4, 4, 8, 8, 16, 1, 32], np.int64)
BATCH = np.array([8, 8, 8, 4, 4, 8, 4, 4, 2], np.int64)
NUM_CLASSES, NUM_DCT = 11, 9
COUNT_LINES, COUNT_PITCH = 33, 32   # kCountLines counters, one 128-byte line each, two sets
FB_ANY, FB_ANY_PITCH = 32, 32
R_ITEMS, R_EITEMS, R_DITEMS, R_FALLBACK = 1, 1 + NUM_CLASSES, 1 + NUM_CLASSES + NUM_DCT, 1 + NUM_CLASSES + 2 * NUM_DCT
R_FB_ANY = R_FALLBACK + NUM_DCT
R_UNITS, R_LLF, NUM_REGIONS = R_FB_ANY + 1, R_FB_ANY + 2, R_FB_ANY + 3


def worst_case_bytes(n):
    """bytes each region must hold for frames of n blocks (n: int64 array) -> [len(n), NUM_REGIONS]"""
    n = np.asarray(n, np.int64)
    need = np.zeros((n.size, NUM_REGIONS), np.int64)
    need[:, 0] = 2 * COUNT_LINES * COUNT_PITCH * 4
    for c in range(NUM_CLASSES):
        need[:, R_ITEMS + c] = n // MIN_AREA[c] * 16
    for c in range(NUM_DCT):
        vb = n // MIN_AREA[c]
        need[:, R_EITEMS + c] = vb * 16
        need[:, R_DITEMS + c] = vb * 16
        need[:, R_FALLBACK + c] = (vb + BATCH[c] - 1) // BATCH[c] * 4
    need[:, R_FB_ANY] = FB_ANY * FB_ANY_PITCH * 4
    # k_vardct_large.hip carves the unit region into the two-pass units and the three fused lists (the last one by
    # its worst case: one entry per 256 blocks)
    need[:, R_UNITS] = ((n // 32 + 16) * 2 + (n // 128 + 16) + n // 256) * 4
    need[:, R_LLF] = 3 * n * 4
    return need


def layout_faults(n, total, off, ln):
    """Block counts (of n) whose layout is wrong, with what is wrong: a region shorter than its worst case, one that
    starts before the previous one ends, one that ends past the allocation, unaligned LLF planes."""
    n, total, off, ln = (np.asarray(a, np.int64) for a in (n, total, off, ln))
    end = off + ln
    bad = {}
    short = ln < worst_case_bytes(n)
    overlap = np.zeros_like(short)
    overlap[:, 1:] = off[:, 1:] < end[:, :-1]
    past = end > total[:, None]
    for name, m in (("short", short), ("overlap", overlap), ("past the end", past)):
        for i in np.flatnonzero(m.any(axis=1)):
            bad.setdefault(int(n[i]), []).append((name, [int(r) for r in np.flatnonzero(m[i])],
                                                  int((end[i].max() - total[i]) if name == "past the end" else 0)))
    for i in np.flatnonzero(off[:, R_LLF] % 64):
        bad.setdefault(int(n[i]), []).append(("llf unaligned", [R_LLF], 0))
    return dict(sorted(bad.items()))


def library_layouts(blocks):
    from jxl_rs_amd import lib
    total = np.zeros(len(blocks), np.int64)
    off = np.zeros((len(blocks), NUM_REGIONS), np.int64)
    ln = np.zeros_like(off)
    for i, (xb, yb) in enumerate(blocks):
        total[i], regions = lib.worklist_layout(xb, yb)
        off[i], ln[i] = np.array(regions, np.int64).T
    return total, off, ln


def test_worklist_layout_sweep_1_to_512_blocks_each_way():
    from jxl_rs_amd import lib
    assert lib.WORKLIST_REGIONS == NUM_REGIONS
    # the layout depends on the block count only: one call per distinct product of 1..512 x 1..512
    xb, yb = np.meshgrid(np.arange(1, 513), np.arange(1, 513))
    prod = (xb * yb).reshape(-1)
    n, first = np.unique(prod, return_index=True)
    blocks = list(zip(xb.reshape(-1)[first].tolist(), yb.reshape(-1)[first].tolist()))
    total, off, ln = library_layouts(blocks)
    faults = layout_faults(n, total, off, ln)
    assert not faults, "first failing block counts: %s" % list(faults.items())[:8]
    # ... and a frame's layout does not depend on its aspect: 28 blocks as 28 x 1, 1 x 28, 7 x 4, 4 x 7
    shapes = [(28, 1), (1, 28), (7, 4), (4, 7)]
    t2, o2, l2 = library_layouts(shapes)
    assert (t2 == t2[0]).all() and (o2 == o2[0]).all() and (l2 == l2[0]).all()


def test_worklist_layout_large_frames():
    """8K and 16K frames and the block-count limit's neighbourhood: the same checks far past the sweep."""
    blocks = [(960, 540), (1920, 1080), (2048, 2048), (4096, 4096 - 1), (8191, 8191)]
    total, off, ln = library_layouts(blocks)
    n = np.array([x * y for x, y in blocks], np.int64)
    assert not layout_faults(n, total, off, ln)


def test_worklist_layout_rejects_bad_sizes():
    import ctypes as C
    from jxl_rs_amd import lib
    L = lib._lib()
    out = np.zeros(1 + 2 * NUM_REGIONS, np.uint64)
    for xb, yb in ((0, 1), (1, 0), (-3, 5)):
        assert L.jxlh_worklist_layout(C.c_int32(xb), C.c_int32(yb), lib._addr(out), C.c_int32(out.size)) != 0
    # n caps what is written
    out[:] = 7
    assert L.jxlh_worklist_layout(C.c_int32(4), C.c_int32(4), lib._addr(out), C.c_int32(3)) == 0
    assert out[0] > 0 and out[1] == 0 and out[2] > 0 and (out[3:] == 7).all()
