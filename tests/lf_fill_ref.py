"""What a frame with groups whose HF has not arrived must look like (jxlh_frame_set_groups_lf_only), built from what the
oracle already has, and a line-by-line emulation of the reference's upsample_lf_group (jxl/src/frame/decode.rs:51-158)
that pins where the two agree.

The contract: ahead of the filters a marked group's pixels are the group's rect of Upsample8x applied to the WHOLE LF
image; an unmarked group's are decode_group's.  Gaborish and the EPF stages then run over the frame as they always do.
With no group marked the composition is oracle.vardct_frame bit for bit (tests/test_lf_fill_cpu.py)."""
import ctypes as C

import numpy as np

from helpers import oracle_params_from

GROUP_BLOCKS = 32


def _ptr(a, ty=C.c_float):
    return a.ctypes.data_as(C.POINTER(ty))


def lf_image(o, wl, p, lf=None, from_slot=False):
    """Frame::finalize_lf: the dequantised LF (or `lf` as handed over), smoothed when the frame asks for it, does not take
    its LF from an LF frame, and is more than 2 blocks each way (adaptive_lf_smoothing.rs:51-53)"""
    lf = o.dequant_lf(p, *wl.lf_q) if lf is None else [np.ascontiguousarray(a, dtype=np.float32) for a in lf]
    if p.do_lf_smoothing and not from_slot and wl.xblocks > 2 and wl.yblocks > 2:
        lf = o.adaptive_lf_smoothing(p, lf)
    return lf


def group_rect(wl, g):
    """pixel rect of group g in whole blocks: (y0, y1, x0, x1)"""
    gx, gy = g % wl.xgroups, g // wl.xgroups
    return (gy * 256, min((gy + 1) * 256, wl.yblocks * 8), gx * 256, min((gx + 1) * 256, wl.xblocks * 8))


def unfiltered_planes(o, wl, p, lf, marked, weights8=None, coeffs=None):
    """the planes ahead of the filters, padded to whole blocks: decode_group for the unmarked groups, the 256 x 256 crop
    of upsample(8, lf[c], weights8) for the marked ones.  coeffs[g] of a marked group is never looked at."""
    coeffs = wl.coeffs if coeffs is None else coeffs
    marked = set(int(g) for g in marked)
    planes = [np.zeros((wl.yblocks * 8, wl.xblocks * 8), np.float32) for _ in range(3)]
    for g in range(wl.xgroups * wl.ygroups):
        if g not in marked:
            o.decode_group(p, g, coeffs[g], wl.transform_map, wl.raw_quant, wl.ytox, wl.ytob, lf, wl.tables, planes)
    if marked:
        up = [o.upsample(8, a, weights8) for a in lf]
        for g in marked:
            y0, y1, x0, x1 = group_rect(wl, g)
            for c in range(3):
                planes[c][y0:y1, x0:x1] = up[c][y0:y1, x0:x1]
    return planes


def filtered(o, wl, p, planes):
    """the stage list of frame/render.rs:569-622 on the frame (mirrored at xsize x ysize), as Oracle.vardct_band runs it"""
    stride = wl.xblocks * 8
    cur = [np.ascontiguousarray(a) for a in planes]
    oth = [np.zeros_like(a) for a in cur]
    sigma = o.sigma_map(p, wl.raw_quant, wl.epf_map)
    stages = ([-1] if p.gab else []) + ([0] if p.epf_iters >= 3 else []) + ([1] if p.epf_iters >= 1 else []) + \
        ([2] if p.epf_iters >= 2 else [])
    for st in stages:
        if st < 0:
            for c in range(3):
                o.lib.jxlo_gaborish_rows(_ptr(cur[c]), p.xsize, p.ysize, stride, C.c_float(p.gab_w1[c]),
                                         C.c_float(p.gab_w2[c]), _ptr(oth[c]), 0, p.ysize)
        else:
            o.lib.jxlo_epf_rows(st, C.byref(p), o._p3(cur), p.xsize, p.ysize, stride, _ptr(sigma), sigma.shape[1],
                                o._p3(oth), 0, p.ysize)
        cur, oth = oth, cur
    return cur


def expected_planes(o, wl, marked, lf=None, from_slot=False, weights8=None, coeffs=None, **over):
    """the frame's planes behind the filters, cropped to the frame; **over as helpers.gpu_params_from takes them"""
    p = oracle_params_from(o, wl, **over)
    lf = lf_image(o, wl, p, lf, from_slot)
    planes = filtered(o, wl, p, unfiltered_planes(o, wl, p, lf, marked, weights8, coeffs))
    return [a[:wl.ysize, :wl.xsize].copy() for a in planes]


# ---------------------------------------------------------------- the reference's function, line by line (4:4:4)
def _mirror(v, s):
    while True:
        if v < 0:
            v = -v - 1
        elif v >= s:
            v = 2 * s - v - 1
        else:
            return v


def emulate_upsample_lf_group(o, lf, group, xgroups, weights8=None):
    """upsample_lf_group(group, ..) on the LF image `lf` (X, Y, B) of a 4:4:4 frame: the five persistent scratch rows
    (zeroed once per call, shared by the rows and the channels), the copy of columns [start_x, end_x), the two paddings
    as the code indexes them, Upsample8x on the scratch rows.  Returns three (8 * rows) x (8 * cols) arrays: the
    group's blocks inside the image."""
    lf_h, lf_w = lf[0].shape
    gx, gy = group % xgroups, group // xgroups
    lf_x0, lf_y0 = gx * GROUP_BLOCKS, gy * GROUP_BLOCKS
    start_x = max(lf_x0 - 2, 0)
    lf_x1 = min(lf_x0 + GROUP_BLOCKS, lf_w)
    end_x = min(lf_x1 + 2, lf_w)
    copy_width = end_x - start_x
    n = lf_x1 - lf_x0
    rows = min(GROUP_BLOCKS, lf_h - lf_y0)
    storage = np.zeros((5, 256 // 8 + 32), np.float32)  # input_rows_storage
    out = []
    for c in range(3):
        img = lf[c]
        res = np.zeros((rows * 8, n * 8), np.float32)
        for y in range(rows):  # (the rows beyond the image are computed and dropped by the reference)
            cy = lf_y0 + y
            for dy in range(-2, 3):
                iy = _mirror(cy + dy, lf_h)
                s = storage[dy + 2]
                save_start = 2 if start_x == lf_x0 else 0
                save_end = save_start + copy_width
                s[save_start:save_end] = img[iy, start_x:end_x]
                if start_x == lf_x0:
                    s[0] = s[2 + _mirror(-2, copy_width)]
                    s[1] = s[2 + _mirror(-1, copy_width)]
                if end_x == lf_x1:
                    s[save_end] = s[save_start + _mirror(save_end, save_end)]
                    s[save_end + 1] = s[save_start + _mirror(save_end + 1, save_end)]
            # process_row_chunk((0, 0), n, ..): pixel x reads scratch columns x .. x + 4 of the five rows.  The oracle's
            # upsample on the 5 x (n + 4) window image computes exactly that for its centre row's columns 2 .. n + 2.
            big = o.upsample(8, np.ascontiguousarray(storage[:, :n + 4]), weights8)
            res[y * 8:(y + 1) * 8] = big[16:24, 16:16 + 8 * n]
        out.append(res)
    return out
