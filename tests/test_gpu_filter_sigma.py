"""The fused Gaborish / EPF kernel, the per-stage kernels and the strip kernel's filter stages against the CPU oracle,
bit for bit, over the sigma-map populations of tests/filter_sigma_cases.py: masks that put the fused kernel's
wavefronts into each of the three forms of an EPF stage (identity, dense, compacted) and onto both sides of each
threshold, at frame sizes on the tile seams, under all seven stage lists.  Which form a case reaches is proven on the
CPU (tests/test_filter_sigma_cases_cpu.py); a failure here names the wavefront the model puts the first bad pixel in."""
import ctypes as C

import numpy as np
import pytest

import filter_sigma_cases as F
from helpers import DeviceArray, bit_equal, diff_report, run_oracle_frame, upload_frame

pytestmark = pytest.mark.gpu
UNFUSED, STRIP = 1, 4  # JXLH_FRAME_UNFUSED_FILTERS, JXLH_FRAME_STRIP
PATHS = [("fused", 0), ("per-stage", UNFUSED), ("strip", STRIP)]


@pytest.fixture(scope="module")
def ctx():
    from jxl_rs_amd import Context
    c = Context(0, n_slots=1)
    yield c
    c.close()


def _hold(got, want, what, wh, mask, gab, epf, rows=None, **band):
    """all three planes bit for bit; on a mismatch: mask, path, plane, and the model's wavefront of the first bad pixel"""
    w, h = wh
    r0, r1 = rows if rows else (0, h)
    for c in range(3):
        g, t = np.ascontiguousarray(got[c][r0:r1]), np.ascontiguousarray(want[c][r0:r1])
        if bit_equal(g, t):
            continue
        y, x = np.argwhere(g.view(np.uint32) != t.view(np.uint32))[0].tolist()
        pytest.fail(f"{what}, plane {c}: {diff_report(g, t)}; first bad pixel (x {x}, y {y + r0}): "
                    f"{F.locate(gab, epf, w, h, mask, x, y + r0, **band)}")


def _strip_applies(wk, epf):
    return epf <= 2  # (every workload here has aligned varblocks)


@pytest.mark.parametrize("gab,epf", F.STAGE_LISTS, ids=lambda v: str(v))
@pytest.mark.parametrize("wk", F.WORKLOADS, ids=lambda wk: wk.key)
def test_sigma_masks_vs_oracle(ctx, oracle, wk, gab, epf):
    """every mask of the workload under one stage list, on the fused path, the per-stage path and the strip kernel: the
    coefficients go up once per path, only the maps are replaced between masks"""
    masks = F.case_masks(wk)
    frames = {name: F.with_mask(wk, name, mask, gab, epf) for name, mask in masks.items()}
    want = {name: run_oracle_frame(oracle, wl, num_threads=16)[0] for name, wl in frames.items()}
    for path, flags in PATHS:
        strip = flags == STRIP
        if strip and not _strip_applies(wk, epf):
            continue
        upload_frame(ctx, next(iter(frames.values())), flags=flags)
        for name, wl in frames.items():
            ctx.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)
            ctx.frame_run()
            ctx.sync()
            assert ctx.frame_path()[0] == strip, f"{wk.key} {name}: the strip kernel did{'' if not strip else ' not'} run"
            _hold(ctx.read_planes(), want[name], f"{wk.key} gab{gab} epf{epf}, mask {name}, {path} path", (wk.w, wk.h),
                  masks[name], gab, epf)


@pytest.mark.parametrize("epf", [2, 3])
def test_band_runs_on_sigma_masks(ctx, oracle, epf):
    """jxlh_frame_run(1, 2) on 200 x 520: the tiles start at the band's first row (256), and epf_iters = 3 widens the
    first pass to rows [252, 515) -- the band's rows equal the whole frame's"""
    wk, gab = F.BAND, 1
    masks = F.case_masks(wk)
    frames = {name: F.with_mask(wk, name, masks[name], gab, epf) for name in ("ramp_x", "cols_p1")}
    want = {name: run_oracle_frame(oracle, wl, num_threads=16)[0] for name, wl in frames.items()}
    for path, flags in PATHS[:2]:
        upload_frame(ctx, frames["ramp_x"], flags=flags)
        for name, wl in frames.items():
            ctx.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)
            ctx.frame_run(1, 2)
            ctx.sync()
            _hold(ctx.read_planes(), want[name], f"{wk.key} epf{epf}, mask {name}, {path} path, band rows 256..512",
                  (wk.w, wk.h), masks[name], gab, epf, rows=(256, 512), y0=256, y1=512)


def _modular_planes(w, h, stride, seed):
    """low-contrast content with edges every 16 columns: the EPF weights are neither all zero nor all one"""
    rng = np.random.default_rng([0x4D53, seed, w, h])
    planes = [np.zeros((h, stride), np.float32) for _ in range(3)]
    for c in range(3):
        amp = 0.004 if c == 0 else 0.03
        planes[c][:, :w] = (0.4 + amp * rng.random((h, w)) + 2 * amp * (np.arange(w) // 16 % 2)[None, :]).astype(np.float32)
    return planes


@pytest.mark.parametrize("size", F.SEAM_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_modular_filters_at_the_tile_seams(ctx, oracle, size):
    """jxlh_modular_frame_filters (raster input, one active sigma for every block) at the seam sizes, all stage lists"""
    w, h = size
    stride = (w + 3) // 4 * 4
    planes = _modular_planes(w, h, stride, 1)
    all_active = np.ones(((h + 7) // 8, (w + 7) // 8), bool)
    sigma = np.full(all_active.shape, np.float32(-1.1715728752538099024) / np.float32(0.7), dtype=np.float32)
    for gab, epf in F.STAGE_LISTS:
        p = ctx.default_params(w, h)
        p.epf_iters, p.gab = epf, gab
        p.epf_sigma_for_modular = 0.7
        po = oracle.default_params(w, h)
        po.epf_iters, po.gab = epf, gab
        cur = [pl[:, :w].copy() for pl in planes]
        if gab:
            cur = [oracle.gaborish(cur[c], po.gab_w1[c], po.gab_w2[c]) for c in range(3)]
        for stage, need in ((0, 3), (1, 1), (2, 2)):
            if epf >= need:
                cur = oracle.epf(stage, po, cur, sigma)
        tin = [DeviceArray(pl) for pl in planes]
        tout = [DeviceArray(nbytes=h * stride * 4) for _ in range(3)]
        try:
            vin = (C.c_void_p * 3)(*[t.ptr for t in tin])
            vout = (C.c_void_p * 3)(*[t.ptr for t in tout])
            ctx._chk(ctx.L.jxlh_modular_frame_filters(ctx._ctx, C.byref(p), vin, vout, w, h, stride), "modular_frame_filters")
            ctx.sync()
            got = [t.download(np.float32, h * stride).reshape(h, stride)[:, :w] for t in tout]
        finally:
            for t in tin + tout:
                t.free()
        _hold(got, cur, f"modular {w}x{h} gab{gab} epf{epf}, fused path", size, all_active, gab, epf, modular=True)
