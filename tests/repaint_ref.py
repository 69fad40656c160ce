"""What tests/test_repaint_cpu.py and tests/test_gpu_repaint.py share: the oracle's frame of a VarDCT or Modular workload
with upsampling and noise (jxlo_vardct_frame / the Modular stages, then jxlo_upsample and the noise functions, in the
reference's order), workloads whose listed groups come from another seed, and the cells of the 256 grid."""
import copy

import numpy as np

from helpers import run_oracle_frame

INV_SIGMA_NUM = np.float32(-1.1715728752538099024)  # features/epf.rs:26
NOISE_LUT = [0.05 + 0.01 * i for i in range(8)]
NOISE = dict(noise=1, visible_frame_index=3)
SIGMA_FOR_MODULAR = 0.7


def result_size(w, h, n, cut=None):
    """the result's (width, height): n times the coded size, or the smaller xsize_upsampled x ysize_upsampled"""
    return cut if cut else (w * n, h * n)


def finish(oracle, planes, n=1, noise=False, size=None):
    """Upsample<n> of the three colour planes, cut to the result's size, then the noise at that size"""
    cur = [np.ascontiguousarray(p) for p in planes]
    if n > 1:
        h, w = cur[0].shape
        ow, oh = size if size else (w * n, h * n)
        cur = [np.ascontiguousarray(oracle.upsample(n, p)[:oh, :ow]) for p in cur]
    if noise:
        h, w = cur[0].shape
        rnd = [oracle.noise_convolve(r) for r in oracle.noise_generate(3, 0, w, h)]
        cur = oracle.noise_add(np.float32(NOISE_LUT), 0.0, 1.0, cur, rnd)
    return cur


def vardct_result(oracle, wl, n=1, noise=False, size=None, coded=None):
    """coded: the coded-size planes where the caller has them already (LF fill)"""
    if coded is None:
        coded, _ = run_oracle_frame(oracle, wl)
    return finish(oracle, coded, n, noise, size)


def with_groups_from(wl, other, groups):
    """wl with the coefficients of `groups` taken from `other` (the same size and maps; another seed's coefficients)"""
    new = copy.copy(wl)
    new.coeffs = wl.coeffs.copy()
    for g in groups:
        new.coeffs[g] = other.coeffs[g]
    return new


def cell(w, h, g):
    """(x0, y0, x1, y1) of cell g of the 256 grid over a w x h frame"""
    xg = (w + 255) // 256
    gx, gy = g % xg, g // xg
    return gx * 256, gy * 256, min(w, gx * 256 + 256), min(h, gy * 256 + 256)


# ---- Modular frames: the route tests/test_gpu_modular_frame.py uses
def modular_samples(seed, w, h, n=3):
    """8-bit integer samples the filters act on (a slope, edges along the block grid, one step of noise)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        a = rng.integers(0, 2, size=(h, w)).astype(np.int64)
        a += (np.arange(w)[None, :] + 2 * np.arange(h)[:, None]) // 6 % 64
        a += 16 * ((np.arange(w) // 16 % 2)[None, :] ^ (np.arange(h) // 8 % 2)[:, None])
        out.append(a.astype(np.int32))
    return out


def modular_filters(oracle, planes, gab, epf):
    """Gaborish / EPF with SigmaSource::Constant"""
    h, w = planes[0].shape
    po = oracle.default_params(w, h)
    po.epf_iters, po.gab = epf, gab
    sigma = np.full(((h + 7) // 8, (w + 7) // 8), INV_SIGMA_NUM / np.float32(SIGMA_FOR_MODULAR), dtype=np.float32)
    cur = [np.ascontiguousarray(p) for p in planes]
    if gab:
        cur = [oracle.gaborish(cur[c], po.gab_w1[c], po.gab_w2[c]) for c in range(3)]
    for stage, need in ((0, 3), (1, 1), (2, 2)):
        if epf >= need:
            cur = oracle.epf(stage, po, cur, sigma)
    return cur


def modular_result(oracle, chans, gab=0, epf=0, n=1, noise=False, size=None):
    coded = modular_filters(oracle, [oracle.modular_to_f32(c, 8, 0) for c in chans], gab, epf)
    return finish(oracle, coded, n, noise, size)


def outside(rects, w, h):
    """boolean map [h, w]: True where no rect (x0, y0, w, h) covers the pixel"""
    m = np.ones((h, w), dtype=bool)
    for x0, y0, rw, rh in np.asarray(rects, dtype=np.int64).reshape(-1, 4):
        m[y0:y0 + rh, x0:x0 + rw] = False
    return m
