"""Sigma-map populations for the fused Gaborish / EPF kernel (k_filters_fused.hip + k_filters_fused_tile.inc), the
per-stage kernels and the strip kernel's filter stages -- and a CPU model of which FORM of an EPF stage every wavefront
of the fused kernel takes on them.

An EPF stage has three forms that must give the same bits: identity (no active strip in the wavefront), dense (one item
per lane, side taps through DPP row shifts) and compacted (active strips pushed to a list, processed by the generic code
with side taps from LDS).  Which one a wavefront takes depends on how many of its strips sit in 8x8 blocks whose
inv_sigma is not below kMinSigma.  The cases below are block-granular ACTIVE MASKS; `with_mask` turns one into the
raw_quant / epf_map of a synth.make_vardct workload.  The model (`reach`) transcribes the kernel's item -> strip map
and counts: it only proves which form a case reaches (tests/test_filter_sigma_cases_cpu.py) and names the wavefront
behind a failing pixel (tests/test_gpu_filter_sigma.py).  It never produces expected pixels: those are the oracle's.

Importing this file needs neither a GPU nor the oracle."""
import dataclasses
import zlib
from collections import namedtuple

import numpy as np

# ---------------------------------------------------------------------------------------------------------------------
# The kernel's geometry, as the model mirrors it.  test_filter_sigma_cases_cpu.py::test_geometry_pin reads the same
# names from the sources and fails when they differ: change the kernel's geometry -> update this block (and the model).
KERNEL = dict(
    kTW=56,                       # k_filters_fused_tile.inc: constexpr int kTW = 56, kTH = JXLH_TILE_TH, kB = 4;
    kB=4,                         #   (same line)
    JXLH_FUSED_TH=56,             # k_filters_fused.hip: #define JXLH_FUSED_TH 56            (tall tile)
    JXLH_FUSED_THREADS=512,       # k_filters_fused.hip: #define JXLH_FUSED_THREADS 512
    JXLH_FUSED_TH_LOW=24,         # k_filters_fused.hip: #define JXLH_FUSED_TH_LOW 24        (low tile)
    JXLH_FUSED_THREADS_LOW=256,   # k_filters_fused.hip: #define JXLH_FUSED_THREADS_LOW 256
    JXLH_FUSED_E0_THREADS=128,    # k_filters_fused.hip: #define JXLH_FUSED_E0_THREADS 128   (EPF0 variants)
    JXLH_SPARSE_MAX=64,           # k_filters_fused.hip: #define JXLH_SPARSE_MAX 64          (EPF1: dense when cnt > it)
    JXLH_DENSE_ITEMS=40,          # k_filters_fused.hip: #define JXLH_DENSE_ITEMS 40         (EPF2: dense when cnt >= it)
    JXLH_DENSE_ITEMS0=40,         # k_filters_fused.hip: #define JXLH_DENSE_ITEMS0 40        (EPF0: dense when cnt >= it)
)
TW, B = KERNEL["kTW"], KERNEL["kB"]
STRIPS = (TW + 2 * B) // 4        # kStrips: 16 strips of 4 pixels per staged row (kBW = kTW + 2 * kB = 64 floats)
WAVE = 64
GEOMS = {  # namespace -> (kTH, kThreadsDefault)
    "tall": (KERNEL["JXLH_FUSED_TH"], KERNEL["JXLH_FUSED_THREADS"]),
    "low": (KERNEL["JXLH_FUSED_TH_LOW"], KERNEL["JXLH_FUSED_THREADS_LOW"]),
}
EPF0, EPF1, EPF2 = 0, 1, 2        # StageList::Kind (run_plan.h)
# smallest active-strip count of a wavefront (EPF1: 128 strips; EPF2 / EPF0: a 64-strip chunk) that takes the dense form
DENSE_FROM = {EPF1: KERNEL["JXLH_SPARSE_MAX"] + 1, EPF2: KERNEL["JXLH_DENSE_ITEMS"], EPF0: KERNEL["JXLH_DENSE_ITEMS0"]}
IDENTITY, COMPACTED, DENSE = "identity", "compacted", "dense"

# the seven stage lists that do something: (gab, epf_iters)
STAGE_LISTS = [(g, e) for e in range(4) for g in (0, 1) if g or e]

# One launch of k23_fused_filters<GAB, E0, E1, E2>: name of the instantiation, tile height, workgroup size, the EPF
# stages as (kind, margin of the stage's output region), input layout, output rows [y0, y1) (tiles start at y0)
Launch = namedtuple("Launch", "name th threads stages tiled y0 y1")


def launches(gab, epf_iters, w, h, y0=0, y1=None, modular=False):
    """launch_fused_filters (k_filters_fused.hip) for output rows [y0, y1): which instantiations run, on which rows.
    modular: jxlh_modular_frame_filters / a Modular frame (raster input); otherwise K1 wrote the 8x8-tiled layout."""
    y1 = h if y1 is None else y1
    low, tall = GEOMS["low"], GEOMS["tall"]
    g = "G," if gab else ""
    tiled = not modular
    if epf_iters >= 3:
        # Gaborish + EPF0 on the band widened by 4 / 3 rows (low tile, 128 threads), then EPF1 + EPF2 (tall, raster)
        return [Launch(f"low<{g}E0>", low[0], KERNEL["JXLH_FUSED_E0_THREADS"], ((EPF0, 0),), tiled, max(0, y0 - 4), min(h, y1 + 3)),
                Launch("tall<E1,E2>", tall[0], tall[1], ((EPF1, 1), (EPF2, 0)), False, y0, y1)]
    if epf_iters == 2:
        return [Launch(f"low<{g}E1,E2>", low[0], low[1], ((EPF1, 1), (EPF2, 0)), tiled, y0, y1)]
    if epf_iters == 1:
        return [Launch(f"low<{g}E1>", low[0], low[1], ((EPF1, 0),), tiled, y0, y1)]
    return [Launch("tall<G>", tall[0], tall[1], (), tiled, y0, y1)] if gab else []


# every instantiation with an EPF stage that launch_fused_filters can pick
EPF_INSTANTIATIONS = ["low<E1>", "low<G,E1>", "low<E1,E2>", "low<G,E1,E2>", "low<E0>", "low<G,E0>", "tall<E1,E2>"]

_GEOM_CACHE = {}


def stage_geometry(launch, kind, margin, w, h):
    """Per tile and wavefront of one EPF stage: the block (row, column) each lane's strip(s) take their sigma from.
    Returns dict(edge [T], tiles (tiles_x, tiles_y), live [W, 64], sy [T, W, 64, R], sx [T, W, 64]): R = 2 rows per
    item for EPF1 (sigma0, sigma1), 1 for EPF2 / EPF0."""
    key = (launch.th, launch.threads, kind, margin, w, h, launch.y0, launch.y1)
    if key in _GEOM_CACHE:
        return _GEOM_CACHE[key]
    th, kT = launch.th, launch.threads
    tiles_x = (w + TW - 1) // TW
    tiles_y = (launch.y1 - launch.y0 + th - 1) // th
    ty0 = (launch.y0 + th * np.arange(tiles_y))[:, None].repeat(tiles_x, 1).reshape(-1)
    tx0 = (TW * np.arange(tiles_x))[None, :].repeat(tiles_y, 0).reshape(-1)
    edge = (tx0 - B < 0) | (ty0 - B < 0) | (tx0 + TW + B > w) | (ty0 + th + B > h)
    if kind == EPF1:
        # 4x2 items, one per thread: n = (rows / 2) * kStrips, item t: by = kB - margin + (t / kStrips) * 2
        rows = th + 2 * margin
        n = (rows // 2) * STRIPS
        assert n <= kT, "one EPF1 item per thread"
        lanes = [np.arange(b, b + WAVE) for b in range(0, n, WAVE)]
        t = np.stack(lanes)
        live = t < n
        tt = np.where(live, t, 0)
        fy = ty0[:, None, None] - margin + 2 * (tt // STRIPS)[None]
        fy = np.stack([fy, fy + 1], axis=-1)
    else:
        # strips of one row, kT at a time: t0 = 0, kT, ...; a wavefront whose first strip is past the end leaves
        ns = th * STRIPS
        lanes = [np.arange(t0 + b, t0 + b + WAVE) for t0 in range(0, ns, kT) for b in range(0, kT, WAVE) if t0 + b < ns]
        t = np.stack(lanes)
        live = t < ns
        tt = np.where(live, t, 0)
        fy = (ty0[:, None, None] + (tt // STRIPS)[None])[..., None]
    fx0 = tx0[:, None, None] - B + 4 * (tt % STRIPS)[None]
    g = dict(edge=edge, tiles=(tiles_x, tiles_y), live=live, tx0=tx0, ty0=ty0,
             sy=np.clip(fy, 0, h - 1) >> 3, sx=np.clip(fx0, 0, w - 1) >> 3)
    _GEOM_CACHE[key] = g
    return g


StageReach = namedtuple("StageReach", "launch kind margin geom counts forms mixed01 mixed10 list_len")


def reach(gab, epf_iters, w, h, mask, y0=0, y1=None, modular=False):
    """The model: for every EPF stage of every launch of the stage list, the active-strip count and form of every
    wavefront (EPF1) / 64-strip chunk (EPF2, EPF0) of every tile.  mask: bool [yblocks, xblocks], True = active.
    mixed01 / mixed10 [T, W]: the wavefront holds a row pair with (sigma0 active, sigma1 not) / the reverse.
    list_len [T]: the length of the tile's compacted list."""
    mask = np.asarray(mask, dtype=bool)
    out = []
    for la in launches(gab, epf_iters, w, h, y0, y1, modular):
        for kind, margin in la.stages:
            g = stage_geometry(la, kind, margin, w, h)
            act = mask[g["sy"], g["sx"][..., None]] & g["live"][None, :, :, None]
            counts = act.sum(axis=(2, 3))
            forms = np.where(counts == 0, 0, np.where(counts >= DENSE_FROM[kind], 2, 1))
            if kind == EPF1:
                m01 = (act[..., 0] & ~act[..., 1] & g["live"][None]).any(axis=2)
                m10 = (~act[..., 0] & act[..., 1] & g["live"][None]).any(axis=2)
            else:
                m01 = m10 = np.zeros(counts.shape, dtype=bool)
            list_len = np.where(forms == 1, counts, 0).sum(axis=1)
            out.append(StageReach(la, kind, margin, g, counts, forms, m01, m10, list_len))
    return out


FORM_NAMES = (IDENTITY, COMPACTED, DENSE)


def wave_weights(sr, tile, wave):
    """{block (row, column): strips of this wavefront that take their sigma from it}: the wavefront's count is the sum
    of the weights of its active blocks"""
    g = sr.geom
    live = g["live"][wave]
    sy, sx = g["sy"][tile, wave][live], g["sx"][tile, wave][live]
    wts = {}
    for r in range(sy.shape[-1]):
        for by, bx in zip(sy[:, r].tolist(), sx.tolist()):
            wts[(by, bx)] = wts.get((by, bx), 0) + 1
    return wts


def subset_sums(weights):
    """{reachable count: one set of blocks that gives it}"""
    sums = {0: ()}
    for blk, wt in sorted(weights.items()):
        for c, s in list(sums.items()):
            sums.setdefault(c + wt, s + (blk,))
    return sums


def reachable_counts(sr, edge):
    """every count some mask gives some wavefront of an edge / interior tile of this stage (by subset sums over the
    wavefront's block weights), and the largest compacted list any mask could give a tile (an upper bound: the
    wavefronts' best counts below the threshold need not be compatible)"""
    counts, longest, seen = set(), 0, {}
    for tile in np.flatnonzero(sr.geom["edge"] == edge).tolist():
        total = 0
        for wave in range(sr.counts.shape[1]):
            wts = wave_weights(sr, tile, wave)
            key = tuple(sorted(wts.values()))
            if key not in seen:
                seen[key] = set(subset_sums(wts))
            counts |= seen[key]
            total += max(c for c in seen[key] if c < DENSE_FROM[sr.kind])
        longest = max(longest, total)
    return counts, longest


def locate(gab, epf_iters, w, h, mask, x, y, y0=0, y1=None, modular=False):
    """Failure output: for output pixel (x, y), the wavefront of each EPF stage that classifies its strip, with form and
    count, e.g. 'low<G,E1,E2> EPF1 tile (1, 3) edge=False wave 2: compacted, 18 active strips'."""
    lines = []
    for sr in reach(gab, epf_iters, w, h, mask, y0, y1, modular):
        la, g = sr.launch, sr.geom
        tiles_x, tiles_y = g["tiles"]
        tx, ty = x // TW, (y - la.y0) // la.th
        if not (0 <= ty < tiles_y and tx < tiles_x):
            lines.append(f"{la.name} EPF{sr.kind}: pixel outside the launch's rows [{la.y0}, {la.y1})")
            continue
        tile = ty * tiles_x + tx
        col = (x - tx * TW + B) // 4
        if sr.kind == EPF1:
            t = ((y - (la.y0 + ty * la.th) + sr.margin) // 2) * STRIPS + col
            wave = t // WAVE
        else:
            t = (y - (la.y0 + ty * la.th)) * STRIPS + col
            kT = la.threads
            per_pass = [min(kT, la.th * STRIPS - t0) for t0 in range(0, la.th * STRIPS, kT)]
            wave = sum((n + WAVE - 1) // WAVE for n in per_pass[:t // kT]) + (t % kT) // WAVE
        lines.append(f"{la.name} EPF{sr.kind} tile ({tx}, {ty}) edge={bool(g['edge'][tile])} wave {wave}: "
                     f"{FORM_NAMES[sr.forms[tile, wave]]}, {int(sr.counts[tile, wave])} active strips, "
                     f"tile's compacted list {int(sr.list_len[tile])} of {la.threads} threads, "
                     f"{'tiled' if la.tiled else 'raster'} input")
    return "; ".join(lines) if lines else "no EPF stage"


# ---------------------------------------------------------------------------------------------------------------------
# masks
def _blocks(w, h):
    return (w + 7) // 8, (h + 7) // 8


def _single_positions(w, h):
    """block (row, column) of: the frame's corners, a tile interior, both sides of a vertical tile seam (x = 56), both
    sides of a horizontal seam of the low tile (y = 24) and of the tall tile (y = 56)"""
    xb, yb = _blocks(w, h)
    assert xb >= 11 and yb >= 9
    return {"corner_tl": (0, 0), "corner_br": (yb - 1, xb - 1), "interior": (4, 10), "vseam_l": (4, 6),
            "vseam_r": (4, 7), "hseam_low_a": (2, 9), "hseam_low_b": (3, 9), "hseam_tall_a": (6, 9),
            "hseam_tall_b": (7, 9)}


def _extra_columns(xb):
    """one odd block column per tile span of 7 block columns"""
    return [c for c in (7 * k + (3 if k % 2 == 0 else 4) for k in range((xb + 6) // 7)) if c < xb]


def basic_masks(w, h, reduced=False):
    """name -> bool [yblocks, xblocks] (True = active).  reduced: the short list of the seam sizes."""
    xb, yb = _blocks(w, h)
    yy, xx = np.mgrid[0:yb, 0:xb]
    rng = np.random.default_rng([0x5347, w, h])
    ramp_x = rng.random((yb, xb)) < xx / max(1, xb - 1)
    ramp_y = rng.random((yb, xb)) < yy / max(1, yb - 1)
    m = {"all_active": np.ones((yb, xb), bool), "cols_p1": xx % 2 == 0, "ramp_x": ramp_x}
    if reduced:
        return m
    m["all_pass"] = np.zeros((yb, xb), bool)
    for name, (by, bx) in _single_positions(w, h).items():
        one = np.zeros((yb, xb), bool)
        one[by, bx] = True
        m["one_active_" + name] = one
        m["one_pass_" + name] = ~one
    m["rows_p1"] = yy % 2 == 0
    m["rows_p2"] = (yy // 2) % 2 == 0
    plus = (xx % 2 == 0)
    plus[:, _extra_columns(xb)] = True
    m["cols_p1_plus"] = plus
    m["checker"] = (xx + yy) % 2 == 0
    m["ramp_y"] = ramp_y
    return m


def threshold_masks(w, h):
    """Masks built from the model: for every EPF stage of every stage list, and for edge and interior tiles, a
    wavefront whose count is the largest reachable one on the compacted side of the threshold, and one with the
    smallest on the dense side; for EPF2 / EPF0 tiles whose compacted list can outgrow the workgroup, such a tile.
    A target fixes the blocks its wavefront (tile) reads; targets whose blocks do not collide share a mask."""
    xb, yb = _blocks(w, h)
    masks, fixed = [], []  # fixed[i]: bool map of the blocks mask i has decided

    def place(active, touched):
        for m, f in zip(masks, fixed):
            if not any(f[b] for b in touched):
                break
        else:
            m, f = np.zeros((yb, xb), bool), np.zeros((yb, xb), bool)
            masks.append(m)
            fixed.append(f)
        for b in touched:
            f[b] = True
        for b in active:
            m[b] = True

    done = set()
    for gab, epf in STAGE_LISTS:
        for sr in reach(gab, epf, w, h, np.zeros((yb, xb), bool)):
            geo_key = (sr.launch.th, sr.launch.threads, sr.kind, sr.margin, sr.launch.y0, sr.launch.y1)
            if geo_key in done:  # (the same item map, e.g. with and without Gaborish)
                continue
            done.add(geo_key)
            thr = DENSE_FROM[sr.kind]
            for edge in (False, True):
                tiles = np.flatnonzero(sr.geom["edge"] == edge).tolist()
                if not tiles:
                    continue
                counts, longest = reachable_counts(sr, edge)
                lo, hi = max(c for c in counts if c < thr), min(c for c in counts if c >= thr)
                for want in (lo, hi):
                    for tile in tiles:
                        hit = next(((wts, s[want]) for wave in range(sr.counts.shape[1])
                                    for wts in [wave_weights(sr, tile, wave)] for s in [subset_sums(wts)] if want in s), None)
                        if hit:
                            place(hit[1], list(hit[0]))
                            break
                if sr.kind != EPF1 and longest > sr.launch.threads:
                    # a tile whose every wavefront sits just below the threshold: block by block, greedily
                    for tile in tiles:
                        touched, active = {}, set()
                        waves = [wave_weights(sr, tile, wv) for wv in range(sr.counts.shape[1])]
                        for wts in waves:
                            touched.update(wts)
                        cnt = [0] * len(waves)
                        for blk in sorted(touched):
                            if all(cnt[i] + wts.get(blk, 0) < thr for i, wts in enumerate(waves)):
                                active.add(blk)
                                cnt = [c + wts.get(blk, 0) for c, wts in zip(cnt, waves)]
                        if sum(cnt) > sr.launch.threads:
                            place(active, list(touched))
                            break
    return {f"model_{i}": m for i, m in enumerate(masks)}


def masks_for(w, h, reduced=False):
    m = basic_masks(w, h, reduced)
    if not reduced:
        m.update(threshold_masks(w, h))
    return m


# ---------------------------------------------------------------------------------------------------------------------
# workloads
# The content.  An active sigma needs raw_quant 1..3, the coarsest quantisation steps there are, and an EPF weight is
# max(0, 1 + SAD * inv_sigma): with make_vardct's coefficient law at coeff_scale = 1 nearly every weight clamps to zero
# and EPF1 is the identity on 93 % of the pixels of an all-active frame.  coeff_scale alone does not mend that: it
# multiplies the integer coefficients and stores them as integers again, so a small scale only thins them out (0.2
# keeps one in sixteen, as +-1).  Blocks left without a coefficient are flat -- the EPF changes nothing in their
# interior -- while a +-1 at a high frequency is still a step large enough to clamp; measured on the oracle, EPF1 alone
# changes at most about 80 % of the active pixels at any scale (0.12: 72 %, 0.2: 80 %, 0.25: 72 %, 0.3: 70 %), and a
# single active block anything from 0 to 100 %.  So the low-contrast content takes coeff_scale = 0 (no coefficient of
# make_vardct's law survives; transform map, LF and colour maps are make_vardct's) and puts one +-1 luma coefficient
# per covered 8x8 block at a low frequency (below 3 cycles per 8 pixels, outside the LLF corner): every pixel has a
# gradient, no step clamps, and the oracle's EPF changes >= 90 % of the pixels of active blocks under every stage
# list (test_filter_sigma_cases_cpu.py).  The high-contrast variant is make_vardct's own law at coeff_scale = 0.5:
# weights anywhere in [0, 1], most of them clamped.
LOW_CONTRAST, HIGH_CONTRAST = 0, 0.5
Workload = namedtuple("Workload", "key w h mix coeff_scale reduced")
FULL_SIZE = [
    Workload("dct8-200x232", 200, 232, "MIX_DCT8", LOW_CONTRAST, False),  # low tile: 4 x 10 tiles, last column partial
    Workload("d1-176x520", 176, 520, "MIX_D1", LOW_CONTRAST, False),      # tall tile: 4 x 10 tiles
]
VARIANTS = [
    Workload("dct8-200x232-contrast", 200, 232, "MIX_DCT8", HIGH_CONTRAST, False),
    Workload("d1-200x232", 200, 232, "MIX_D1", LOW_CONTRAST, False),
]
# tile seams: w % 56 in {0, 1, 3}, h % 24 in {0, 1} and h % 56 in {0, 1}
SEAM_SIZES = [(57, 25), (113, 49), (56, 24), (112, 56), (59, 57)]
SEAMS = [Workload(f"{'dct8' if i % 2 == 0 else 'd1'}-{w}x{h}", w, h, "MIX_DCT8" if i % 2 == 0 else "MIX_D1", LOW_CONTRAST, True)
         for i, (w, h) in enumerate(SEAM_SIZES)]
BAND = Workload("d1-200x520", 200, 520, "MIX_D1", LOW_CONTRAST, True)
WORKLOADS = FULL_SIZE + VARIANTS + SEAMS
BY_KEY = {wk.key: wk for wk in WORKLOADS + [BAND]}

_BASE = {}


def base_workload(wk):
    """the content: coefficients, transform map, LF and colour maps of synth.make_vardct (aligned varblocks, so that
    the strip kernel takes the frame); raw_quant and epf_map are replaced per mask"""
    from jxl_rs_amd import synth
    if wk.key not in _BASE:
        wl = synth.make_vardct(wk.w, wk.h, mix=getattr(synth, wk.mix), seed=CONTENT_SEED, coeff_scale=wk.coeff_scale,
                               aligned=True)
        _BASE[wk.key] = wl if wk.coeff_scale else low_frequency_texture(wl, CONTENT_SEED)
    return _BASE[wk.key]


CONTENT_SEED = 1


def low_frequency_texture(wl, seed):
    """one +-1 Y coefficient per covered block of every varblock, at a frequency below 3 cycles per 8 pixels in each
    direction and outside the LLF corner (which the LF overwrites); the slabs hold the varblocks back to back in
    raster order of their top-left blocks, each as [min side, max side] coefficients in natural order"""
    from jxl_rs_amd import synth
    assert not wl.coeffs.any()
    rng = np.random.default_rng([0x5458, seed, wl.xsize, wl.ysize])
    coeffs = np.zeros_like(wl.coeffs)
    xg = wl.xgroups
    for g in range(coeffs.shape[0]):
        bx0, by0 = (g % xg) * 32, (g // xg) * 32
        tm = wl.transform_map[by0:by0 + 32, bx0:bx0 + 32]
        off = 0
        for by, bx in np.argwhere(tm & 0x80).tolist():
            t = int(tm[by, bx] & 127)
            cx, cy = synth.COVERED_X[t], synth.COVERED_Y[t]
            lo, hi = min(cx, cy), max(cx, cy)
            for _ in range(cx * cy):
                while True:
                    r, c = int(rng.integers(0, 3 * lo)), int(rng.integers(0, 3 * hi))
                    if r >= lo or c >= hi:
                        break
                coeffs[g, 1, off + r * hi * 8 + c] = 1 if rng.random() < 0.5 else -1
            off += cx * cy * 64
    return dataclasses.replace(wl, coeffs=coeffs)


def derive_maps(wk, name, mask):
    """raw_quant / epf_map that make exactly the blocks of `mask` active (default header parameters: raw_quant 1 is
    active from epf_map 2, raw_quant 2 from 4, raw_quant 3 from 5, raw_quant >= 5 never).  Active blocks draw epf_map
    from 4..7 and, on DCT8 content, raw_quant from 1..3 (the pair (3, 4) passes through: it becomes (3, 5)), so that
    neighbouring active strips carry different sigmas.  MIX_D1 content keeps raw_quant = 2 everywhere (it is constant
    per varblock) and passes through with epf_map 0..3; DCT8 content passes with that or with raw_quant 5..16."""
    mask = np.asarray(mask, dtype=bool)
    rng = np.random.default_rng([0x5347, wk.w, wk.h, zlib.crc32(name.encode())])
    shape = mask.shape
    epf_act = rng.integers(4, 8, size=shape)
    epf_pass_lo = rng.integers(0, 4, size=shape)
    if wk.mix == "MIX_DCT8":
        rq_act = rng.integers(1, 4, size=shape)
        epf_act = np.where((rq_act == 3) & (epf_act == 4), 5, epf_act)
        coarse = rng.random(shape) < 0.5
        rq_pass = np.where(coarse, rng.integers(5, 17, size=shape), 2)
        epf_pass = np.where(coarse, rng.integers(0, 8, size=shape), epf_pass_lo)
    else:
        rq_act = rq_pass = np.full(shape, 2)
        epf_pass = epf_pass_lo
    return (np.where(mask, rq_act, rq_pass).astype(np.int32), np.where(mask, epf_act, epf_pass).astype(np.uint8))


def with_mask(wk, name, mask, gab, epf_iters):
    base = base_workload(wk)
    rq, em = derive_maps(wk, name, mask)
    assert rq.shape == base.raw_quant.shape
    return dataclasses.replace(base, raw_quant=rq, epf_map=em, opts=dict(base.opts, gab=bool(gab), epf_iters=epf_iters))


_MASKS = {}


def case_masks(wk):
    if wk.key not in _MASKS:
        _MASKS[wk.key] = masks_for(wk.w, wk.h, wk.reduced)
    return _MASKS[wk.key]


def all_cases():
    """(workload, mask name, mask) of every case; each runs under the seven stage lists"""
    return [(wk, name, mask) for wk in WORKLOADS for name, mask in case_masks(wk).items()]
