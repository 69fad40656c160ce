"""The sigma-map cases of tests/filter_sigma_cases.py, checked without a GPU: the model's constants are the kernel's,
every case's maps give exactly its mask, the case list reaches every form of every EPF stage of every instantiation of
the fused kernel on both sides of its threshold (proven by the model), and the content is one on which the oracle's EPF
does something on active blocks and nothing on passing ones."""
import os
import re

import numpy as np
import pytest

import filter_sigma_cases as F
from helpers import oracle_params_from, run_oracle_frame

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "jxl_rs_amd", "csrc")
K_MIN_SIGMA = np.float32(-3.90524291751269967465540850526868)  # jxlh_internal.h: kMinSigma (jxl/src/lib.rs:28)


def test_geometry_pin():
    """the model's constants are the defaults of k_filters_fused.hip and k_filters_fused_tile.inc"""
    hip = open(os.path.join(CSRC, "k_filters_fused.hip")).read()
    inc = open(os.path.join(CSRC, "k_filters_fused_tile.inc")).read()
    got = {}
    for name in F.KERNEL:
        if name.startswith("JXLH_"):
            m = re.findall(r"^#ifndef %s\b.*\n#define %s (\d+)\s*$" % (name, name), hip, flags=re.M)
            assert len(m) == 1, f"{name}: expected one guarded default in k_filters_fused.hip, found {m}"
            got[name] = int(m[0])
    m = re.search(r"^constexpr int kTW = (\d+), kTH = JXLH_TILE_TH, kB = (\d+);", inc, flags=re.M)
    assert m, "k_filters_fused_tile.inc no longer declares kTW / kTH / kB on one line"
    got["kTW"], got["kB"] = int(m.group(1)), int(m.group(2))
    assert got == F.KERNEL, "the kernel's geometry changed: update filter_sigma_cases.KERNEL and the model with it"
    # the two geometries are instantiated from those macros, the EPF0 variants from JXLH_FUSED_E0_THREADS
    for ns, th, threads in (("tall", "JXLH_FUSED_TH", "JXLH_FUSED_THREADS"), ("low", "JXLH_FUSED_TH_LOW", "JXLH_FUSED_THREADS_LOW")):
        assert re.search(r"namespace %s \{\n#define JXLH_TILE_TH %s\n#define JXLH_TILE_THREADS %s\n" % (ns, th, threads), hip)
    assert "return E0 ? JXLH_FUSED_E0_THREADS : kThreadsDefault;" in inc
    assert "constexpr int kDenseItems = JXLH_DENSE_ITEMS, kDenseItems0 = JXLH_DENSE_ITEMS0, kSparseMax = JXLH_SPARSE_MAX;" in inc
    assert "dense = cnt > kSparseMax;" in inc and "cnt >= (STAGE == 3 ? kDenseItems0 : kDenseItems)" in inc


def test_stage_lists_pick_the_modelled_instantiations():
    names = {la.name for g, e in F.STAGE_LISTS for la in F.launches(g, e, 200, 232)}
    assert names == set(F.EPF_INSTANTIATIONS) | {"tall<G>"}
    assert len(F.STAGE_LISTS) == 7


def test_masks_are_what_the_maps_give(oracle):
    """oracle.sigma_map of the derived raw_quant / epf_map is not below kMinSigma on exactly the mask's blocks"""
    n = 0
    for wk in F.WORKLOADS + [F.BAND]:
        for name, mask in F.case_masks(wk).items():
            wl = F.with_mask(wk, name, mask, 1, 2)
            sigma = oracle.sigma_map(oracle_params_from(oracle, wl), wl.raw_quant, wl.epf_map)
            active = ~(sigma < K_MIN_SIGMA)
            assert np.array_equal(active, mask), f"{wk.key} {name}: {np.argwhere(active != mask)[:5].tolist()}"
            if wk.mix == "MIX_D1":
                assert (wl.raw_quant == 2).all()  # constant per varblock
            if mask.sum() > 64 and wk.mix == "MIX_DCT8":
                assert len(np.unique(sigma[mask])) >= 8, "active blocks carry different sigmas"
            n += 1
    assert n >= len(F.all_cases())


# ---------------------------------------------------------------------------------------------------------------------
# Targets the model proves unreachable AT ANY MASK, by instantiation (both tile classes).  test_reach verifies each
# entry against the model (an entry the model can reach is an error) and requires every other target.
UNREACHABLE = {
    # EPF1 as the only / last EPF stage has margin 0: its 4x2 items start on even rows of tiles that start on
    # multiples of 8, so both rows of an item always lie in the same block row.
    ("low<E1>", "sigma0_active_sigma1_pass"), ("low<E1>", "sigma0_pass_sigma1_active"),
    ("low<G,E1>", "sigma0_active_sigma1_pass"), ("low<G,E1>", "sigma0_pass_sigma1_active"),
    # ... and its 192 items fill three wavefronts exactly.
    ("low<E1>", "partial_wavefront"), ("low<G,E1>", "partial_wavefront"),
    # EPF0 works on single-row strips, 384 of them per tile: six whole 64-strip chunks, no row pairs.
    ("low<E0>", "sigma0_active_sigma1_pass"), ("low<E0>", "sigma0_pass_sigma1_active"), ("low<E0>", "partial_wavefront"),
    ("low<G,E0>", "sigma0_active_sigma1_pass"), ("low<G,E0>", "sigma0_pass_sigma1_active"), ("low<G,E0>", "partial_wavefront"),
    # EPF2's chunks cover four rows of one block row: counts are multiples of 4, at most 36 below the threshold of 40.
    # Low tile: 6 chunks x 36 = 216 <= 256 threads.  Tall tile: 14 x 36 = 504 <= 512 threads.  (EPF0's 128-thread
    # workgroups do outgrow: 216 > 128.)
    ("low<E1,E2>", "long_list_epf2"), ("low<G,E1,E2>", "long_list_epf2"), ("tall<E1,E2>", "long_list_epf2"),
}


@pytest.fixture(scope="module")
def reach_report():
    """per (instantiation, edge tile?): what the union of the cases reaches, and what the model says any mask could"""
    rep = {}

    def entry(sr, edge):
        return rep.setdefault((sr.launch.name, edge), dict(stages={}, partial=False, partial_possible=False, tiled=set()))

    def stage(e, sr):
        return e["stages"].setdefault(sr.kind, dict(counts=set(), possible=set(), longest=0, list_len=0, m01=False, m10=False,
                                                     straddle=False, threads=sr.launch.threads))

    # what is possible: at the sizes of the cases, any mask
    for w, h in sorted({(wk.w, wk.h) for wk in F.WORKLOADS}):
        for gab, epf in F.STAGE_LISTS:
            for sr in F.reach(gab, epf, w, h, np.zeros(((h + 7) // 8, (w + 7) // 8), bool)):
                for edge in (False, True):
                    sel = sr.geom["edge"] == edge
                    if not sel.any():
                        continue
                    e = entry(sr, edge)
                    s = stage(e, sr)
                    counts, longest = F.reachable_counts(sr, edge)
                    s["possible"] |= counts
                    s["longest"] = max(s["longest"], longest)
                    live = sr.geom["live"]
                    e["partial_possible"] |= bool(((live.sum(axis=1) > 0) & (live.sum(axis=1) < 64)).any())
                    if sr.kind == F.EPF1:
                        sy = sr.geom["sy"][sel]
                        s["straddle"] |= bool(((sy[..., 0] != sy[..., 1]) & live[None]).any())
    # what the cases reach
    for wk, name, mask in F.all_cases():
        for gab, epf in F.STAGE_LISTS:
            for sr in F.reach(gab, epf, wk.w, wk.h, mask):
                for edge in (False, True):
                    sel = sr.geom["edge"] == edge
                    if not sel.any():
                        continue
                    e = entry(sr, edge)
                    s = stage(e, sr)
                    e["tiled"].add(sr.launch.tiled)
                    s["counts"] |= set(sr.counts[sel].reshape(-1).tolist())
                    s["m01"] |= bool(sr.mixed01[sel].any())
                    s["m10"] |= bool(sr.mixed10[sel].any())
                    s["list_len"] = max(s["list_len"], int(sr.list_len[sel].max()))
                    part = (sr.geom["live"].sum(axis=1) > 0) & (sr.geom["live"].sum(axis=1) < 64)
                    e["partial"] |= bool((sr.counts[sel][:, part] > 0).any())
    return rep


def test_reach(reach_report):
    """For every instantiation with an EPF stage that launch_fused_filters can pick, on edge and on interior tiles, the
    cases reach all three forms of every EPF stage, the largest reachable count on the compacted side and the smallest
    on the dense side of every threshold, row pairs with sigma0 != sigma1 in both orders, a partially live last
    wavefront with active strips and a compacted list longer than the workgroup -- or the model proves the target
    unreachable at any mask and UNREACHABLE names it."""
    missing, wrongly_allowed, used = [], [], set()

    def check(inst, edge, target, reached, possible, shown):
        print(f"  {target:32s} {'reached' if reached else 'UNREACHABLE (model)' if not possible else 'MISSED'}  {shown}")
        if (inst, target) in UNREACHABLE:
            used.add((inst, target))
            if possible:
                wrongly_allowed.append((inst, edge, target))
        elif not reached:
            missing.append((inst, edge, target))

    for inst in F.EPF_INSTANTIATIONS:
        for edge in (False, True):
            assert (inst, edge) in reach_report, f"no {'edge' if edge else 'interior'} tile of {inst} at any case's size"
            e = reach_report[(inst, edge)]
            print(f"{inst} {'edge' if edge else 'interior'} tiles, input {'/'.join('tiled' if t else 'raster' for t in sorted(e['tiled']))}:")
            m01 = m10 = straddle = False
            for kind, s in sorted(e["stages"].items()):
                thr = F.DENSE_FROM[kind]
                lo, hi = max(c for c in s["possible"] if c < thr), min(c for c in s["possible"] if c >= thr)
                c = s["counts"]
                got_lo, got_hi = max(x for x in c if x < thr), min([x for x in c if x >= thr] or [None])
                tag = f"epf{kind}"
                check(inst, edge, f"identity_{tag}", 0 in c, True, "")
                check(inst, edge, f"compacted_{tag}", any(0 < x < thr for x in c), True, "")
                check(inst, edge, f"dense_{tag}", any(x >= thr for x in c), True, "")
                check(inst, edge, f"threshold_compacted_side_{tag}", got_lo == lo, True, f"count {got_lo} (largest reachable {lo}, dense from {thr})")
                check(inst, edge, f"threshold_dense_side_{tag}", got_hi == hi, True, f"count {got_hi} (smallest reachable {hi})")
                if kind != F.EPF1:
                    check(inst, edge, f"long_list_{tag}", s["list_len"] > s["threads"], s["longest"] > s["threads"],
                          f"list {s['list_len']} (bound at any mask {s['longest']}) vs {s['threads']} threads")
                else:
                    m01, m10, straddle = m01 | s["m01"], m10 | s["m10"], straddle | s["straddle"]
            check(inst, edge, "sigma0_active_sigma1_pass", m01, straddle, "")
            check(inst, edge, "sigma0_pass_sigma1_active", m10, straddle, "")
            check(inst, edge, "partial_wavefront", e["partial"], e["partial_possible"], "")
    assert not wrongly_allowed, f"UNREACHABLE names targets the model can reach: {wrongly_allowed}"
    assert not missing, f"the case list does not reach: {missing}"
    assert used == UNREACHABLE, f"stale entries in UNREACHABLE: {sorted(UNREACHABLE - used)}"


def test_model_counts_against_a_direct_transcription():
    """the vectorised model against a lane-by-lane loop written from the kernel's text, on one ragged mask"""
    wk = F.FULL_SIZE[0]
    w, h = wk.w, wk.h
    mask = F.case_masks(wk)["ramp_x"]
    for gab, epf in ((1, 2), (0, 3)):
        for sr in F.reach(gab, epf, w, h, mask):
            la = sr.launch
            tiles_x = (w + 55) // 56
            for tile in (0, tiles_x + 1, sr.counts.shape[0] - 1):
                tx0, ty0 = (tile % tiles_x) * 56, la.y0 + (tile // tiles_x) * la.th
                blk = lambda fx, fy: mask[min(max(fy, 0), h - 1) >> 3, min(max(fx, 0), w - 1) >> 3]
                if sr.kind == F.EPF1:
                    n = (la.th + 2 * sr.margin) // 2 * 16
                    want = [0] * ((n + 63) // 64)
                    for t in range(n):
                        by, bx0 = 4 - sr.margin + (t // 16) * 2, (t % 16) * 4
                        fy, fx0 = ty0 - 4 + by, tx0 - 4 + bx0
                        want[t // 64] += int(blk(fx0, fy)) + int(blk(fx0, fy + 1))
                else:
                    ns, kT, want = la.th * 16, la.threads, []
                    for t0 in range(0, ns, kT):
                        for b in range(0, kT, 64):
                            if t0 + b >= ns:
                                break
                            want.append(sum(int(blk(tx0 - 4 + (t % 16) * 4, ty0 + t // 16)) for t in range(t0 + b, min(t0 + b + 64, ns))))
                assert sr.counts[tile].tolist() == want, (la.name, sr.kind, tile)


# ---------------------------------------------------------------------------------------------------------------------
def _changed_share(oracle, wk, only=None):
    """per case (all, or the masks named in `only`) and EPF stage list: passing blocks keep the bits of the frame
    without EPF; returns the smallest share of active-block pixels (any plane differs) the EPF changes, and where"""
    worst = (1.0, None)
    for name, mask in F.case_masks(wk).items():
        if only and name not in only:
            continue
        px = np.kron(mask.astype(np.uint8), np.ones((8, 8), np.uint8)).astype(bool)[:wk.h, :wk.w]
        for gab in (0, 1):
            base, _ = run_oracle_frame(oracle, F.with_mask(wk, name, mask, gab, 0))
            for epf in (1, 2, 3):
                got, _ = run_oracle_frame(oracle, F.with_mask(wk, name, mask, gab, epf))
                diff = np.zeros((wk.h, wk.w), bool)
                for c in range(3):
                    diff |= got[c].view(np.uint32) != base[c].view(np.uint32)
                assert not diff[~px].any(), f"{wk.key} {name} gab{gab} epf{epf}: the EPF changed a passing block"
                if px.any():
                    share = diff[px].mean()
                    if share < worst[0]:
                        worst = (share, (name, gab, epf))
    return worst


@pytest.mark.parametrize("wk", F.FULL_SIZE, ids=lambda wk: wk.key)
def test_oracle_content_is_filtered_where_active(oracle, wk):
    """Every pixel of a passing block keeps the bits of the same frame with epf_iters = 0; at least 90 % of the pixels
    of active blocks change.  (A condition on the content, chosen through coeff_scale: see filter_sigma_cases.)"""
    share, where = _changed_share(oracle, wk)
    print(f"{wk.key}: smallest changed share of active pixels {share:.3f} at {where}")
    assert share >= 0.90, (share, where)


def test_oracle_content_high_contrast_variant(oracle):
    """the high-contrast variant exists for the opposite reason: weights that clamp to zero next to weights near one.
    Passing blocks keep their bits on every mask; on the all-active frame (one 64-pixel block says little) between a
    tenth and nine tenths of the pixels change under every stage list."""
    wk = F.BY_KEY["dct8-200x232-contrast"]
    _changed_share(oracle, wk, only=[n for n in F.case_masks(wk) if n != "all_active"][::4])
    share, where = _changed_share(oracle, wk, only=["all_active"])
    print(f"{wk.key}: smallest changed share of active pixels {share:.3f} at {where}")
    assert 0.10 <= share < 0.90, (share, where)
