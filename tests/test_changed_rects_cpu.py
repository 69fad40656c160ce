"""jxlh_changed_rects (host code, through ctypes) against a Python statement of its rule -- merging of horizontal
neighbours, clipping, duplicates, the cap / *n protocol, every status -- and its soundness on the oracle: after ALL
coefficients of the listed groups are replaced with large random values, every pixel of the oracle's frame that differs
lies inside the rects.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from helpers import run_oracle_frame

SIZES = [(600, 520), (264, 300)]  # 3 x 3 groups; a one-block-wide last column
# (gab, epf_iters) -> the stage list's reach: Gaborish 1, EPF0 3 (with three iterations only), EPF1 2, EPF2 1
STAGES = {"none": (False, 0, 0), "gab": (True, 0, 1), "epf1": (False, 1, 2), "gab_epf2": (True, 2, 4),
          "gab_epf3": (True, 3, 7)}
S420 = ((1, 0, 1), (1, 0, 1))


def frame_params(w, h, gab, epf, shifts=((0, 0, 0), (0, 0, 0))):
    from jxl_rs_amd import lib
    p = lib.FrameParams()
    assert lib.load().jxlh_default_frame_params(p, w, h) == lib.OK
    p.gab, p.epf_iters = int(gab), int(epf)
    for c in range(3):
        p.hshift[c], p.vshift[c] = shifts[0][c], shifts[1][c]
    return p


def rule(w, h, reach_x, reach_y, ids):
    """one rect per maximal run of listed horizontal neighbours of a group row, ascending; widened, clipped"""
    xg = (w + 255) // 256
    ids = sorted(set(int(i) for i in ids))
    out, i = [], 0
    while i < len(ids):
        j = i
        while j + 1 < len(ids) and ids[j + 1] == ids[j] + 1 and ids[j + 1] // xg == ids[i] // xg:
            j += 1
        gy, gx0, gx1 = ids[i] // xg, ids[i] % xg, ids[j] % xg + 1
        x0, x1 = max(0, gx0 * 256 - reach_x), min(w, gx1 * 256 + reach_x)
        y0, y1 = max(0, gy * 256 - reach_y), min(h, (gy + 1) * 256 + reach_y)
        out.append((x0, y0, x1 - x0, y1 - y0))
        i = j + 1
    return out


def runs(w, ids):
    """(group row, first group column, one past the last) of every maximal run of listed horizontal neighbours"""
    xg = (w + 255) // 256
    ids = sorted(set(int(i) for i in ids))
    out = []
    for g in ids:
        if out and out[-1][0] == g // xg and out[-1][2] == g % xg:
            out[-1][2] += 1
        else:
            out.append([g // xg, g % xg, g % xg + 1])
    return out


def group_sets(w, h):
    xg, yg = (w + 255) // 256, (h + 255) // 256
    n = xg * yg
    centre = (yg // 2) * xg + xg // 2
    return {"centre": [centre], "corner": [n - 1], "two_neighbours": [0, 1], "all": list(range(n))}


@pytest.mark.parametrize("w,h", SIZES)
def test_geometry_follows_the_rule(w, h):
    from jxl_rs_amd import lib
    xg, yg = (w + 255) // 256, (h + 255) // 256
    n = xg * yg
    rng = np.random.default_rng(w)
    lists = list(group_sets(w, h).values()) + [[], [0, 0, 0], [n - 1, 0], list(range(n))[::-1] * 2,
                                                 [xg - 1, xg] if n > xg else [0]]  # (last of a row, first of the next: two rects)
    lists += [list(rng.integers(0, n, size=int(rng.integers(1, 2 * n)))) for _ in range(40)]
    for name, (gab, epf, reach) in STAGES.items():
        for shifts, rx, ry in ((((0, 0, 0), (0, 0, 0)), reach, reach), (S420, reach + 1, reach + 1),
                               (((1, 0, 1), (0, 0, 0)), reach + 1, reach)):
            p = frame_params(w, h, gab, epf, shifts)
            for ids in lists:
                want = rule(w, h, rx, ry, ids)
                got = lib.changed_rects(p, ids)
                assert [tuple(int(v) for v in r) for r in got] == want, (name, shifts, ids)
                # a condition, not a measurement: no rect extends more than 8 pixels beyond its groups
                for (x0, y0, rw, rh), (gy, gx0, gx1) in zip(got.tolist(), runs(w, ids)):
                    assert x0 >= gx0 * 256 - 8 and y0 >= gy * 256 - 8, (name, ids)
                    assert x0 + rw <= min(w, gx1 * 256) + 8 and y0 + rh <= min(h, (gy + 1) * 256) + 8, (name, ids)
    # the reach itself never passes 8: the widest list with both axes sub-sampled
    assert max(r[2] for r in STAGES.values()) + 1 <= 8


def test_cap_protocol_and_statuses():
    from jxl_rs_amd import lib
    L = lib.load()
    INV, UNS = lib.ERR_INVALID_ARGUMENT, lib.ERR_UNSUPPORTED
    w, h = SIZES[0]
    p = frame_params(w, h, True, 2)
    ids = np.array([0, 2, 4, 8, 8], dtype=np.uint32)  # four rects
    want = rule(w, h, 4, 4, ids)
    assert len(want) == 4
    n = C.c_uint32(77)
    buf = np.full((8, 4), 0xdeadbeef, dtype=np.uint32)

    def call(pp, i, count, out, cap, nn):
        return L.jxlh_changed_rects(pp, None if i is None else i.ctypes.data, count, None if out is None else out.ctypes.data,
                                    cap, nn)
    # *n is always the number needed; too little room is an error that still sets it and writes nothing
    assert call(p, ids, len(ids), None, 0, C.byref(n)) == INV and n.value == 4
    n.value = 77
    assert call(p, ids, len(ids), buf, 3, C.byref(n)) == INV and n.value == 4 and np.all(buf == 0xdeadbeef)
    assert call(p, ids, len(ids), buf, 4, C.byref(n)) == lib.OK and n.value == 4
    assert [tuple(int(v) for v in r) for r in buf[:4]] == want and np.all(buf[4:] == 0xdeadbeef)
    assert call(p, ids, len(ids), buf, 8, C.byref(n)) == lib.OK and n.value == 4
    assert call(p, ids, 0, None, 0, C.byref(n)) == lib.OK and n.value == 0          # no groups: no rects
    assert call(p, None, 0, None, 0, C.byref(n)) == lib.OK and n.value == 0
    st, rects, need = lib.try_changed_rects(p, ids, cap=2)
    assert (st, rects, need) == (INV, None, 4)
    # null pointers
    assert call(None, ids, len(ids), buf, 8, C.byref(n)) == INV
    assert call(p, None, 1, buf, 8, C.byref(n)) == INV
    assert call(p, ids, len(ids), None, 8, C.byref(n)) == INV
    assert call(p, ids, len(ids), buf, 8, None) == INV
    # a wrong abi_version; an id beyond the frame's nine groups
    q = frame_params(w, h, True, 2)
    q.abi_version += 1
    assert call(q, ids, len(ids), buf, 8, C.byref(n)) == INV
    assert call(p, np.array([9], dtype=np.uint32), 1, buf, 8, C.byref(n)) == INV
    assert call(p, np.array([0, 0xffffffff], dtype=np.uint32), 2, buf, 8, C.byref(n)) == INV
    assert call(p, np.array([8], dtype=np.uint32), 1, buf, 8, C.byref(n)) == lib.OK
    # where jxlh_frame_rerender_groups is unsupported from the parameters alone
    q = frame_params(w, h, True, 2)
    q.upsampling = 2
    assert call(q, ids, len(ids), buf, 8, C.byref(n)) == UNS
    for up in (0, 1):
        q.upsampling = up
        assert call(q, ids, len(ids), buf, 8, C.byref(n)) == lib.OK
    q.flags |= lib.FRAME_MODULAR
    assert call(q, ids, len(ids), buf, 8, C.byref(n)) == UNS


def soundness_cases():
    from jxl_rs_amd import synth
    out = []
    for w, h in SIZES:
        for name, (gab, epf, _) in STAGES.items():
            out.append((f"{w}x{h}_{name}", w, h, dict(mix=synth.MIX_D1, gab=gab, epf_iters=epf)))
    # 4:2:0, 8x8 DCTs only, with the widest filter list and with none
    out.append(("600x520_420_gab_epf2", 600, 520, dict(mix=synth.MIX_DCT8, gab=True, epf_iters=2, hshift=S420[0], vshift=S420[1])))
    out.append(("600x520_420_none", 600, 520, dict(mix=synth.MIX_DCT8, gab=False, epf_iters=0, hshift=S420[0], vshift=S420[1])))
    return out


def scramble_groups(wl, ids, rng):
    """the workload with ALL coefficients of the listed groups replaced by large random values (a sub-sampled channel
    keeps the zeros of the blocks it does not hold: a decoder never writes those)"""
    import copy
    new = copy.copy(wl)
    new.coeffs = wl.coeffs.copy()
    hs, vs = wl.opts.get("hshift", (0, 0, 0)), wl.opts.get("vshift", (0, 0, 0))
    for g in ids:
        slab = rng.integers(-3000, 3001, size=(3, 65536)).astype(np.int32)
        if any(hs) or any(vs):  # 8x8 blocks in raster order of the group's own block grid
            gx, gy = g % wl.xgroups, g // wl.xgroups
            bw, bh = min(32, wl.xblocks - gx * 32), min(32, wl.yblocks - gy * 32)
            by, bx = np.divmod(np.arange(bw * bh), bw)
            for c in range(3):
                absent = ((bx % (1 << hs[c])) != 0) | ((by % (1 << vs[c])) != 0)
                blocks = slab[c, :bw * bh * 64].reshape(bw * bh, 64)
                blocks[absent] = 0
            slab[:, bw * bh * 64:] = 0
        new.coeffs[g] = slab
    return new


@pytest.mark.parametrize("name,w,h,kw", soundness_cases(), ids=[c[0] for c in soundness_cases()])
def test_changes_stay_inside_the_rects(oracle, name, w, h, kw):
    from jxl_rs_amd import lib, synth
    wl = synth.make_vardct(w, h, seed=5, **kw)
    before, _ = run_oracle_frame(oracle, wl)
    p = frame_params(w, h, kw["gab"], kw["epf_iters"], (kw.get("hshift", (0, 0, 0)), kw.get("vshift", (0, 0, 0))))
    rng = np.random.default_rng(len(name))
    for sname, ids in group_sets(w, h).items():
        after, _ = run_oracle_frame(oracle, scramble_groups(wl, ids, rng))
        differ = np.zeros((h, w), dtype=bool)
        for a, b in zip(before, after):
            differ |= a.view(np.uint32) != b.view(np.uint32)
        inside = np.zeros((h, w), dtype=bool)
        for x0, y0, rw, rh in lib.changed_rects(p, ids):
            inside[y0:y0 + rh, x0:x0 + rw] = True
        assert differ.any(), (name, sname)  # the scramble did change the frame
        outside = differ & ~inside
        assert not outside.any(), (name, sname, int(outside.sum()), np.argwhere(outside)[:5].tolist())
