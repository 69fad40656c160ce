"""The cases of the blend-rectangle tests, shared by tests/test_blend_rects_cpu.py (which holds every frame case to the
non-vacuity rules on the oracle: a test must not be able to pass by writing nothing) and tests/test_gpu_blend_rects.py
(which runs them on the device).  A frame case is (desc, refs before, refs after, frame planes before, frame planes
after, image rects): the canvas is composed from "before", the inputs change to "after", and only the rects are composed
again.  Everything expected comes from the oracle and blending_ref.blend_frame."""
import numpy as np

import blending_ref as br
import patches_ref as pr
import repaint_ref as rr
from helpers import run_oracle_frame

ALPHA = pr.EC_ALPHA

# ---------------------------------------------------------------- the stage hook's geometry
STAGE_IMAGE = (517, 11)  # no multiple of 4; two full 256-pixel pieces and a ragged third; three rows of pieces, the last of 3
STAGE_FRAME = (300, 9)
STAGE_ORIGINS = [(-7, -2), (1, 1), (255, 3), (509, 8)]


def frame_box(x0, y0, fw, fh, iw, ih):
    """the frame cut to the image, in image coordinates: (ax, ay, bx, by), empty when ax >= bx or ay >= by"""
    return max(x0, 0), max(y0, 0), min(x0 + fw, iw), min(y0 + fh, ih)


def straddling(box, iw, ih):
    """one rect across each edge of the frame's box that lies inside the image"""
    ax, ay, bx, by = box
    out = []
    if 0 < ax < iw:
        out.append((max(ax - 2, 0), ay, 5, min(3, by - ay)))
    if 0 < bx < iw:
        out.append((bx - 3, ay, 5, min(3, by - ay)))
    if 0 < ay < ih:
        out.append((ax, ay - 1, min(9, bx - ax), 3))
    if 0 < by < ih:
        out.append((ax, by - 2, min(9, bx - ax), 4))
    return out


def meets(r, box):
    x0, y0, w, h = r
    return x0 < box[2] and x0 + w > box[0] and y0 < box[3] and y0 + h > box[1]


def stage_rects(x0, y0):
    """the hand-picked list for a STAGE_FRAME at (x0, y0) of a STAGE_IMAGE"""
    iw, ih = STAGE_IMAGE
    box = frame_box(x0, y0, *STAGE_FRAME, iw, ih)
    rects = [(0, 0, 1, 1),
             (3, 1, 2, 2),      # inside one lane's four pixels
             (253, 2, 7, 6)]    # across the piece seam
    rects += straddling(box, iw, ih)
    rects.append(next(r for r in [(400, 4, 9, 3), (10, 0, 30, 3), (100, 2, 20, 5)] if not meets(r, box)))  # extend only
    rects += [(516, 10, 1, 1),
              (100, 3, 40, 5), (120, 5, 40, 4),  # an overlapping pair
              (5, 5, 0, 3), (600, 20, 0, 0)]     # empty; the second starts outside the image
    return rects


def union_mask(rects, iw, ih):
    m = np.zeros((ih, iw), dtype=bool)
    for x0, y0, w, h in rects:
        if w and h:
            m[y0:y0 + h, x0:x0 + w] = True
    return m


def poison(nch, h, stride):
    """nch planes [h, stride] of quiet NaNs, every sample with a payload of its own"""
    n = h * stride
    return [(np.uint32(0x7fc00001) + np.arange(c * n, (c + 1) * n, dtype=np.uint32)).view(np.float32).reshape(h, stride)
            for c in range(nch)]


# ---------------------------------------------------------------- the frame cases
FRAME = (520, 300)  # 3 x 2 groups
IMAGE = (400, 280)
ORIGIN = (-7, 5)
STAGES = dict(epf_iters=2, gab=True)
GROUP = 1  # the group that arrives again: frame x 256..511, y 0..255

DESCS = {
    "blend_alpha": br.BlendDesc(ORIGIN[0], ORIGIN[1], *IMAGE, (br.BLEND, 0, True, 0), [(br.BLEND, 0, False, 0)], [ALPHA]),
    "replace": br.BlendDesc(ORIGIN[0], ORIGIN[1], *IMAGE, (br.REPLACE, 0, False, 0), [], []),
}

# the hand-picked list scaled to IMAGE: the frame covers x 0..399, y 5..279, so the only edge inside the image is its top
STALE_RECTS = [(0, 0, 1, 1), (3, 1, 2, 2), (253, 2, 7, 6), (100, 3, 50, 6), (300, 0, 40, 4), (399, 279, 1, 1),
               (60, 100, 80, 40), (100, 120, 80, 50), (5, 5, 0, 3), (1000, 1000, 0, 0)]
EXTEND_RECTS = [(0, 0, 1, 1), (3, 1, 2, 2), (300, 0, 40, 4), (10, 0, 380, 5), (250, 2, 12, 3), (399, 0, 9, 4)]

_CACHE = {}


def workloads():
    from jxl_rs_amd import synth
    if "wl" not in _CACHE:
        _CACHE["wl"] = tuple(synth.make_vardct(*FRAME, mix=synth.MIX_D1, seed=s, **STAGES) for s in (71, 72))
    return _CACHE["wl"]


def slot_planes(seed, nch, size=IMAGE):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-0.5, 1.5, (size[1], size[0])).astype(np.float32) for _ in range(nch)]


def ec_samples(seed, w, h, bits=16):
    return np.random.default_rng(seed).integers(0, 1 << bits, size=(h, w)).astype(np.int32)


def oracle_frame(oracle, key, make):
    if key not in _CACHE:
        _CACHE[key] = [np.ascontiguousarray(p) for p in run_oracle_frame(oracle, make())[0]]
    return _CACHE[key]


def frames(oracle):
    """the oracle's colour planes of A, of A with GROUP's coefficients from B, and of A with every group's from B (the
    LF image and the maps stay A's: only coefficients arrive again)"""
    a, b = workloads()
    return (oracle_frame(oracle, "A", lambda: a), oracle_frame(oracle, "A+B", lambda: rr.with_groups_from(a, b, [GROUP])),
            oracle_frame(oracle, "B", lambda: rr.with_groups_from(a, b, list(range(a.coeffs.shape[0])))))


def with_ec(oracle, colour, desc, seed=5):
    """the frame's 3 + num_ec planes: the colour planes plus the converted 16-bit extra channels"""
    h, w = colour[0].shape
    return list(colour) + [oracle.modular_to_f32(ec_samples(seed + i, w, h), 16, 0) for i in range(len(desc.ec))]


def frame_rects(desc, fw, fh, rects):
    """jxlh_blend_image_rects restated: cut at the frame, shift, clip to the image, drop"""
    out = []
    for x0, y0, w, h in np.asarray(rects, dtype=np.int64).reshape(-1, 4).tolist():
        ax, ay = max(x0 + desc.x0, 0), max(y0 + desc.y0, 0)
        bx, by = min(min(x0 + w, fw) + desc.x0, desc.image_w), min(min(y0 + h, fh) + desc.y0, desc.image_h)
        if x0 < fw and y0 < fh and w and h and ax < bx and ay < by:
            out.append((ax, ay, bx - ax, by - ay))
    return out


def differing(before, after):
    d = np.zeros(before[0].shape, dtype=bool)
    for x, y in zip(before, after):
        d |= np.ascontiguousarray(x).view(np.uint32) != np.ascontiguousarray(y).view(np.uint32)
    return d


def check_case(desc, fw, fh, before, after, rects, what):
    """the non-vacuity rules: in every non-empty rect (cut to the image) at least half of the pixels differ in at least
    one channel between the two expectations, and a rect that straddles an edge of the frame's box holds a differing pixel
    on each side of it"""
    diff = differing(before, after)
    ax, ay, bx, by = frame_box(desc.x0, desc.y0, fw, fh, desc.image_w, desc.image_h)
    inside = np.zeros(diff.shape, dtype=bool)
    inside[ay:by, ax:bx] = True
    seen = 0
    for x0, y0, w, h in rects:
        if not w or not h:
            continue
        seen += 1
        sel = (slice(y0, y0 + h), slice(x0, x0 + w))
        d, m = diff[sel], inside[sel]
        assert d.size and d.mean() >= 0.5, (what, (x0, y0, w, h), float(d.mean()) if d.size else None)
        if m.any() and not m.all():  # the rect straddles an edge of the frame
            assert d[m].any() and d[~m].any(), (what, (x0, y0, w, h), "one side of the frame's edge does not change")
    assert seen, what


# ---------------------------------------------------------------- the other routes
def frame_params(w, h, gab=True, epf=2, n=1, modular=False):
    from jxl_rs_amd import lib
    p = lib.FrameParams()
    assert lib.load().jxlh_default_frame_params(p, w, h) == lib.OK
    p.gab, p.epf_iters, p.upsampling = int(gab), int(epf), n
    if modular:
        p.flags |= lib.FRAME_MODULAR
        p.epf_sigma_for_modular = rr.SIGMA_FOR_MODULAR
    return p


# an upsampled frame: coded 264 x 300 (2 x 2 groups), factor 2, group 2 arrives again; the frame ends at image row 400
UPS_CODED, UPS_N, UPS_GROUP = (264, 300), 2, 2
UPS_DESC = br.BlendDesc(-20, -200, 500, 420, (br.ADD, 0, False, 2), [], [])


def ups_workloads():
    from jxl_rs_amd import synth
    if "ups" not in _CACHE:
        _CACHE["ups"] = tuple(synth.make_vardct(*UPS_CODED, mix=synth.MIX_D1, seed=s, **STAGES) for s in (81, 82))
    return _CACHE["ups"]


def ups_frames(oracle):
    a, b = ups_workloads()
    return tuple([oracle.upsample(UPS_N, p) for p in oracle_frame(oracle, key, make)]
                 for key, make in (("ups A", lambda: a), ("ups A+B", lambda: rr.with_groups_from(a, b, [UPS_GROUP]))))


# a Modular frame by cell: 300 x 520 (2 x 3 cells), Gaborish + EPF 2, cell 2 gets other samples
MOD_SIZE, MOD_CELL = (300, 520), 2
MOD_DESC = br.BlendDesc(10, -40, 320, 500, (br.MUL, 0, True, 1), [], [])


def mod_samples():
    w, h = MOD_SIZE
    chans, other = rr.modular_samples(5, w, h), rr.modular_samples(6, w, h)
    cur = [c.copy() for c in chans]
    x0, y0, x1, y1 = rr.cell(w, h, MOD_CELL)
    for c in range(3):
        cur[c][y0:y1, x0:x1] = other[c][y0:y1, x0:x1] + 64
    return chans, cur, (x0, y0, x1, y1)


def mod_frames(oracle):
    if "mod" not in _CACHE:
        chans, cur, _ = mod_samples()
        _CACHE["mod"] = tuple(rr.modular_result(oracle, c, 1, 2, 1, False) for c in (chans, cur))
    return _CACHE["mod"]


# an alpha channel delivered by rects: this rect of its samples arrives again
EC_UPDATE = (260, 40, 100, 90)


def ec_planes():
    """the alpha channel's samples before and after EC_UPDATE"""
    w, h = FRAME
    first = ec_samples(5, w, h)
    x0, y0, rw, rh = EC_UPDATE
    new = first.copy()
    new[y0:y0 + rh, x0:x0 + rw] = ec_samples(6, rw, rh)
    return first, new
