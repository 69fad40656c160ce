"""numpy float32 restatement of the reference's patches stage: perform_blending (jxl/src/features/blending.rs:199-474)
and PatchesDictionary::add_one_row (features/patches.rs:683-759).  Every operation is one float32 numpy operation, in
the reference's association and without fusion; the arrays are the pixels one patch covers, so the blend is pointwise
exactly as in the reference (its "old alpha" scratch is a copy of the extra channels taken before each patch).

Modes are PatchBlendMode values (patches.rs:41-74); a blending is (mode, alpha_channel, clamp); ec_flags[k] holds
EC_ALPHA / EC_ALPHA_ASSOCIATED of extra channel k."""
import numpy as np

NONE, REPLACE, ADD, MUL, BLEND_ABOVE, BLEND_BELOW, AWA_ABOVE, AWA_BELOW = range(8)
EC_ALPHA, EC_ALPHA_ASSOCIATED = 1, 2
F = np.float32
ONE, ZERO = F(1.0), F(0.0)


def uses_alpha(mode):
    return mode in (BLEND_ABOVE, BLEND_BELOW, AWA_ABOVE, AWA_BELOW)


def _clamp(v, clamp):
    return np.minimum(np.maximum(v, ZERO), ONE) if clamp else v


def _recip(new_a):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = ONE / new_a
    return np.where(new_a > ZERO, r, ZERO).astype(F)


def perform_blending(bg, fg, color_blending, ec_blendings, ec_flags):
    """bg: list of 3 + num_ec float32 arrays (same shape), blended in place; fg: the same of the foreground"""
    num_ec = len(ec_flags)
    has_alpha = any(f & EC_ALPHA for f in ec_flags)
    assoc = [bool(f & EC_ALPHA_ASSOCIATED) for f in ec_flags]
    old = [bg[3 + i].copy() for i in range(num_ec)]
    for i in range(num_ec):
        mode, alpha, clamp = ec_blendings[i]
        o, f = bg[3 + i], fg[3 + i]
        if mode == ADD:
            o[...] = o + f
        elif mode == BLEND_ABOVE:
            if i == alpha:
                top_a = _clamp(f, clamp)
                o[...] = ONE - (ONE - top_a) * (ONE - o)
            elif assoc[alpha]:
                fa = _clamp(fg[3 + alpha], clamp)
                o[...] = f + o * (ONE - fa)
            else:
                fa = _clamp(fg[3 + alpha], clamp)
                oa = old[alpha]
                new_a = ONE - (ONE - fa) * (ONE - oa)
                o[...] = (f * fa + o * oa * (ONE - fa)) * _recip(new_a)
        elif mode == BLEND_BELOW:
            if i == alpha:
                top_a = _clamp(o, clamp)
                o[...] = ONE - (ONE - top_a) * (ONE - f)
            elif assoc[alpha]:
                ba = _clamp(old[alpha], clamp)
                o[...] = o + f * (ONE - ba)
            else:
                ba = _clamp(old[alpha], clamp)
                new_a = ONE - (ONE - ba) * (ONE - fg[3 + alpha])
                o[...] = (o * ba + f * fg[3 + alpha] * (ONE - ba)) * _recip(new_a)
        elif mode == AWA_ABOVE:
            if i != alpha:
                o[...] = o + f * _clamp(fg[3 + alpha], clamp)
        elif mode == AWA_BELOW:
            if i == alpha:
                o[...] = f
            else:
                o[...] = f + o * _clamp(old[alpha], clamp)
        elif mode == MUL:
            o[...] = o * _clamp(f, clamp)
        elif mode == REPLACE:
            o[...] = f
    mode, alpha, clamp = color_blending
    if mode == ADD or (mode in (AWA_ABOVE, AWA_BELOW) and not has_alpha):
        for c in range(3):
            bg[c][...] = bg[c] + fg[c]
    elif mode == AWA_ABOVE:
        w = _clamp(fg[3 + alpha], clamp)
        for c in range(3):
            bg[c][...] = bg[c] + fg[c] * w
    elif mode == AWA_BELOW:
        w = _clamp(old[alpha], clamp)
        for c in range(3):
            bg[c][...] = fg[c] + bg[c] * w
    elif mode in (BLEND_ABOVE, BLEND_BELOW):
        if not has_alpha:
            if mode == BLEND_ABOVE:
                for c in range(3):
                    bg[c][...] = fg[c]
        else:
            above = mode == BLEND_ABOVE
            top_a = _clamp(fg[3 + alpha] if above else old[alpha], clamp)
            bottom_a = old[alpha] if above else fg[3 + alpha]
            omta = ONE - top_a
            new_a = ONE - omta * (ONE - bottom_a)
            r = _recip(new_a)
            for c in range(3):
                top_c, bottom_c = (fg[c], bg[c]) if above else (bg[c], fg[c])
                if assoc[alpha]:
                    out = top_c + bottom_c * omta
                else:
                    out = (top_c * top_a + bottom_c * bottom_a * omta) * r
                bg[c][...] = out
            bg[3 + alpha][...] = new_a
    elif mode == MUL:
        for c in range(3):
            bg[c][...] = bg[c] * _clamp(fg[c], clamp)
    elif mode == REPLACE:
        for c in range(3):
            bg[c][...] = fg[c]


def sanitize(blending, num_ec):
    """the alpha channel as PatchesDictionary::read leaves it: read only for a mode that uses alpha with more than
    one extra channel (patches.rs:585-596), 0 otherwise"""
    mode, alpha, clamp = blending
    return (mode, alpha if uses_alpha(mode) and num_ec > 1 else 0, bool(clamp))


def apply_patches(planes, patches, blendings, refs, ec_flags, x0=0, x1=None, y0=0, y1=None):
    """planes: 3 + num_ec float32 [h, w] arrays, patched in place on the window [x0, x1) x [y0, y1) (the row chunk a
    render pass hands PatchesStage); patches: (x, y, slot, rx, ry, xs, ys); blendings: flat, 1 + num_ec per patch;
    refs[slot]: list of 3 + num_ec planes"""
    num_ec = len(ec_flags)
    h, w = planes[0].shape
    x1 = w if x1 is None else min(x1, w)
    y1 = h if y1 is None else min(y1, h)
    stride = 1 + num_ec
    for i, (px, py, slot, rx, ry, xs, ys) in enumerate(patches):
        ax0, ax1 = max(px, x0), min(px + xs, x1)
        ay0, ay1 = max(py, y0), min(py + ys, y1)
        if ax0 >= ax1 or ay0 >= ay1:
            continue
        bl = [sanitize(b, num_ec) for b in blendings[i * stride:(i + 1) * stride]]
        bg = [p[ay0:ay1, ax0:ax1].copy() for p in planes]
        fg = [r[ry + ay0 - py:ry + ay1 - py, rx + ax0 - px:rx + ax1 - px] for r in refs[slot]]
        perform_blending(bg, fg, bl[0], bl[1:], ec_flags)
        for p, b in zip(planes, bg):
            p[ay0:ay1, ax0:ax1] = b
    return planes
