"""What the reference runs for the steps of a squeezed channel whose residual GROUPS have partly arrived: a restatement
of the per-cell bookkeeping of SqueezeInfo::new (transforms/step.rs:123-198), get_grid_idx and get_grid_rect
(frame/modular/mod.rs:133-181), kept apart from the library's planner, and tiles_reference, which computes EVERY cell of
EVERY level the way the reference does (dead ones included): smooth cells through the oracle's smooth_unsqueeze on the
cell's rect, regular cells through a numpy restatement of unsqueeze_scalar + smooth_tendency_scalar with explicit
prev / next_avg (squeeze.rs:143-194, 389-481, 576-682).

The reference names cells by grid index: a buffer's cell for an output cell is the same index for equal grid kinds,
index / 8 for a group cell over an LF-group buffer, 0 for a whole channel (get_grid_idx).  Every one of these is "the
cell that contains the output cell's first sample, mapped into the buffer's coordinates" -- a buffer's grid dimension is
the group dimension shifted by the channel's own shift (grid_dim) -- so the rule is stated on positions here, which also
covers grids the test chooses freely.

Levels are in the decoder's order throughout (smallest first); tiles[L] = (tile_w, tile_h, present): one cell in samples
of level L's output (0 / 0: the whole channel), present None or [tiles_y, tiles_x], non-zero where the residuals of the
cell have arrived."""
import numpy as np

from squeeze_preview_ref import D2, H, REGULAR, SMOOTH_1D, SMOOTH_2D, V, has_res


def grid_of(step, tile):
    """-> (tile_w, tile_h, tiles_x, tiles_y) of a level (get_grid_rect's grid_dim and the grid shape)"""
    _, ow, oh = step
    tw, th = (tile[0], tile[1]) if tile[0] and tile[1] else (ow, oh)
    return tw, th, -(-ow // tw), -(-oh // th)


def cell_rect(step, tile, tx, ty):
    """get_grid_rect: origin and size of cell (tx, ty), clipped to the channel"""
    _, ow, oh = step
    tw, th, _, _ = grid_of(step, tile)
    return tx * tw, ty * th, min(tw, ow - tx * tw), min(th, oh - ty * th)


def cell_zero(steps, tiles, level_missing, level, tx, ty):
    """the residual buffer of cell (tx, ty) of `level` is DataStatus::Zero: nothing of it has arrived"""
    if not has_res(*steps[level]):
        return False
    if level_missing[level]:
        return True
    present = tiles[level][2]
    return present is not None and not np.asarray(present)[ty, tx]


def cell_kind(steps, tiles, level_missing, level, tx, ty):
    """SqueezeInfo::new, step.rs:138-150: buf_in_avg is set when the step that produced this step's average squeezes
    the other axis (meta_apply.rs:150-161), and names that step's inputs"""
    if not cell_zero(steps, tiles, level_missing, level, tx, ty):
        return REGULAR
    hz = steps[level][0]
    if level > 0 and steps[level - 1][0] != hz:
        x0, y0, _, _ = cell_rect(steps[level], tiles[level], tx, ty)
        px, py = (x0 >> 1, y0) if hz else (x0, y0 >> 1)          # the cell's origin in the average = level - 1's output
        tw1, th1, nx1, ny1 = grid_of(steps[level - 1], tiles[level - 1])
        if cell_zero(steps, tiles, level_missing, level - 1, min(px // tw1, nx1 - 1), min(py // th1, ny1 - 1)):
            return SMOOTH_2D
    return SMOOTH_1D


def tile_kinds_ref(steps, tiles, level_missing, level):
    _, _, nx, ny = grid_of(steps[level], tiles[level])
    return np.array([[cell_kind(steps, tiles, level_missing, level, tx, ty) for tx in range(nx)] for ty in range(ny)], np.uint8)


def _trunc_div(x, d):
    return np.where(x >= 0, x // d, -((-x) // d))


def smooth_tendency(b, a, n):
    """smooth_tendency_scalar (squeeze.rs:143-168) on int64 arrays; b = prev, a = avg, n = next_avg"""
    up = (b >= a) & (a >= n)
    down = ~up & (b <= a) & (a <= n)
    d_up = _trunc_div(4 * b - 3 * n - a + 6, 12)
    d_up = np.where(d_up - (d_up & 1) > 2 * (b - a), 2 * (b - a) + 1, d_up)
    d_up = np.where(d_up + (d_up & 1) > 2 * (a - n), 2 * (a - n), d_up)
    d_dn = _trunc_div(4 * b - 3 * n - a - 6, 12)
    d_dn = np.where(d_dn + (d_dn & 1) < 2 * (b - a), 2 * (b - a) - 1, d_dn)
    d_dn = np.where(d_dn - (d_dn & 1) < 2 * (a - n), 2 * (a - n), d_dn)
    return np.where(up, d_up, np.where(down, d_dn, 0))


def unsqueeze_pair(avg, res, next_avg, prev):
    """unsqueeze_scalar (squeeze.rs:187-194) on int64 arrays -> (a, b)"""
    diff = res + smooth_tendency(prev, avg, next_avg)
    a = avg + _trunc_div(diff, 2)
    return a, a - diff


def regular_cell(avg, res, out, horizontal, x0, y0, w, h):
    """hsqueeze_scalar / vsqueeze_scalar for one cell, written into `out`: prev is the output sample just in front of the
    cell on the squeezed axis (out_prev; avg[0] at the channel's start), next_avg is avg[x + 1] also across the cell
    edge (in_next_avg; avg[x] at the channel's end), the odd tail is copied.  Only the cell's own residuals are read."""
    if not horizontal:
        return regular_cell(avg.T, res.T, out.T, True, y0, x0, h, w)
    a = avg[y0:y0 + h].astype(np.int64)
    n_avg = a.shape[1]
    p0, n_pairs = x0 // 2, w // 2
    r = res[y0:y0 + h, p0:p0 + n_pairs].astype(np.int64)
    prev = a[:, 0] if x0 == 0 else out[y0:y0 + h, x0 - 1].astype(np.int64)
    for i in range(n_pairs):
        x = p0 + i
        va, vb = unsqueeze_pair(a[:, x], r[:, i], a[:, min(x + 1, n_avg - 1)], prev)
        out[y0:y0 + h, 2 * x] = va.astype(np.int32)
        out[y0:y0 + h, 2 * x + 1] = vb.astype(np.int32)
        prev = vb
    if w & 1:
        out[y0:y0 + h, x0 + w - 1] = a[:, p0 + n_pairs].astype(np.int32)


def run_level(oracle, steps, tiles, level_missing, residuals, outputs, level, cvt_rne=False):
    """every cell of `level`, in raster order, into a fresh (zero) buffer per channel -> the level's planes.
    outputs[i]: the planes level i wrote (-1: the base)"""
    hz, ow, oh = steps[level]
    kinds = tile_kinds_ref(steps, tiles, level_missing, level)
    avg = outputs[level - 1]
    planes = [np.zeros((oh, ow), np.int32) for _ in avg]
    for ty in range(kinds.shape[0]):
        for tx in range(kinds.shape[1]):
            x0, y0, w, h = cell_rect(steps[level], tiles[level], tx, ty)
            for c, out in enumerate(planes):
                if kinds[ty, tx] == REGULAR:
                    res = residuals[level][c]
                    regular_cell(avg[c], res if res.size else np.zeros((oh, ow), np.int32), out, hz, x0, y0, w, h)
                else:
                    two_d = kinds[ty, tx] == SMOOTH_2D
                    src = outputs[level - 2][c] if two_d else avg[c]
                    # (a rect without one complete pair on a doubled axis comes back untouched: the fresh buffer's zeros)
                    out[y0:y0 + h, x0:x0 + w] = oracle.smooth_unsqueeze(D2 if two_d else H if hz else V, src, w, h, x0, y0, cvt_rne=cvt_rne)
    return planes


def tiles_reference(oracle, base, residuals, steps, tiles, level_missing=None, rct=None, cvt_rne=False, outputs=None, start=0):
    """-> (final planes, outputs).  outputs / start: levels below `start` are taken from an earlier call's outputs (masks
    of levels >= start changed since)"""
    level_missing = [False] * len(steps) if level_missing is None else level_missing
    outputs = {-1: [np.ascontiguousarray(b, dtype=np.int32) for b in base]} if outputs is None else {k: v for k, v in outputs.items() if k < start}
    for level in range(start, len(steps)):
        outputs[level] = run_level(oracle, steps, tiles, level_missing, residuals, outputs, level, cvt_rne)
    final = outputs[len(steps) - 1]
    return (oracle.rct(final, *rct) if rct is not None else final), outputs


# ---------------------------------------------------------------- the case lists of the tile tests (CPU and GPU)
# (size, the finest level's cell): coarser levels halve the cell on the axis the level between squeezes, the way a
# buffer's grid dimension is the group dimension shifted by its channel's shift
GEOMETRIES = {
    "40x24": ((40, 24), (8, 8)),        # the finest 3 of 5 levels mixed
    "33x29": ((33, 29), (16, 8)),       # odd tails, ragged last cells, the 1-wide last cell
    "200x70": ((200, 70), (32, 96)),    # more than 64 lines in a cell band
    "600x40": ((600, 40), (256, 40)),   # cells longer than one staged chunk of the line kernels (one cell row: the
                                        # issue's "256 x 0" -- a zero tile_h beside a non-zero tile_w is refused)
    "24x600": ((24, 600), (40, 256)),   # the transpose of the row above
}
N_MIXED = 3   # levels that get a grid, counted from the finest


def level_tiles(steps, finest, k):
    """the cell of the k-th level from the end"""
    tw, th = finest
    for level in range(len(steps) - 1, len(steps) - 1 - k, -1):
        tw, th = (max(tw >> 1, 1), th) if steps[level][0] else (tw, max(th >> 1, 1))
    return tw, th


def build_tiles(steps, finest, masks):
    """masks: {k: mask | None | "missing"} for the k-th level from the end (absent: one cell, present) ->
    (tiles, level_missing)"""
    n = len(steps)
    tiles, missing = [(0, 0, None)] * n, [False] * n
    for k, m in masks.items():
        tw, th = level_tiles(steps, finest, k)
        if isinstance(m, str):
            missing[n - 1 - k] = True
            m = None
        tiles[n - 1 - k] = (tw, th, None if m is None else np.ascontiguousarray(m, dtype=np.uint8))
    return tiles, missing


def grid_shapes(steps, finest):
    """-> [(tiles_y, tiles_x)], [(pad_y, pad_x)] for the N_MIXED finest levels: pad counts a last cell row / column that is
    one sample thick.  The families below are laid over the cells in front of it and the thin cells are present: missing,
    such a cell is zero under a 2-D or 1-D kind alike (no complete pair), so a byte of the level before it would change
    nothing -- and every byte of every mask is to matter (test_every_mask_byte_matters)."""
    shapes, pads = [], []
    for k in range(N_MIXED):
        step = steps[len(steps) - 1 - k]
        tw, th, nx, ny = grid_of(step, level_tiles(steps, finest, k) + (None,))
        pad = (int(ny > 1 and step[2] - (ny - 1) * th == 1), int(nx > 1 and step[1] - (nx - 1) * tw == 1))
        shapes.append((ny - pad[0], nx - pad[1]))
        pads.append(pad)
    return shapes, pads


def _front(shape, k):
    m = np.zeros(shape[0] * shape[1], np.uint8)
    m[:k] = 1
    return m.reshape(shape)


def _checker(shape, phase=0):
    ty, tx = np.indices(shape)
    return ((tx + ty + phase) % 2).astype(np.uint8)


def mask_families(shapes):
    """-> [(name, {k: mask})] for grids of the given [tiles_y, tiles_x] shapes (finest first)"""
    s0, s1, s2 = shapes
    cases = []
    spots = {"first": (0, 0), "last": (-1, -1), "centre": None}
    for name, at in spots.items():
        masks_p, masks_m = {}, {}
        for k, s in ((0, s0), (1, s1)):
            pos = (s[0] // 2, s[1] // 2) if at is None else at
            p, m = np.zeros(s, np.uint8), np.ones(s, np.uint8)
            p[pos], m[pos] = 1, 0
            masks_p[k], masks_m[k] = p, m
        cases.append((f"one_present_{name}", masks_p))
        cases.append((f"one_missing_{name}", masks_m))
    for phase in (0, 1):
        cols = {k: np.tile(((np.arange(s[1]) + phase + k) % 2).astype(np.uint8), (s[0], 1)) for k, s in enumerate(shapes)}
        rows = {k: np.tile(((np.arange(s[0]) + phase + k) % 2).astype(np.uint8)[:, None], (1, s[1])) for k, s in enumerate(shapes)}
        cases.append((f"stripes_columns_{phase}", cols))
        if s0[0] > 1:
            cases.append((f"stripes_rows_{phase}", rows))
        cases.append((f"checker_{phase}", {k: _checker(s, phase + k) for k, s in enumerate(shapes)}))
    n0 = s0[0] * s0[1]
    for k in sorted({1, n0 // 2, n0 - 1}):
        cases.append((f"front_finest_{k}", {0: _front(s0, k)}))
        cases.append((f"front_two_{k}", {0: _front(s0, k), 1: _front(s1, min(k + 1, s1[0] * s1[1] - 1))}))
    cases.append(("present_behind_mixed", {0: None, 1: _checker(s1), 2: _front(s2, 1)}))
    cases.append(("mixed_behind_missing", {0: _checker(s0, 1), 1: "missing"}))
    cases.append(("mixed_behind_missing_front", {0: _front(s0, max(n0 // 2, 1)), 1: "missing", 2: _checker(s2)}))
    return cases


def case_list(steps_of):
    """steps_of(w, h) -> decoder-order steps.  -> [(geometry, mask name)] -> (size, steps, tiles, level_missing, masks)"""
    out = {}
    for g, (size, finest) in GEOMETRIES.items():
        steps = steps_of(*size)
        shapes, pads = grid_shapes(steps, finest)
        for name, masks in mask_families(shapes):
            masks = {k: m if m is None or isinstance(m, str) else np.pad(m, ((0, pads[k][0]), (0, pads[k][1])), constant_values=1)
                     for k, m in masks.items()}
            out[(g, name)] = (size, steps) + build_tiles(steps, finest, masks) + (masks,)
    return out
