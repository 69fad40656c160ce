"""Squeeze previews per grid cell in one call (jxlh_unsqueeze_chain_preview_tiles): images forward-squeezed in
default_squeeze order, the residuals of some grid cells withheld -- their samples in the device planes poisoned -- and
the device planes against squeeze_tiles_ref.tiles_reference: every cell of every level, dead ones included, smooth cells
through the oracle, regular cells through the restated scalar step.  Bit exact: there are no tolerances.  What the masks
exercise is held by tests/test_squeeze_tiles_cpu.py on the reference alone."""
import numpy as np
import pytest

import squeeze_tiles_ref as ref
from helpers import DeviceArray
from test_gpu_squeeze_preview import CANARY, DeviceChain, assert_planes, chain_of, reference as preview_reference_of

pytestmark = pytest.mark.gpu

POISON = 0x3ABCDEF1      # what a residual sample under a missing cell holds: read, it would show in every output it reaches
RCT = (6, 0)


@pytest.fixture(scope="module")
def ctx():
    from jxl_rs_amd import Context
    c = Context(0)
    yield c
    c.close()


def default_steps(w, h):
    from jxl_rs_amd import synth
    return synth.default_squeeze_steps(w, h)[0]


CASES = ref.case_list(default_steps)
_PREFIX, _REFERENCES = {}, {}


def reference(oracle, chain, tiles, level_missing, key, cvt_rne=False):
    """-> (planes, planes behind the RCT, outputs); computed once per case, shared, handed out as it is.  The levels in
    front of the N_MIXED finest ones are the same for every case of a chain"""
    key = (id(chain), key, cvt_rne)
    if key not in _REFERENCES:
        n = chain.n
        if id(chain) not in _PREFIX:
            _PREFIX[id(chain)] = ref.tiles_reference(oracle, chain.base, chain.residuals, chain.steps[:n - ref.N_MIXED],
                                                     [(0, 0, None)] * (n - ref.N_MIXED))[1]
        assert all(t[2] is None and not m for t, m in zip(tiles[:n - ref.N_MIXED], level_missing))
        planes, outputs = ref.tiles_reference(oracle, chain.base, chain.residuals, chain.steps, tiles, level_missing, cvt_rne=cvt_rne,
                                              outputs=_PREFIX[id(chain)], start=n - ref.N_MIXED)
        _REFERENCES[key] = (planes, oracle.rct(planes, *RCT) if chain.nch == 3 else None, outputs)
    return _REFERENCES[key]


def residual_region(step, tile, tx, ty):
    """the residual samples of cell (tx, ty): (rows, columns) slices of the level's residual plane"""
    x0, y0, w, h = ref.cell_rect(step, tile, tx, ty)
    return (slice(y0, y0 + h), slice(x0 // 2, x0 // 2 + w // 2)) if step[0] else (slice(y0 // 2, y0 // 2 + h // 2), slice(x0, x0 + w))


def poison_missing_cells(dev, tiles):
    """the residual samples of cells whose byte of `present` is 0 become POISON, on the device and in the host copy that
    DeviceChain.result compares the planes with afterwards"""
    for level, (step, tile) in enumerate(zip(dev.chain.steps, tiles)):
        if tile[2] is None:
            continue
        for ty, tx in np.argwhere(tile[2] == 0):
            rows, cols = residual_region(step, tile, tx, ty)
            for host in dev.res_host[level]:
                host[rows, cols] = POISON
        for d, host in zip(dev.res[level], dev.res_host[level]):
            d.upload(host)


def run_tiles(ctx, dev, tiles, level_missing, n_planes=None, rct=None, cvt_rne=False):
    chain = dev.chain
    n_planes = chain.nch if n_planes is None else n_planes
    bw, bh = chain.base[0].shape[1], chain.base[0].shape[0]
    ctx.unsqueeze_chain_preview_tiles(dev.levels(level_missing, n_planes), tiles, dev.base[:n_planes], bw, bw, bh,
                                      dev.out_ptr[:n_planes], dev.out_stride, rct=rct, cvt_rne=cvt_rne)
    ctx.sync()
    planes = dev.result()[:n_planes]
    dev.poison()
    return planes


def check_case(ctx, oracle, chain, tiles, level_missing, key, both_flags=False, **pads):
    dev = DeviceChain(chain, **pads)
    try:
        poison_missing_cells(dev, tiles)
        plain, behind_rct, _ = reference(oracle, chain, tiles, level_missing, key)
        assert_planes(run_tiles(ctx, dev, tiles, level_missing), plain, (key, "3 planes"))
        assert_planes(run_tiles(ctx, dev, tiles, level_missing, rct=RCT), behind_rct, (key, "3 planes + RCT"))
        assert_planes(run_tiles(ctx, dev, tiles, level_missing, n_planes=1), plain[:1], (key, "1 plane"))
        if both_flags:
            plain_rne, behind_rct_rne, _ = reference(oracle, chain, tiles, level_missing, key, cvt_rne=True)
            assert any((a != b).any() for a, b in zip(plain, plain_rne))     # the two reference builds really differ
            assert_planes(run_tiles(ctx, dev, tiles, level_missing, rct=RCT, cvt_rne=True), behind_rct_rne, (key, "nearest even + RCT"))
            assert_planes(run_tiles(ctx, dev, tiles, level_missing, n_planes=1, cvt_rne=True), plain_rne[:1], (key, "nearest even, 1 plane"))
    finally:
        dev.free()


@pytest.mark.parametrize("g,name", list(CASES), ids=lambda v: v)
def test_mask_families(ctx, oracle, g, name):
    size, steps, tiles, level_missing, _ = CASES[(g, name)]
    chain = chain_of(*size, 3)
    assert chain.steps == steps
    check_case(ctx, oracle, chain, tiles, level_missing, (g, name), both_flags=name.startswith(("checker", "front_two")))


def _thin_cases():
    """33 x 29, cells of 16 x 8: the cells of the last column are one sample wide on the horizontal levels.  Missing, such a
    cell is ZERO (no complete pair: the reference leaves its fresh buffer untouched) -- under a uniform mask too, which
    is therefore not the whole-level preview here.  (The mask families keep these cells present: see grid_shapes.)"""
    steps = default_steps(33, 29)
    finest = ref.GEOMETRIES["33x29"][1]
    full = [(4, 3)] * 3
    return {
        "all_missing_finest": ref.build_tiles(steps, finest, {0: np.zeros(full[0], np.uint8)}),
        "all_missing_two": ref.build_tiles(steps, finest, {0: np.zeros(full[0], np.uint8), 1: np.zeros(full[1], np.uint8)}),
        "front": ref.build_tiles(steps, finest, {0: ref._front(full[0], 5), 1: ref._front(full[1], 7)}),
        "checker": ref.build_tiles(steps, finest, {k: ref._checker(full[k], k) for k in range(3)}),
        "thin_present_only": ref.build_tiles(steps, finest, {k: np.pad(np.zeros((4, 2), np.uint8), ((0, 0), (0, 1)), constant_values=1)
                                                             for k in range(2)}),
    }


@pytest.mark.parametrize("name", list(_thin_cases()))
def test_cells_without_a_complete_pair(ctx, oracle, name):
    tiles, level_missing = _thin_cases()[name]
    chain = chain_of(33, 29, 3)
    check_case(ctx, oracle, chain, tiles, level_missing, ("thin", name), both_flags=True)
    plain = reference(oracle, chain, tiles, level_missing, ("thin", name))[0]
    if name == "all_missing_finest":
        whole = preview_reference_of(oracle, chain, chain.suffix(1))
        assert (plain[0][:, 32] == 0).all() and (whole[0][:, 32] != 0).any()
        assert all(np.array_equal(a[:, :32], b[:, :32]) for a, b in zip(plain, whole))


@pytest.mark.parametrize("size", [(40, 24), (200, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_whole_channel_cells_of_each_kind(ctx, oracle, size):
    """tile_w = tile_h = 0: one cell, the whole channel -- regular, 1-D, 2-D by one byte each"""
    chain = chain_of(*size, 3)
    n = chain.n
    one, zero = np.ones((1, 1), np.uint8), np.zeros((1, 1), np.uint8)
    for masks, missing in (({0: zero}, chain.suffix(1)), ({0: zero, 1: zero}, chain.suffix(2)), ({0: one, 1: zero}, None),
                           ({0: zero, 1: one, 2: zero}, None), ({0: one, 1: one, 2: one}, chain.suffix(0))):
        tiles = [(0, 0, None)] * (n - 3) + [(0, 0, masks.get(k)) for k in (2, 1, 0)]
        key = ("whole", tuple(sorted((k, int(m[0, 0])) for k, m in masks.items())))
        check_case(ctx, oracle, chain, tiles, [False] * n, key)
        if missing is not None:
            assert_planes(reference(oracle, chain, tiles, [False] * n, key)[0], preview_reference_of(oracle, chain, missing), key)


def _timed(ctx, fn):
    ctx.kernel_timing(True)
    ctx.kernel_timing_reset()
    try:
        fn()
        ctx.sync()
        return {name: n for name, (_, n) in ctx.kernel_times().items()}
    finally:
        ctx.kernel_timing(False)


@pytest.mark.parametrize("size", [(40, 24), (64, 64), (300, 280)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_no_partly_arrived_level_is_the_preview_call(ctx, oracle, size):
    """masks NULL or uniform per level (grids whose cells all hold a complete pair): the planes AND the launches of
    jxlh_unsqueeze_chain_preview; with nothing missing those of jxlh_unsqueeze_chain"""
    chain = chain_of(*size, 3)
    n = chain.n
    bw, bh = chain.base[0].shape[1], chain.base[0].shape[0]
    dev = DeviceChain(chain)
    try:
        for missing, by_mask in ((chain.suffix(0), ()), (chain.suffix(2), (n - 1,)), (chain.suffix(3), (n - 1, n - 3)),
                                 (tuple(i in (n - 2, n - 4) for i in range(n)), (n - 2,)), (chain.suffix(1), ())):
            tiles, level_missing = [], []
            for level, step in enumerate(chain.steps):
                tw, th = ref.level_tiles(chain.steps, (8, 8), n - 1 - level) if level >= n - 3 else (0, 0)
                nx, ny = ref.grid_of(step, (tw, th))[2:]
                # a missing level: res[] NULL, or planes named and every byte zero; a present one: NULL mask or every byte set
                use_mask = level in by_mask or (not missing[level] and level % 2 == 0)
                tiles.append((tw, th, np.full((ny, nx), 0 if missing[level] else 1 + level, np.uint8) if use_mask else None))
                level_missing.append(missing[level] and level not in by_mask)
            for rct in (None, RCT):
                args = (dev.base, bw, bw, bh, dev.out_ptr, dev.out_stride)
                counts = _timed(ctx, lambda: ctx.unsqueeze_chain_preview_tiles(dev.levels(level_missing), tiles, *args, rct=rct))
                got = dev.result()
                dev.poison()
                want_counts = _timed(ctx, lambda: ctx.unsqueeze_chain_preview(dev.levels(missing), *args, rct=rct))
                assert_planes(got, dev.result(), (size, missing, rct))
                dev.poison()
                assert counts == want_counts and counts, (counts, want_counts)
                assert_planes(got, preview_reference_of(oracle, chain, missing, rct), (size, missing, rct, "the oracle"))
                if not any(missing):
                    chain_counts = _timed(ctx, lambda: ctx.unsqueeze_chain(dev.levels(missing), *args, rct=rct))
                    assert_planes(got, dev.result(), (size, "the chain call"))
                    dev.poison()
                    assert counts == chain_counts, (counts, chain_counts)
    finally:
        dev.free()


def test_a_mixed_level_takes_two_launches(ctx, oracle):
    """the library's timers, one per launch: 200 x 70 with checkerboards on its three finest levels (7 cells each) is the
    prefix as the chain it is, then one smooth-cell launch and one run launch per level whatever the number of cells,
    then the RCT"""
    size, steps, tiles, level_missing, _ = CASES[("200x70", "checker_0")]
    chain = chain_of(*size, 3)
    dev = DeviceChain(chain)
    try:
        bw, bh = chain.base[0].shape[1], chain.base[0].shape[0]
        counts = _timed(ctx, lambda: ctx.unsqueeze_chain_preview_tiles(dev.levels(level_missing), tiles, dev.base, bw, bw, bh, dev.out_ptr,
                                                                       dev.out_stride, rct=RCT))
        assert counts == {"k6_unsqueeze_chain": 1, "k6_smooth_unsqueeze_cells": 3, "k6_unsqueeze_runs": 3, "k4_rct": 1}, counts
    finally:
        dev.free()


@pytest.mark.parametrize("g,name", [("40x24", "checker_0"), ("33x29", "front_two_4"), ("600x40", "stripes_columns_1"),
                                    ("24x600", "checker_1")], ids=lambda v: v)
def test_padded_strides_and_unaligned_planes(ctx, oracle, g, name):
    """output rows wider than the image (odd and even paddings: the pair stores give way to single ones), residual rows
    padded, bases four bytes off 16-byte alignment: same planes, canaries in the row padding and around the planes intact"""
    size, steps, tiles, level_missing, _ = CASES[(g, name)]
    chain = chain_of(*size, 3)
    for res_pad, out_pad, skew in ((3, 7, 0), (5, 2, 1), (0, 1, 1)):
        check_case(ctx, oracle, chain, tiles, level_missing, (g, name), res_pad=res_pad, out_pad=out_pad, base_skew=skew)


@pytest.mark.parametrize("g", ["40x24", "33x29"])
def test_streaming_sequence(ctx, oracle, g):
    """a download: the cells of the two finest levels arrive one group at a time -- group i brings cell i of both levels --
    and the image is painted again after each, on the same buffers; every paint is the reference's, the last one the
    chain call's.  Residual samples are POISON until their cell has arrived."""
    size, finest = ref.GEOMETRIES[g]
    chain = chain_of(*size, 3)
    n = chain.n
    shapes = [ref.grid_of(chain.steps[n - 1 - k], ref.level_tiles(chain.steps, finest, k))[3:1:-1] for k in range(2)]
    assert shapes[0] == shapes[1]
    dev = DeviceChain(chain)
    real = {level: [h.copy() for h in dev.res_host[level]] for level in (n - 2, n - 1)}
    try:
        masks = {k: np.zeros(shapes[k], np.uint8) for k in range(2)}
        tiles, level_missing = ref.build_tiles(chain.steps, finest, masks)
        poison_missing_cells(dev, tiles)
        order = list(np.ndindex(shapes[0]))
        for i, at in enumerate([None] + order):
            if at is not None:
                ty, tx = at
                for k in range(2):
                    level = n - 1 - k
                    masks[k][ty, tx] = 1
                    rows, cols = residual_region(chain.steps[level], tiles[level], tx, ty)
                    for d, host, src in zip(dev.res[level], dev.res_host[level], real[level]):
                        host[rows, cols] = src[rows, cols]
                        d.upload(host)
            tiles, level_missing = ref.build_tiles(chain.steps, finest, {k: m.copy() for k, m in masks.items()})
            want = reference(oracle, chain, tiles, level_missing, ("stream", g, i))[1]
            assert_planes(run_tiles(ctx, dev, tiles, level_missing, rct=RCT), want, (g, "after group", i))
        bw, bh = chain.base[0].shape[1], chain.base[0].shape[0]
        ctx.unsqueeze_chain(dev.levels([False] * n), dev.base, bw, bw, bh, dev.out_ptr, dev.out_stride, rct=RCT)
        ctx.sync()
        assert_planes(dev.result(), want, (g, "the chain call"))
        assert_planes(want, oracle.rct(chain.image, *RCT), (g, "the image comes back"))
    finally:
        dev.free()


def test_modular_chain_route(ctx, oracle):
    from jxl_rs_amd.modular import ModularChain
    size, steps, tiles, level_missing, _ = CASES[("40x24", "front_two_7")]
    chain = chain_of(*size, 3)
    mc = ModularChain(ctx, *size, rct=RCT, planes=(chain.base, chain.residuals, chain.steps))
    try:
        mc.preview_tiles(tiles)
        assert_planes(mc.result(), reference(oracle, chain, tiles, level_missing, ("40x24", "front_two_7"))[1], "ModularChain.preview_tiles")
    finally:
        mc.free()


def test_argument_errors_launch_nothing(ctx):
    from jxl_rs_amd import lib, JxlHipError
    size, steps, tiles, level_missing, _ = CASES[("40x24", "checker_0")]
    chain = chain_of(*size, 3)
    dev = DeviceChain(chain)
    bw, bh = chain.base[0].shape[1], chain.base[0].shape[0]
    n = chain.n
    good = dev.levels(level_missing)

    def refused(levels=good, tiles_=tiles, base=None, bw_=bw, out=None, out_stride=None, **kw):
        with pytest.raises(JxlHipError) as e:
            ctx.unsqueeze_chain_preview_tiles(levels, tiles_, dev.base if base is None else base, bw_, bw_, bh,
                                              dev.out_ptr if out is None else out, dev.out_stride if out_stride is None else out_stride, **kw)
        assert e.value.status == lib.ERR_INVALID_ARGUMENT

    def with_tile(level, tw, th):
        t = list(tiles)
        nx, ny = ref.grid_of(chain.steps[level], (tw, th))[2:] if tw and th else (1, 1)
        t[level] = (tw, th, np.ones((ny, nx), np.uint8))
        return t

    try:
        # what jxlh_unsqueeze_chain_preview refuses
        partly = list(good)
        hz, ow, oh, res, rs = good[n - 3]
        partly[n - 3] = (hz, ow, oh, [res[0], None, res[2]], rs)
        refused(partly)
        refused(flags=0x200)
        refused(rct=(7, 0))
        refused(rct=(6, 6))
        refused(base=dev.base[:1], out=dev.out_ptr[:1], levels=dev.levels(level_missing, 1), rct=RCT)
        refused(bw_=bw + 1)
        refused(out_stride=chain.w - 1)
        host = np.zeros((bh, bw), np.int32)
        refused(base=[host, host, host])
        # the grids
        assert chain.steps[n - 1][0] and not chain.steps[n - 2][0]
        refused(tiles_=with_tile(n - 1, 8, 0))
        refused(tiles_=with_tile(n - 1, 0, 8))
        refused(tiles_=with_tile(n - 1, 7, 8))                     # an odd tile_w on a horizontal level with several columns
        refused(tiles_=with_tile(n - 2, 4, 7))                     # an odd tile_h on a vertical level with several rows
        L, arr = lib._lib(), lib._squeeze_levels(good, 3)
        import ctypes as C
        bv, ov = (C.c_void_p * 3)(*dev.base), (C.c_void_p * 3)(*dev.out_ptr)
        assert L.jxlh_unsqueeze_chain_preview_tiles(ctx._ctx, 3, n, C.cast(arr, C.c_void_p), None, bv, bw, bw, bh, ov, dev.out_stride,
                                                    -1, 0, 0) == lib.ERR_INVALID_ARGUMENT       # tiles == NULL
        ctx.sync()
        for raw in dev.raw_out():
            assert (raw == CANARY).all()
        # ... and what it accepts still runs afterwards
        ctx.unsqueeze_chain_preview_tiles(good, with_tile(n - 1, 8, 7), dev.base, bw, bw, bh, dev.out_ptr, dev.out_stride)
        ctx.unsqueeze_chain_preview_tiles(good, with_tile(n - 1, 41, 8), dev.base, bw, bw, bh, dev.out_ptr, dev.out_stride)
        ctx.sync()
    finally:
        dev.free()


def test_too_many_cells(ctx):
    """more than 2^20 cells in a level: refused before anything is enqueued"""
    from jxl_rs_amd import lib, JxlHipError
    from squeeze_preview_ref import explicit_steps
    steps = explicit_steps(4096, 1024, [True])[0]
    base = DeviceArray(nbytes=2048 * 1024 * 4)
    res = DeviceArray(nbytes=2048 * 1024 * 4)
    out = DeviceArray(np.full((1024, 4096), CANARY, np.int32))
    try:
        levels = [(True, 4096, 1024, [res.ptr, None, None], 2048)]
        with pytest.raises(JxlHipError) as e:
            ctx.unsqueeze_chain_preview_tiles(levels, [(2, 1, None)], [base.ptr], 2048, 2048, 1024, [out.ptr], 4096)
        assert e.value.status == lib.ERR_INVALID_ARGUMENT
        ctx.sync()
        assert (out.download(np.int32, 4096 * 1024) == CANARY).all()
    finally:
        for d in (base, res, out):
            d.free()
