"""Groups whose HF has not arrived (run with -m gpu on an MI355X): jxlh_frame_set_groups_lf_only marks them, the next
run fills them from the LF image upsampled 8x (k_lf_fill.hip) instead of transforming them.  Every comparison is bit for
bit against tests/lf_fill_ref.py: decode_group for the unmarked groups, the group's rect of upsample(8, whole LF image)
for the marked ones, then the oracle's filters, noise and upsampling."""
import numpy as np
import pytest

from helpers import bit_equal, diff_report, gpu_params_from, oracle_params_from, run_oracle_frame
from lf_fill_ref import expected_planes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import jxl_rs_amd
    c = jxl_rs_amd.Context(0, 1)
    yield c
    c.close()


_frames = {}


def frame(w, h, seed=5):
    """one workload per size and seed for the whole module (MIX_ALL: every transform family next to the filled groups)"""
    from jxl_rs_amd import synth
    key = (w, h, seed)
    if key not in _frames:
        _frames[key] = synth.make_vardct(w, h, mix=synth.MIX_ALL, seed=seed, epf_iters=2)
    return _frames[key]


def assert_planes(got, want, what):
    for c, (g, e) in enumerate(zip(got, want)):
        assert g.shape == e.shape, (what, c, g.shape, e.shape)
        assert bit_equal(g, e), f"{what}: channel {c}: {diff_report(g, e)}"


def submit(ctx, wl, groups, transport="dense"):
    from jxl_rs_amd import lib, synth
    groups = [int(g) for g in groups]
    if transport == "dense":
        for g in groups:
            ctx.submit_group(g, wl.coeffs[g])
    elif transport == "sparse":
        for g in groups:
            ctx.submit_group_sparse(g, *synth.to_sparse(wl.coeffs[g]))
    elif transport == "slots" and groups:
        parts = [lib.host_pack_slots(wl.coeffs[g], group_id=g) for g in groups]
        assert all(len(q[3]) == 0 for q in parts)
        ctx.submit_groups_slots(np.asarray(groups, np.uint32), np.concatenate([q[0] for q in parts]),
                                np.concatenate([q[1].reshape(-1) for q in parts]), np.concatenate([q[2] for q in parts]), None)
    ctx.slot_wait(0)


def begin(ctx, wl, marked, transport="dense", lf_slot=None, tweak=None, **over):
    """the frame with its LF and HF metadata, `marked` marked and every other group submitted"""
    p = gpu_params_from(ctx, wl, **over)
    if tweak:
        tweak(p)
    ctx.frame_begin(p)
    ctx.set_dequant_tables(wl.tables)
    if lf_slot is None:
        ctx.set_lf_quantized(*wl.lf_q)
    else:
        ctx.set_lf_from_slot(lf_slot)
    ctx.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)
    ctx.set_groups_lf_only(list(marked))
    n = wl.xgroups * wl.ygroups
    submit(ctx, wl, [g for g in range(n) if g not in set(marked)], transport)
    return p


def render(ctx, wl, marked, **kw):
    begin(ctx, wl, marked, **kw)
    ctx.frame_run()
    ctx.sync()
    return ctx.read_planes()


def marked_sets(wl):
    xg, yg = wl.xgroups, wl.ygroups
    n = xg * yg
    sets = {"all": list(range(n))}
    if n > 1:
        sets["corner"] = [0]
        sets["checker"] = [g for g in range(n) if (g % xg + g // xg) % 2 == 0]
    if n >= 6:  # one interior-edge pair of neighbours: the middle column (3 x 2) or the middle row (2 x 3)
        sets["pair"] = [1, 1 + xg] if xg == 3 else [xg, xg + 1]
    return sets


SHAPES = {"256x256": ["all"], "520x300": ["corner", "pair", "checker", "all"], "300x520": ["corner", "pair", "checker", "all"],
          "200x300": ["corner", "all"], "24x16": ["all"]}
CASES = [(s, m) for s, ms in SHAPES.items() for m in ms]


# ---------------------------------------------------------------- shapes and marked sets (Gaborish + EPF2: fused, tiled)
@pytest.mark.parametrize("shape,which", CASES, ids=[f"{s}-{m}" for s, m in CASES])
def test_shapes_and_marked_sets(ctx, oracle, shape, which):
    """256 x 256: one group.  520 x 300: 3 x 2 groups, ragged, xblocks % 32 == 1 (the reference's geometry (b)).  300 x 520.
    200 x 300: one column of groups (geometry (a)).  24 x 16: a 3 x 2 LF image, the window mirrors more than once."""
    w, h = [int(v) for v in shape.split("x")]
    wl = frame(w, h)
    marked = marked_sets(wl)[which]
    got = render(ctx, wl, marked)
    assert_planes(got, expected_planes(oracle, wl, marked), f"{shape} {which} {marked}")
    plain, _ = run_oracle_frame(oracle, wl)
    assert any(not bit_equal(a, b) for a, b in zip(got, plain)), "the marked groups look transformed"


# ---------------------------------------------------------------- stage lists and flags
@pytest.mark.parametrize("name,over", [
    ("no_filter_raster", dict(epf_iters=0, gab=0)),
    ("gab_only", dict(epf_iters=0, gab=1)),
    ("epf3", dict(epf_iters=3)),
    ("unfused", dict(flags=1)),        # JXLH_FRAME_UNFUSED_FILTERS: raster, per-stage kernels
    ("unfused_epf1", dict(flags=1, epf_iters=1, gab=0)),
    ("no_lf_smoothing", dict(do_lf_smoothing=0)),
])
def test_stage_lists_and_flags(ctx, oracle, name, over):
    wl = frame(520, 300)
    marked = marked_sets(wl)["checker"]
    oracle_over = {k: v for k, v in over.items() if k != "flags"}
    assert_planes(render(ctx, wl, marked, **over), expected_planes(oracle, wl, marked, **oracle_over), name)


def test_lf_smoothing_is_what_the_fill_reads(ctx, oracle):
    wl = frame(520, 300)
    on = expected_planes(oracle, wl, [0], do_lf_smoothing=1)
    off = expected_planes(oracle, wl, [0], do_lf_smoothing=0)
    assert not bit_equal(on[1][:256, :256], off[1][:256, :256]), "smoothing changes nothing on this input"
    assert_planes(render(ctx, wl, [0], do_lf_smoothing=1), on, "smoothed LF")
    assert_planes(render(ctx, wl, [0], do_lf_smoothing=0), off, "raw LF")


def test_strip_flag_falls_back_to_the_two_kernel_path(ctx, oracle):
    from jxl_rs_amd import lib
    wl = frame(520, 300)
    plain = render(ctx, wl, [], flags=lib.FRAME_STRIP)
    assert ctx.frame_path()[0], "the flag is live: a frame without marks takes the strip kernel"
    assert_planes(plain, run_oracle_frame(oracle, wl)[0], "strip, no marks")
    marked = [1, 3]
    got = render(ctx, wl, marked, flags=lib.FRAME_STRIP)
    assert not ctx.frame_path()[0], "a frame with a marked group must not take the strip kernel"
    assert_planes(got, expected_planes(oracle, wl, marked), "JXLH_FRAME_STRIP with marks")


# ---------------------------------------------------------------- stages behind it
LUT = np.float32([0.02, 0.05, 0.1, 0.2, 0.15, 0.1, 0.05, 0.3])


def test_noise_behind_the_fill(ctx, oracle):
    wl = frame(300, 520)
    marked = [0, 3, 5]

    def tweak(p):
        p.noise, p.visible_frame_index = 1, 1
        for i in range(8):
            p.noise_lut[i] = float(LUT[i])
    begin(ctx, wl, marked, tweak=tweak)
    ctx.frame_run()
    ctx.sync()
    rnd = [oracle.noise_convolve(r) for r in oracle.noise_generate(1, 0, wl.xsize, wl.ysize)]
    want = oracle.noise_add(LUT, 0.0, 1.0, expected_planes(oracle, wl, marked), rnd)
    assert_planes(ctx.read_planes(), want, "noise")


def custom_weights(n, seed):
    return np.random.default_rng(seed).uniform(-0.05, 0.12, n).astype(np.float32)


def test_custom_weights8_are_the_ones_the_fill_uses(ctx, oracle):
    wl = frame(300, 520)
    marked = [0, 3]
    w8 = custom_weights(210, 8)
    dflt = expected_planes(oracle, wl, marked)
    want = expected_planes(oracle, wl, marked, weights8=w8)
    assert not bit_equal(dflt[1], want[1])
    try:
        ctx.set_upsampling_weights(w8=w8)
        assert_planes(render(ctx, wl, marked), want, "custom weights8")
    finally:
        ctx.set_upsampling_weights()
    assert_planes(render(ctx, wl, marked), dflt, "back to the default weights8")


def test_upsampling_2_keeps_its_own_kernels_behind_the_fill(ctx, oracle):
    wl = frame(200, 300)
    marked = [1]
    w2, w8 = custom_weights(15, 2), custom_weights(210, 9)
    base = expected_planes(oracle, wl, marked, weights8=w8)
    want = [oracle.upsample(2, np.ascontiguousarray(a), w2) for a in base]
    try:
        ctx.set_upsampling_weights(w2=w2, w8=w8)
        for attempt in range(2):  # (the second run finds both kernel sets uploaded)
            got = render(ctx, wl, marked, upsampling=2)
            assert ctx.out_size == (400, 600)
            assert_planes(got, want, f"upsampling = 2, run {attempt}")
    finally:
        ctx.set_upsampling_weights()


# ---------------------------------------------------------------- slot-fed LF, transports, stale store
def test_frame_fed_from_an_lf_slot(ctx, oracle):
    wl = frame(300, 520)
    p = oracle_params_from(oracle, wl)
    rng = np.random.default_rng(12)
    lf = [(a + rng.uniform(-0.02, 0.02, a.shape)).astype(np.float32) for a in oracle.dequant_lf(p, *wl.lf_q)]
    marked = [1, 2, 5]
    ctx.set_lf_frame(2, *lf)
    try:
        got = render(ctx, wl, marked, lf_slot=2)
    finally:
        ctx.clear_lf_frame(2)
    assert_planes(got, expected_planes(oracle, wl, marked, lf=lf, from_slot=True), "slot-fed LF (no smoothing)")


@pytest.mark.parametrize("transport", ["dense", "sparse", "slots"])
def test_transports_of_the_unmarked_groups(ctx, oracle, transport):
    wl = frame(520, 300)
    marked = [1, 4]
    assert_planes(render(ctx, wl, marked, transport=transport), expected_planes(oracle, wl, marked), transport)


def test_a_marked_group_does_not_read_the_previous_frames_coefficients(ctx, oracle):
    a, b = frame(520, 300, seed=5), frame(520, 300, seed=6)
    assert_planes(render(ctx, a, []), run_oracle_frame(oracle, a)[0], "frame A, complete")
    marked = [0, 4]  # never submitted in B: the store still holds A's groups 0 and 4
    assert_planes(render(ctx, b, marked), expected_planes(oracle, b, marked), "frame B on A's store")


# ---------------------------------------------------------------- the streaming sequence
def test_streaming_sequence(ctx, oracle):
    wl = frame(520, 300)
    n = wl.xgroups * wl.ygroups
    every = list(range(n))
    begin(ctx, wl, every)  # LF first: nothing submitted
    ctx.frame_run()
    ctx.sync()
    assert_planes(ctx.read_planes(), expected_planes(oracle, wl, every), "first paint: every group from the LF")
    # two groups arrive
    submit(ctx, wl, [4, 0])
    ctx.rerender_groups([4, 0])
    ctx.sync()
    left = [1, 2, 3, 5]
    want = expected_planes(oracle, wl, left)
    assert_planes(ctx.read_planes(), want, "groups 0 and 4 arrived")
    # a still-marked group in the list is filled again: nothing changes
    ctx.rerender_groups([2])
    ctx.sync()
    assert_planes(ctx.read_planes(), want, "rerender of a still-marked group")
    # the rest arrives
    submit(ctx, wl, left)
    ctx.rerender_groups(left)
    ctx.sync()
    final = ctx.read_planes()
    assert_planes(final, expected_planes(oracle, wl, []), "all groups arrived: the builder")
    assert_planes(final, run_oracle_frame(oracle, wl)[0], "all groups arrived: oracle.vardct_frame")
    # marking a submitted group and running fills it again (its coefficients stay and are not read)
    ctx.set_groups_lf_only([3])
    ctx.frame_run()
    ctx.sync()
    assert_planes(ctx.read_planes(), expected_planes(oracle, wl, [3]), "marked after its submission")
    # ... and its next submission clears the mark
    submit(ctx, wl, [3])
    ctx.rerender_groups([3])
    ctx.sync()
    assert_planes(ctx.read_planes(), final, "submitted again")


def test_marks_are_per_frame_and_persist_across_runs(ctx, oracle):
    wl = frame(300, 520)
    marked = [2]
    begin(ctx, wl, marked)
    for run in range(2):
        ctx.frame_run()
        ctx.sync()
        assert_planes(ctx.read_planes(), expected_planes(oracle, wl, marked), f"run {run}")
    assert_planes(render(ctx, wl, []), run_oracle_frame(oracle, wl)[0], "the next frame starts without marks")


# ---------------------------------------------------------------- band run, long axis
def test_band_run_fills_the_band_and_its_halo_rows(ctx, oracle):
    """300 x 700: 2 x 3 groups.  jxlh_frame_run(1, 2) transforms / fills group rows 0..2 (the band and its halo rows)
    and filters rows 256..511; marked groups sit in the band and in both halo rows."""
    wl = frame(300, 700)
    marked = [1, 2, 5]
    begin(ctx, wl, marked)
    ctx.frame_run(1, 2)
    ctx.sync()
    got = [a[256:512] for a in ctx.read_planes()]
    want = [a[256:512] for a in expected_planes(oracle, wl, marked)]
    assert_planes(got, want, "band rows")


def test_long_axis_every_group_marked(ctx, oracle):
    """16 x 65 552: 257 groups in one column, every one filled: no image axis may be a grid dimension"""
    from jxl_rs_amd import synth
    wl = synth.make_vardct(16, 65552, mix=synth.MIX_DCT8, seed=1, unique_groups=1, epf_iters=1)
    every = list(range(wl.xgroups * wl.ygroups))
    assert len(every) == 257
    p = gpu_params_from(ctx, wl)
    ctx.frame_begin(p)
    ctx.set_dequant_tables(wl.tables)
    ctx.set_lf_quantized(*wl.lf_q)
    ctx.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)
    ctx.set_groups_lf_only(every)
    ctx.frame_run()
    ctx.sync()
    got = ctx.read_planes()
    want = expected_planes(oracle, wl, every)
    assert not bit_equal(want[1][:8], want[1][65536:65544])  # the tail is not a copy of the head
    assert_planes(got, want, "16 x 65552")


# ---------------------------------------------------------------- argument and state errors
def test_argument_and_state_errors(ctx, oracle):
    import jxl_rs_amd
    from jxl_rs_amd import lib, synth
    INV, BAD, UNS = lib.ERR_INVALID_ARGUMENT, lib.ERR_BAD_STATE, lib.ERR_UNSUPPORTED
    wl = frame(520, 300)
    n = wl.xgroups * wl.ygroups
    begin(ctx, wl, [])
    assert ctx.try_set_groups_lf_only([n]) == INV
    assert ctx.try_set_groups_lf_only([0, 2, n]) == INV  # ... and neither 0 nor 2 is marked by the refused call
    assert ctx.try_set_groups_lf_only([]) == lib.OK
    assert ctx.L.jxlh_frame_set_groups_lf_only(ctx._ctx, None, 1) == INV
    ctx.frame_run()
    ctx.sync()
    assert_planes(ctx.read_planes(), run_oracle_frame(oracle, wl)[0], "refused calls mark nothing")
    # a Modular frame, a chroma-subsampled frame
    mp = ctx.default_params(40, 24)
    mp.gab, mp.epf_iters = 0, 0
    ctx.modular_frame_begin(mp)
    assert ctx.try_set_groups_lf_only([0]) == BAD
    sub = synth.make_vardct(72, 40, mix=synth.MIX_8X8, seed=7, epf_iters=0, hshift=(1, 0, 1), vshift=(1, 0, 1))
    ctx.frame_begin(gpu_params_from(ctx, sub))
    assert ctx.try_set_groups_lf_only([0]) == UNS
    # no frame begun
    fresh = jxl_rs_amd.Context(0, 1)
    try:
        assert fresh.try_set_groups_lf_only([0]) == BAD
        assert fresh.try_set_groups_lf_only([]) == BAD
    finally:
        fresh.close()


def test_sharded_context_is_unsupported():
    import jxl_rs_amd
    from jxl_rs_amd import lib
    wl = frame(300, 520)
    peers = [jxl_rs_amd.Context(0, 1) for _ in range(2)]
    try:
        lib.comm_init_local(peers)
        for c in peers:
            c.frame_begin(gpu_params_from(c, wl))
            assert c.try_set_groups_lf_only([0]) == lib.ERR_UNSUPPORTED
    finally:
        for c in peers:
            c.close()
