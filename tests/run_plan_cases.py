"""The cases behind tests/test_gpu_run_plan.py and tools/record_run_launches.py: what a frame run enqueues and what it
leaves in the planes, for every stage list and every way a run is routed (csrc/run_plan.h).  A case runs on a 40 x 600
frame (1 x 3 groups: the smallest with an interior group row that has a halo on both sides) and yields the timer scope
names with their launch counts plus a SHA-256 of read_planes()."""
import hashlib

import numpy as np

W, H = 40, 600
UNFUSED, STRIP = 1, 4  # JXLH_FRAME_UNFUSED_FILTERS, JXLH_FRAME_STRIP
SCENARIOS = ("whole", "band", "rerender", "rerender_first")


def _case(name, **kw):
    c = dict(name=name, kind="vardct", gab=1, epf=2, flags=0, scenario="whole", spline=False, noise=False, sub420=False,
             lf_only=())
    c.update(kw)
    return c


CASES = [_case(f"gab{g}_epf{e}_{'single' if u else 'fused'}_{s}", gab=g, epf=e, flags=UNFUSED if u else 0, scenario=s)
         for g in (0, 1) for e in (0, 1, 2, 3) for u in (0, 1) for s in SCENARIOS]
CASES += [
    _case("spline_band_result_in_tmp", spline=True, scenario="band"),           # the band stays a band
    _case("spline_band_result_in_planes", epf=3, spline=True, scenario="band"),  # ... becomes the whole frame
    _case("noise_rerender_no_stage", gab=0, epf=0, noise=True, scenario="rerender"),  # in place: a full run
    _case("noise_rerender_filtered", noise=True, scenario="rerender"),
    _case("strip_eligible", flags=STRIP),
    _case("strip_ineligible", epf=3, flags=STRIP),
    _case("lazy_chroma_420", gab=0, epf=0, sub420=True),
    _case("lf_only_group", lf_only=(1,)),
    _case("modular_band_epf3", kind="modular", epf=3, scenario="band"),
]

_workloads = {}


def _workload(sub420):
    from jxl_rs_amd import synth
    if sub420 not in _workloads:
        kw = dict(mix=synth.MIX_8X8, hshift=(1, 0, 1), vshift=(1, 0, 1)) if sub420 else dict(mix=synth.MIX_D1)
        _workloads[sub420] = synth.make_vardct(W, H, seed=40600, **kw)
    return _workloads[sub420]


def _splines():
    """segments across both group-row seams and inside the middle group row"""
    seg = [[20.0, 255.0, 6.0, 0.7, 0.3, 0.4, -0.3, 0.2], [8.0, 384.0, 9.0, 0.5, 0.4, 0.2, 0.3, -0.1],
           [30.0, 513.0, 5.0, 0.9, 0.25, -0.2, 0.1, 0.3]]
    return np.asarray(seg, dtype=np.float32)


def _modular_samples(seed=0):
    """8-bit samples the filters act on: a slope, edges along the block grid, one step of noise"""
    rng = np.random.default_rng([0x52504C, seed])
    out = []
    for _ in range(3):
        a = rng.integers(0, 2, size=(H, W)).astype(np.int64)
        a += (np.arange(W)[None, :] + 2 * np.arange(H)[:, None]) // 6 % 64
        a += 16 * ((np.arange(W) // 16 % 2)[None, :] ^ (np.arange(H) // 8 % 2)[:, None])
        out.append(a.astype(np.int32))
    return out


def _second_call(ctx, case, resubmit):
    s = case["scenario"]
    if s != "rerender_first":
        ctx.frame_run()
    if s == "whole":
        return
    if s != "rerender_first":
        resubmit()  # group row 1 changes: the second call's rows show in the planes
    if s == "band":
        ctx.frame_run(1, 2)
    else:
        ctx.rerender_groups([1])


def run_case(ctx, case):
    """-> {"launches": {scope: count}, "sha256": hex digest of the three planes}"""
    ctx.kernel_timing(True)
    ctx.kernel_timing_reset()
    try:
        p = ctx.default_params(W, H)
        p.gab, p.epf_iters, p.flags = case["gab"], case["epf"], case["flags"]
        if case["noise"]:
            p.noise, p.visible_frame_index = 1, 1
            for i in range(8):
                p.noise_lut[i] = 0.05 + 0.01 * i
        if case["kind"] == "modular":
            chans, other = _modular_samples(0), _modular_samples(1)
            ctx.modular_frame_begin(p)
            ctx.set_modular_channels(*chans, 8)
            _second_call(ctx, case, lambda: ctx.set_modular_channels(*[c[256:512] for c in other], 8, y0=256))
        else:
            wl = _workload(case["sub420"])
            for c in range(3):
                p.hshift[c], p.vshift[c] = wl.opts["hshift"][c], wl.opts["vshift"][c]
            ctx.frame_begin(p)
            ctx.set_dequant_tables(wl.tables)
            ctx.set_lf_quantized(*wl.lf_q)
            ctx.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)
            if case["lf_only"]:
                ctx.set_groups_lf_only(list(case["lf_only"]))
            if case["spline"]:
                ctx.set_splines(_splines())
            for g in range(wl.coeffs.shape[0]):
                if g not in case["lf_only"]:
                    ctx.submit_group(g, wl.coeffs[g])
            ctx.slot_wait(0)

            def resubmit():
                ctx.submit_group(1, wl.coeffs[0])
                ctx.slot_wait(0)
            _second_call(ctx, case, resubmit)
        ctx.sync()
        sha = hashlib.sha256()
        for plane in ctx.read_planes():  # (inside the timed part: a deferred chroma upsampling runs here)
            sha.update(np.ascontiguousarray(plane, dtype=np.float32).tobytes())
        launches = {k: v[1] for k, v in sorted(ctx.kernel_times().items())}
        return {"launches": launches, "sha256": sha.hexdigest()}
    finally:
        ctx.kernel_timing(False)
        ctx.kernel_timing_reset()
