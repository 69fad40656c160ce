"""Progressive previews of a squeezed image in one call (jxlh_unsqueeze_chain_preview): images forward-squeezed in
default_squeeze order, the residuals of some levels withheld, the device planes against
squeeze_preview_ref.preview_reference -- every level, dead ones included, through the oracle's step functions, the way
the reference's step list runs them.  Bit exact: there are no tolerances."""
import functools
import os
import sys

import numpy as np
import pytest

from helpers import DeviceArray
from squeeze_preview_ref import explicit_steps, forward_chain, missing_flags, preview_kinds_ref, preview_reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = -0x5A5A5A5B
GUARD = 2   # canary rows above and below every output plane
SIZES = [(37, 29), (64, 64), (130, 65), (257, 96), (1, 40)]


@pytest.fixture(scope="module")
def ctx():
    from jxl_rs_amd import Context
    c = Context(0)
    yield c
    c.close()


class Chain:
    """an image's channels squeezed down to the base: host arrays"""

    def __init__(self, w, h, nch, directions=None, seed=0):
        from jxl_rs_amd import synth
        rng = np.random.default_rng([w, h, nch, seed])
        self.w, self.h, self.nch = w, h, nch
        self.image = [rng.integers(-4000, 4001, size=(h, w)).astype(np.int32) for _ in range(nch)]
        self.steps, _ = synth.default_squeeze_steps(w, h) if directions is None else explicit_steps(w, h, directions)
        self.base, self.residuals = forward_chain(self.image, self.steps)
        self.n = len(self.steps)

    def suffix(self, k):
        return tuple(i >= self.n - k for i in range(self.n))


@functools.lru_cache(maxsize=None)
def chain_of(w, h, nch, directions=None):
    return Chain(w, h, nch, directions)


_REFERENCES = {}


def reference(oracle, chain, missing, rct=None, cvt_rne=False):
    """computed once per case, shared, handed out as it is (the tests do not write to it)"""
    key = (id(chain), tuple(missing), rct, cvt_rne)
    if key not in _REFERENCES:
        _REFERENCES[key] = preview_reference(oracle, chain.base, chain.residuals, chain.steps, missing, rct, cvt_rne)
    return _REFERENCES[key]


class DeviceChain:
    """the chain's planes on the device: residual rows padded by res_pad samples of canary, bases `base_skew` samples
    into their allocations, output planes with out_pad canary samples behind every row and GUARD canary rows around"""

    def __init__(self, chain, res_pad=0, out_pad=0, base_skew=0):
        self.chain, self.out_pad = chain, out_pad
        self.bufs = []
        self.base = []
        for b in chain.base:
            d = self._keep(DeviceArray(nbytes=b.nbytes + 4 * base_skew))
            d.upload(b, 4 * base_skew)
            self.base.append(d.ptr + 4 * base_skew)
        self.res_host, self.res = [], []
        for planes in chain.residuals:
            hosts = []
            for r in planes:
                padded = np.full((max(r.shape[0], 1), max(r.shape[1], 1) + res_pad), CANARY, np.int32)
                padded[:r.shape[0], :r.shape[1]] = r
                hosts.append(padded)
            self.res_host.append(hosts)
            self.res.append([self._keep(DeviceArray(p)) for p in hosts])
        self.out_stride = chain.w + out_pad
        self.out = [self._keep(DeviceArray(np.full((chain.h + 2 * GUARD, self.out_stride), CANARY, np.int32)))
                    for _ in range(chain.nch)]
        self.out_ptr = [d.ptr + 4 * GUARD * self.out_stride for d in self.out]

    def _keep(self, d):
        self.bufs.append(d)
        return d

    def levels(self, missing, n_planes=None):
        n_planes = self.chain.nch if n_planes is None else n_planes
        return [(hz, ow, oh, [None] * 3 if m else [d.ptr for d in devs[:n_planes]] + [None] * (3 - n_planes), hosts[0].shape[1])
                for (hz, ow, oh), m, devs, hosts in zip(self.chain.steps, missing, self.res, self.res_host)]

    def run(self, ctx, missing, rct=None, cvt_rne=False, call="preview"):
        bw, bh = self.chain.base[0].shape[1], self.chain.base[0].shape[0]
        args = (self.levels(missing), self.base, bw, bw, bh, self.out_ptr, self.out_stride)
        if call == "preview":
            ctx.unsqueeze_chain_preview(*args, rct=rct, cvt_rne=cvt_rne)
        else:
            ctx.unsqueeze_chain(*args, rct=rct)
        ctx.sync()
        return self.result()

    def raw_out(self):
        n = (self.chain.h + 2 * GUARD) * self.out_stride
        return [d.download(np.int32, n).reshape(-1, self.out_stride) for d in self.out]

    def result(self):
        """the output planes; canaries around them and in their row padding, and the residual planes, unchanged"""
        planes = []
        for raw in self.raw_out():
            assert (raw[:GUARD] == CANARY).all() and (raw[GUARD + self.chain.h:] == CANARY).all(), "wrote outside the plane"
            assert (raw[:, self.chain.w:] == CANARY).all(), "wrote into the row padding"
            planes.append(raw[GUARD:GUARD + self.chain.h, :self.chain.w].copy())
        for devs, hosts in zip(self.res, self.res_host):
            for d, h in zip(devs, hosts):
                assert np.array_equal(d.download(np.int32, h.size).reshape(h.shape), h), "a residual plane changed"
        return planes

    def poison(self):
        for d in self.out:
            d.upload(np.full((self.chain.h + 2 * GUARD, self.out_stride), CANARY, np.int32))

    def free(self):
        for d in self.bufs:
            d.free()


def assert_planes(got, want, what):
    assert len(got) == len(want)
    for c, (g, e) in enumerate(zip(got, want)):
        assert g.shape == e.shape and np.array_equal(g, e), (what, c, np.argwhere(g != e)[:4], int((g != e).sum()))


@pytest.mark.parametrize("nch", [1, 3])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_missing_suffixes(ctx, oracle, size, nch):
    """1..5 missing levels: with default_squeeze's alternating directions five are 1-D, 2-D, 2-D, 2-D, 2-D with two
    dead levels; 1 x 40 squeezes vertically only, so every level is 1-D"""
    chain = chain_of(*size, nch)
    dev = DeviceChain(chain)
    try:
        for k in range(1, min(5, chain.n) + 1):
            missing = chain.suffix(k)
            assert_planes(dev.run(ctx, missing), reference(oracle, chain, missing), f"{size} x{nch}, {k} missing")
            dev.poison()
    finally:
        dev.free()


def test_the_cases_exercise_what_they_claim():
    """five missing levels of the larger images: 1-D + four 2-D with two dead levels, on even level numbers in one
    chain and odd ones in another; 1 x 40 squeezes one way only"""
    dead_parities = set()
    for size in ((64, 64), (130, 65), (257, 96)):
        chain = chain_of(*size, 1)
        kinds, _, live = preview_kinds_ref([s[0] for s in chain.steps], missing_flags(chain.steps, chain.suffix(5)))
        assert kinds[-5:] == [1, 2, 2, 2, 2], (size, kinds)
        dead = [i for i, lv in enumerate(live) if not lv]
        assert dead == [chain.n - 4, chain.n - 2], (size, dead)
        dead_parities |= {i % 2 for i in dead}
    assert dead_parities == {0, 1}
    chain = chain_of(1, 40, 1)
    assert set(preview_kinds_ref([s[0] for s in chain.steps], [True] * chain.n)[0]) == {1}


@pytest.mark.parametrize("directions,size", [((True, True, False, False), (70, 50)), ((False, False, True, True, True), (45, 70)),
                                             ((False, True, True), (33, 21))], ids=["HHVV", "VVHHH", "VHH"])
def test_neighbours_of_one_direction_stay_one_dimensional(ctx, oracle, directions, size):
    chain = chain_of(*size, 3, directions)
    kinds, _, _ = preview_kinds_ref(list(directions), [True] * chain.n)
    assert 1 in kinds[1:] and 2 in kinds, kinds   # a same-direction pair, and a 2-D level next to it
    dev = DeviceChain(chain)
    try:
        for k in range(1, chain.n + 1):
            missing = chain.suffix(k)
            assert_planes(dev.run(ctx, missing), reference(oracle, chain, missing), f"{directions}, {k} missing")
            dev.poison()
    finally:
        dev.free()


@pytest.mark.parametrize("rct", [None, (6, 0)], ids=["plain", "rct"])
def test_a_present_level_behind_missing_ones(ctx, oracle, rct):
    """holes: the regular step runs on smooth planes; with the last level present the RCT takes the regular fused route"""
    chain = chain_of(130, 65, 3)
    n = chain.n
    dev = DeviceChain(chain)
    try:
        for holes in ({n - 3}, {n - 2, n - 3}, {n - 4, n - 5, n - 1}, {0}, {1, 2, n - 2}):
            missing = tuple(i in holes for i in range(n))
            assert_planes(dev.run(ctx, missing, rct=rct), reference(oracle, chain, missing, rct), f"missing {sorted(holes)}")
            dev.poison()
    finally:
        dev.free()


@pytest.mark.parametrize("size", [(130, 65), (1, 40), (300, 280)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_nothing_missing_is_the_chain_call(ctx, oracle, size):
    chain = chain_of(*size, 3)
    dev = DeviceChain(chain)
    try:
        for rct in (None, (6, 0)):
            got = dev.run(ctx, chain.suffix(0), rct=rct)
            dev.poison()
            assert_planes(got, dev.run(ctx, chain.suffix(0), rct=rct, call="chain"), f"rct {rct}")
            dev.poison()
            assert_planes(got, oracle.rct(chain.image, *rct) if rct else chain.image, "the image comes back")
    finally:
        dev.free()


@pytest.mark.parametrize("perm", [0, 5])
@pytest.mark.parametrize("op", [0, 6])
def test_rct_fused_into_the_last_level(ctx, oracle, op, perm):
    """a smooth last level takes k6_smooth_unsqueeze_rct (1-D horizontal, 1-D vertical and 2-D), a regular one the
    chain's fused step; either way the planes are those of the preview without an RCT followed by jxlh_rct"""
    cases = [(chain_of(130, 65, 3), 1), (chain_of(130, 65, 3), 3), (chain_of(64, 64, 3), 1), (chain_of(257, 96, 3), 2)]
    for chain, k in cases:
        dev = DeviceChain(chain)
        try:
            for missing in (chain.suffix(k), tuple(i == chain.n - 2 for i in range(chain.n))):   # smooth last / regular last
                got = dev.run(ctx, missing, rct=(op, perm))
                dev.poison()
                assert_planes(got, reference(oracle, chain, missing, (op, perm)), f"{chain.w} x {chain.h}, {missing}")
                plain = dev.run(ctx, missing)
                dev.poison()
                assert_planes(got, ctx.rct(plain, op, perm), "unfused: preview, then jxlh_rct")
        finally:
            dev.free()
    kinds = [preview_kinds_ref([s[0] for s in c.steps], c.suffix(k))[0][-1] for c, k in cases]
    lasts = [(kd, c.steps[-1][0]) for kd, (c, _) in zip(kinds, cases)]
    assert {(1, True), (1, False)} <= set(lasts) and any(kd == 2 for kd, _ in lasts), lasts


@pytest.mark.parametrize("nch", [1, 3])
def test_both_rounding_modes(ctx, oracle, nch):
    chain = chain_of(257, 96, nch)
    dev = DeviceChain(chain)
    try:
        rct = (6, 0) if nch == 3 else None
        for k in (1, 4):
            missing = chain.suffix(k)
            trunc = dev.run(ctx, missing, rct=rct)
            dev.poison()
            rne = dev.run(ctx, missing, rct=rct, cvt_rne=True)
            dev.poison()
            assert_planes(trunc, reference(oracle, chain, missing, rct, False), f"truncating, {k} missing")
            assert_planes(rne, reference(oracle, chain, missing, rct, True), f"nearest even, {k} missing")
            differing = np.mean([(a != b).mean() for a, b in zip(trunc, rne)])
            assert differing > 0.1, differing   # the two reference builds really differ
    finally:
        dev.free()


@pytest.mark.parametrize("size", [(37, 29), (130, 65), (257, 96)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_padded_strides_and_unaligned_planes(ctx, oracle, size):
    """output rows wider than the image by an odd count (the pair stores give way to single ones), residual rows padded,
    bases four bytes off 16-byte alignment (the prefix takes its 4-byte movers): same planes, canaries untouched"""
    chain = chain_of(*size, 3)
    want = {k: reference(oracle, chain, chain.suffix(k), (6, 0)) for k in (1, 2, 5)}
    for res_pad, out_pad, skew in ((3, 7, 0), (0, 0, 1), (5, 2, 1), (4, 4, 0)):
        dev = DeviceChain(chain, res_pad=res_pad, out_pad=out_pad, base_skew=skew)
        try:
            for k in want:
                assert_planes(dev.run(ctx, chain.suffix(k), rct=(6, 0)), want[k], f"pads {res_pad} {out_pad} skew {skew}, {k} missing")
                dev.poison()
        finally:
            dev.free()


def test_equals_the_route_of_single_calls(ctx, oracle):
    """130 x 65 x 3, four levels missing: jxlh_unsqueeze_chain for the prefix, jxlh_smooth_unsqueeze per level and
    plane, jxlh_rct -- what a caller had to issue before -- gives the same planes"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_squeeze_preview import ManualRoute
    chain = chain_of(130, 65, 3)
    dev = DeviceChain(chain)
    try:
        for cvt_rne in (False, True):
            missing = chain.suffix(4)
            got = dev.run(ctx, missing, rct=(6, 0), cvt_rne=cvt_rne)
            dev.poison()
            bw, bh = chain.base[0].shape[1], chain.base[0].shape[0]
            manual = ManualRoute(ctx, dev.levels(missing), dev.base, bw, bw, bh, dev.out_ptr, dev.out_stride, (6, 0), cvt_rne)
            manual.run()
            ctx.sync()
            manual.free()
            assert_planes(got, dev.result(), f"cvt_rne {cvt_rne}")
            dev.poison()
    finally:
        dev.free()


def test_preview_planes_feed_a_modular_frame(ctx, oracle):
    """end to end: ModularChain.preview leaves device planes that go straight into jxlh_frame_set_modular_channels of a
    Modular frame with Gaborish + EPF; the rendered planes are the oracle's stages on preview_reference's planes"""
    from jxl_rs_amd.modular import ModularChain
    from jxl_rs_amd import synth
    from test_gpu_modular_frame import _assert_planes, _convert, _filters, _params, _samples
    w, h = 96, 80
    r, g, b = [p.astype(np.int64) for p in _samples(np.random.default_rng(3), w, h)]
    co = r - b                       # forward YCoCg (the inverse is RCT op 6, rct.rs:118-157)
    tmp = b + (co >> 1)
    cg = g - tmp
    coded = [(tmp + (cg >> 1)).astype(np.int32), co.astype(np.int32), cg.astype(np.int32)]
    steps, _ = synth.default_squeeze_steps(w, h)
    base, residuals = forward_chain(coded, steps)
    mc = ModularChain(ctx, w, h, rct=(6, 0), planes=(base, residuals, steps))
    try:
        for k in (2, 3):
            missing = [i >= len(steps) - k for i in range(len(steps))]
            planes = preview_reference(oracle, base, residuals, steps, missing, (6, 0))
            want = _filters(oracle, _convert(oracle, planes, 8), 1, 2, 0.7)
            ctx.modular_frame_begin(_params(ctx, w, h, 1, 2, epf_sigma_for_modular=0.7))
            d = mc.preview(len(steps) - k)
            ctx.set_modular_channels(*[p.ptr for p in d], 8, w=w, h=h, stride=w)
            ctx.frame_run()
            ctx.sync()
            _assert_planes(ctx.read_planes(), want, f"{k} levels missing")
    finally:
        mc.free()


def test_argument_errors_launch_nothing(ctx):
    from jxl_rs_amd import lib, JxlHipError
    chain = chain_of(130, 65, 3)
    dev = DeviceChain(chain)
    bw, bh = chain.base[0].shape[1], chain.base[0].shape[0]
    n = chain.n
    good = dev.levels(chain.suffix(2))

    def refused(levels=good, base=None, bw_=bw, out=None, out_stride=None, **kw):
        with pytest.raises(JxlHipError) as e:
            ctx.unsqueeze_chain_preview(levels, dev.base if base is None else base, bw_, bw_, bh,
                                        dev.out_ptr if out is None else out, dev.out_stride if out_stride is None else out_stride, **kw)
        assert e.value.status == lib.ERR_INVALID_ARGUMENT

    try:
        partly = list(good)
        hz, ow, oh, res, rs = good[n - 3]
        partly[n - 3] = (hz, ow, oh, [res[0], None, res[2]], rs)
        refused(partly)                                            # a level with some planes named
        refused(flags=0x200)                                       # an unknown flag
        refused(flags=lib.SMOOTH_CVT_NEAREST_EVEN | 1)
        refused(rct=(7, 0))
        refused(rct=(6, 6))
        refused(base=dev.base[:1], out=dev.out_ptr[:1], levels=dev.levels(chain.suffix(2), 1), rct=(6, 0))   # an RCT of one plane
        refused(bw_=bw + 1)                                        # geometry
        refused(out_stride=chain.w - 1)
        wrong = list(good)
        wrong[n - 1] = (good[n - 1][0], good[n - 1][1] + 2, good[n - 1][2], good[n - 1][3], good[n - 1][4])
        refused(wrong)                                             # ... also of a missing level
        host = np.zeros((bh, bw), np.int32)
        refused(base=[host, host, host])                           # a host pointer
        present = list(good)
        present[0] = (good[0][0], good[0][1], good[0][2], good[0][3], 0)
        refused(present)                                           # a present level's stride
        refused(levels=[])
        # the chain call still refuses what it refused
        with pytest.raises(JxlHipError) as e:
            ctx.unsqueeze_chain(good, dev.base, bw, bw, bh, dev.out_ptr, dev.out_stride)
        assert e.value.status == lib.ERR_INVALID_ARGUMENT
        ctx.sync()
        for raw in dev.raw_out():
            assert (raw == CANARY).all()
    finally:
        dev.free()
