// C ABI, Squeeze: single steps, fused chains (squeeze_plan.h), progressive previews of a chain by whole levels and by
// grid cells (squeeze_preview_plan.h), and the smooth steps on their own.  Every chain call is: validate, plan, issue.
#include <algorithm>
#include <cstring>
#include <optional>

#include "jxlh_ctx.h"
#include "squeeze_preview_plan.h"

namespace {
using namespace jxlh;

// a single squeeze step as squeeze_plan.h and the launchers read it (res: already the planes the kernel reads)
SqueezeStep step_of(int horizontal, int n_planes, const int32_t* const avg[], size_t avg_stride, const int32_t* const res[],
                    size_t res_stride, uint32_t out_w, uint32_t out_h, int32_t* const out[], size_t out_stride) {
  SqueezeStep s{horizontal != 0, n_planes, out_w, out_h, avg_stride, res_stride, out_stride, {}, {}, {}};
  for (int p = 0; p < n_planes; p++) {
    s.avg[p] = (uintptr_t)avg[p];
    s.res[p] = (uintptr_t)res[p];
    s.out[p] = (uintptr_t)out[p];
  }
  return s;
}
// one planned launch of a single level: the step, the step fused with the RCT, or the RCT on the step's output
void issue_step(hipStream_t s, const SqueezeLaunch& L, const SqueezeStep& st, int rct_op, int rct_perm) {
  int32_t* const o[3] = {(int32_t*)st.out[0], (int32_t*)st.out[1], (int32_t*)st.out[2]};
  switch (L.kind) {
    case SqueezeLaunch::kFusedRct: return launch_unsqueeze_rct(s, L, st, rct_op, rct_perm);
    case SqueezeLaunch::kRctFlat: return launch_rct(s, o[0], o[1], o[2], (size_t)st.out_w * st.out_h, rct_op, rct_perm);
    case SqueezeLaunch::kRctRows: return launch_rct_rows(s, o[0], o[1], o[2], st.out_w, st.out_h, st.out_stride, rct_op, rct_perm);
    default: return launch_unsqueeze(s, L, st);
  }
}
// JXLH_SEPARATE_RCT=1, JXLH_CHAIN_FLOW=0 (tests, A/B): read on every call
bool env_is(const char* name, char v) { return getenv(name) && *getenv(name) == v; }
// a planned chain (squeeze_plan.h) onto the context's stream; in.arena is the context's hook_i[0]
jxlh_status issue_chain(jxlh_ctx* ctx, const SqueezeChainIn& in, const SqueezePlan& plan, int rct_op, int rct_perm) {
  jxlh_status st;
  const int n_planes = in.n_planes;
  const jxlh_squeeze_level* levels = in.levels;
  const int32_t* base[3];
  for (int p = 0; p < n_planes; p++) base[p] = (const int32_t*)in.base[p];
  if (plan.flow_words) {
    if ((st = ensure(ctx, ctx->flow_words, plan.flow_words))) return st;
    if (!ctx->host_flow_flag.p) {
      // the error word lives in pinned host memory (device-visible under the same address): jxlh_ctx_sync AND
      // jxlh_ctx_wait_mark read it without queueing a copy behind later work
      HIPCHK(ctx, ctx->host_flow_flag.alloc(1));
      *ctx->host_flow_flag.p = 0;
    }
    if (ctx->flow_prof_on && (st = ensure(ctx, ctx->flow_prof, 11 * (size_t)kFlowMaxLevels))) return st;
  }
  ScopedKernelTimer t(ctx, "k6_unsqueeze_chain");
  for (int k = 0; k < plan.n; k++) {
    const SqueezeLaunch& L = plan.launch[k];
    if (L.kind == SqueezeLaunch::kLevels) {
      int32_t* dst[3];
      for (int p = 0; p < n_planes; p++) dst[p] = (int32_t*)squeeze_plane_addr(in, plan.arena, L.dst, p);
      launch_unsqueeze_levels(ctx->stream, n_planes, L.n_levels, levels, base, in.base_stride, in.base_w, in.base_h, dst, L.dst.stride);
    } else if (L.kind == SqueezeLaunch::kFlow) {
      SqueezeStep steps[kFlowRunCap];
      SqueezeLoc a = L.src;
      for (int n = 0; n < L.n_levels; n++) {  // every level of the run but its last writes its own plane set
        const int j = L.level0 + n;
        const SqueezeLoc d = n == L.n_levels - 1 ? L.dst : SqueezeLoc{j, plan.arena.stride[j]};
        steps[n] = squeeze_level_step(in, plan.arena, j, a, d);
        a = d;
      }
      launch_unsqueeze_flow(ctx->stream, L.n_levels, steps, plan.vec + L.level0, ctx->flow_words.p, ctx->host_flow_flag.p, 4.0f,
                            ctx->flow_prof_on ? ctx->flow_prof.p : nullptr);
      ctx->flow_prof_levels = L.n_levels;
      ctx->flow_used = true;
    } else {
      issue_step(ctx->stream, L, squeeze_level_step(in, plan.arena, L.level0, L.src, L.dst), rct_op, rct_perm);
    }
  }
  HIPCHK(ctx, hipGetLastError());
  return JXLH_OK;
}
// What the three chain calls do before they plan: the RCT and the flags, the chain's arguments (a preview's levels may
// be missing) and a per-cell preview's grids, the arena -> *in, what they plan from
enum ChainCall { kChain, kPreview, kPreviewTiles };
jxlh_status chain_begin(jxlh_ctx* ctx, ChainCall call, int n_planes, int n_levels, const jxlh_squeeze_level* levels,
                        const jxlh_squeeze_tiles* tiles, const int32_t* const base[], size_t base_stride, uint32_t base_w, uint32_t base_h,
                        int32_t* const out[], size_t out_stride, int rct_op, int rct_perm, uint32_t flags, SqueezeChainIn* in) {
  const bool with_rct = rct_op >= 0;
  if (!ctx || (with_rct && (n_planes != 3 || rct_op > 6 || rct_perm < 0 || rct_perm > 5)) ||
      (flags != 0 && flags != JXLH_SMOOTH_CVT_NEAREST_EVEN))
    return JXLH_ERR_INVALID_ARGUMENT;
  jxlh_status st;
  if ((st = check_squeeze_chain(n_planes, n_levels, levels, base, base_stride, base_w, base_h, out, out_stride, is_device_ptr, call != kChain)))
    return st;
  if (call == kPreviewTiles && (st = check_squeeze_tiles(n_levels, levels, tiles))) return st;
  if ((st = ensure(ctx, ctx->hook_i[0], std::max<size_t>(squeeze_arena(n_planes, n_levels, levels).total, 1)))) return st;
  *in = {n_planes, n_levels, levels, base_w, base_h, base_stride, out_stride, {}, {}, (uintptr_t)ctx->hook_i[0].p,
         with_rct, env_is("JXLH_SEPARATE_RCT", '1'), !env_is("JXLH_CHAIN_FLOW", '0')};
  for (int p = 0; p < n_planes; p++) {
    in->base[p] = (uintptr_t)base[p];
    in->out[p] = (uintptr_t)out[p];
  }
  return JXLH_OK;
}
// the chain's geometry and NULL rules for the two *_kinds calls: no planes are named there, so every pointer passes for
// a device one
jxlh_status check_kinds_geometry(int n_planes, int n_levels, const jxlh_squeeze_level* levels, uint32_t base_w, uint32_t base_h) {
  static const int32_t some = 0;
  const int32_t* const base[3] = {&some, &some, &some};
  int32_t* const out[3] = {const_cast<int32_t*>(&some), const_cast<int32_t*>(&some), const_cast<int32_t*>(&some)};
  return check_squeeze_chain(n_planes, n_levels, levels, base, base_w, base_w, base_h, out, (size_t)kMaxModularDim,
                             [](const void*) { return true; }, true);
}
// A planned preview (squeeze_preview_plan.h) onto the context's stream: the work lists in one copy, the regular prefix as
// the chain it is, then per live level its whole-level launch or its two list launches, in stream order.  One timer per
// launch group: whole levels under the preview call's name, the list launches under their kernels'
jxlh_status issue_preview(jxlh_ctx* ctx, const SqueezeChainIn& in, const SqueezePreviewPlan& plan, int rct_op, int rct_perm, uint32_t flags) {
  if (plan.too_large) return JXLH_ERR_UNSUPPORTED;
  jxlh_status st;
  const int n_planes = in.n_planes;
  if (const size_t n_rec = plan.records.size()) {  // the lists: one pinned block, one copy
    if ((st = ensure(ctx, ctx->sq_tiles_dev, n_rec))) return st;
    Pinned<int4>& host = ctx->sq_tiles_host[ctx->sq_tiles_next];
    Fence& copied = ctx->sq_tiles_copied[ctx->sq_tiles_next];
    ctx->sq_tiles_next = (ctx->sq_tiles_next + 1) % jxlh_ctx::kSqTilesRing;
    HIPCHK(ctx, copied.sync());  // the block's previous lists are on the device
    copied.clear();
    if (host.n < n_rec) {
      HIPCHK(ctx, host.reset());
      HIPCHK(ctx, host.alloc(n_rec + n_rec / 2));
    }
    static_assert(sizeof(SqTileRecord) == sizeof(int4), "the lists are 16-byte records");
    std::memcpy(host.p, plan.records.data(), n_rec * sizeof(int4));
    HIPCHK(ctx, hipMemcpyAsync(ctx->sq_tiles_dev.p, host.p, n_rec * sizeof(int4), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, copied.record(ctx->stream));
  }
  if (plan.n_prefix > 0 && (st = issue_chain(ctx, plan.prefix_in, plan.prefix, rct_op, rct_perm))) return st;
  for (int k = 0; k < plan.n; k++) {
    const PreviewEntry& e = plan.entry[k];
    const jxlh_squeeze_level& lv = in.levels[e.level];
    const SqueezeStep step = squeeze_level_step(in, plan.arena, e.level, e.src, e.dst);
    if (e.kind == JXLH_PREVIEW_REGULAR) {
      ScopedKernelTimer t(ctx, "k6_unsqueeze_chain_preview");
      for (int j = 0; j < e.n_launch; j++) issue_step(ctx->stream, e.launch[j], step, rct_op, rct_perm);
      continue;
    }
    const int32_t* src[3] = {};
    const int32_t* src2[3] = {};
    int32_t* dst[3] = {};
    for (int p = 0; p < n_planes; p++) {
      src[p] = (const int32_t*)squeeze_plane_addr(in, plan.arena, e.src, p);
      src2[p] = (const int32_t*)squeeze_plane_addr(in, plan.arena, e.src2, p);
      dst[p] = (int32_t*)squeeze_plane_addr(in, plan.arena, e.dst, p);
    }
    if (e.kind >= 0) {  // every cell smooth, of one kind: the whole-level launch
      const bool two_d = e.kind == JXLH_PREVIEW_SMOOTH_2D;
      ScopedKernelTimer t(ctx, "k6_unsqueeze_chain_preview");
      launch_smooth_unsqueeze_planes(ctx->stream, two_d ? JXLH_SMOOTH_2D : lv.horizontal ? JXLH_SMOOTH_H : JXLH_SMOOTH_V, n_planes,
                                     two_d ? src2 : src, two_d ? e.src2.stride : e.src.stride, (int)(two_d ? e.src2_w : e.src_w),
                                     (int)(two_d ? e.src2_h : e.src_h), dst, e.dst.stride, (int)lv.out_w, (int)lv.out_h, flags != 0,
                                     e.rct ? rct_op : -1, rct_perm);
      continue;
    }
    const int4* lists = ctx->sq_tiles_dev.p;
    if (e.n_smooth) {
      ScopedKernelTimer t(ctx, "k6_smooth_unsqueeze_cells");
      launch_smooth_unsqueeze_cells(ctx->stream, lv.horizontal != 0, n_planes, src, e.src.stride, (int)e.src_w, (int)e.src_h, src2,
                                    e.src2.stride, (int)e.src2_w, (int)e.src2_h, dst, e.dst.stride,
                                    reinterpret_cast<const SqTileSmoothCell*>(lists + e.smooth_off), e.n_smooth, e.tiles_x, e.tiles_per_cell,
                                    flags != 0);
    }
    if (e.n_runs) {
      ScopedKernelTimer t(ctx, "k6_unsqueeze_runs");
      launch_unsqueeze_runs(ctx->stream, step, reinterpret_cast<const SqTileRun*>(lists + e.runs_off), e.n_runs, e.groups_per_run);
    }
    if (e.rct) {
      ScopedKernelTimer t(ctx, "k4_rct");
      if (e.dst.stride == lv.out_w) launch_rct(ctx->stream, dst[0], dst[1], dst[2], (size_t)lv.out_w * lv.out_h, rct_op, rct_perm);
      else launch_rct_rows(ctx->stream, dst[0], dst[1], dst[2], lv.out_w, lv.out_h, e.dst.stride, rct_op, rct_perm);
    }
  }
  HIPCHK(ctx, hipGetLastError());
  return JXLH_OK;
}
}  // namespace

extern "C" {

jxlh_status jxlh_unsqueeze(jxlh_ctx* ctx, int32_t horizontal, const int32_t* avg, size_t avg_stride,
                           const int32_t* res, size_t res_stride, uint32_t out_w, uint32_t out_h, int32_t* out,
                           size_t out_stride) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !avg || !out || out_stride < out_w) return JXLH_ERR_INVALID_ARGUMENT;
  if (out_w == 0 || out_h == 0) return JXLH_OK;
  if (out_w > kMaxModularDim || out_h > kMaxModularDim) return JXLH_ERR_UNSUPPORTED;
  const SqueezeExtents e = squeeze_extents(horizontal != 0, out_w, out_h);
  if (avg_stride < e.avg_w || (e.has_res && (!res || res_stride < e.res_w))) return JXLH_ERR_INVALID_ARGUMENT;
  auto run = [&](const int32_t* a, const int32_t* r, int32_t* o) {
    const int32_t* av[1] = {a};
    const int32_t* rv[1] = {r};
    int32_t* ov[1] = {o};
    const SqueezeStep st = step_of(horizontal, 1, av, avg_stride, rv, res_stride, out_w, out_h, ov, out_stride);
    launch_unsqueeze(ctx->stream, plan_squeeze_step(st), st);
  };
  if (is_device_ptr(avg) && is_device_ptr(out) && (!e.has_res || is_device_ptr(res))) {
    ScopedKernelTimer t(ctx, horizontal ? "k6_unsqueeze_h" : "k6_unsqueeze_v");
    run(avg, res ? res : avg, out);
    HIPCHK(ctx, hipGetLastError());
    return JXLH_OK;
  }
  jxlh_status st;
  if ((st = stage_in(ctx, ctx->hook_i[0], avg, avg_stride * e.avg_h))) return st;
  const size_t res_n = e.has_res ? res_stride * e.res_h : 0;
  if (res_n) {
    if ((st = stage_in(ctx, ctx->hook_i[1], res, res_n))) return st;
  } else if ((st = ensure(ctx, ctx->hook_i[1], 1))) {
    return st;
  }
  if ((st = ensure(ctx, ctx->hook_i[2], out_stride * out_h))) return st;
  run(ctx->hook_i[0].p, ctx->hook_i[1].p, ctx->hook_i[2].p);
  HIPCHK(ctx, hipGetLastError());
  return stage_out(ctx, out, (const int32_t*)ctx->hook_i[2].p, out_stride * out_h);
}

jxlh_status jxlh_unsqueeze_levels(jxlh_ctx* ctx, int32_t n_planes, int32_t n_levels, const jxlh_squeeze_level* levels,
                                  const int32_t* const base[], size_t base_stride, uint32_t base_w, uint32_t base_h,
                                  int32_t* const out[], size_t out_stride) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx) return JXLH_ERR_INVALID_ARGUMENT;
  if (jxlh_status st = check_squeeze_chain(n_planes, n_levels, levels, base, base_stride, base_w, base_h, out, out_stride,
                                           is_device_ptr))
    return st;
  if (squeeze_levels_fit(n_levels, levels, base_w, base_h)) {
    ScopedKernelTimer t(ctx, "k6_unsqueeze_levels");
    launch_unsqueeze_levels(ctx->stream, n_planes, n_levels, levels, base, base_stride, base_w, base_h, out, out_stride);
    HIPCHK(ctx, hipGetLastError());
    return JXLH_OK;
  }
  // anything else: the chain's route without an RCT (LDS-resident prefix, the streamed levels as one dataflow launch)
  return jxlh_unsqueeze_chain(ctx, n_planes, n_levels, levels, base, base_stride, base_w, base_h, out, out_stride, -1, 0);
}

// The inverse of a whole squeeze transform as one call (+ the RCT that follows it in the transform list): validate,
// plan (squeeze_plan.h), issue.
jxlh_status jxlh_unsqueeze_chain(jxlh_ctx* ctx, int32_t n_planes, int32_t n_levels, const jxlh_squeeze_level* levels,
                                 const int32_t* const base[], size_t base_stride, uint32_t base_w, uint32_t base_h,
                                 int32_t* const out[], size_t out_stride, int32_t rct_op, int32_t rct_perm) {
  JXLH_ON_DEVICE(ctx);
  SqueezeChainIn in;
  if (jxlh_status st = chain_begin(ctx, kChain, n_planes, n_levels, levels, nullptr, base, base_stride, base_w, base_h, out, out_stride,
                                   rct_op, rct_perm, 0, &in))
    return st;
  return issue_chain(ctx, in, plan_squeeze_chain(in), rct_op, rct_perm);
}

jxlh_status jxlh_squeeze_preview_kinds(int32_t n_planes, int32_t n_levels, const jxlh_squeeze_level* levels, uint32_t base_w,
                                       uint32_t base_h, uint8_t* kinds, uint8_t* live) {
  if (!kinds) return JXLH_ERR_INVALID_ARGUMENT;
  if (jxlh_status st = check_kinds_geometry(n_planes, n_levels, levels, base_w, base_h)) return st;
  squeeze_preview_kinds(n_planes, n_levels, levels, kinds, live);
  return JXLH_OK;
}

jxlh_status jxlh_squeeze_tile_kinds(int32_t n_planes, int32_t n_levels, const jxlh_squeeze_level* levels,
                                    const jxlh_squeeze_tiles* tiles, uint32_t base_w, uint32_t base_h, int32_t level, uint8_t* kinds) {
  if (!kinds) return JXLH_ERR_INVALID_ARGUMENT;
  if (jxlh_status st = check_kinds_geometry(n_planes, n_levels, levels, base_w, base_h)) return st;
  if (jxlh_status st = check_squeeze_tiles(n_levels, levels, tiles)) return st;
  if (level < 0 || level >= n_levels) return JXLH_ERR_INVALID_ARGUMENT;
  squeeze_tile_kinds(n_planes, levels, tiles, level, kinds);
  return JXLH_OK;
}

// A progressive preview of a whole squeeze transform, by whole levels: the per-cell call whose every level is one cell
jxlh_status jxlh_unsqueeze_chain_preview(jxlh_ctx* ctx, int32_t n_planes, int32_t n_levels, const jxlh_squeeze_level* levels,
                                         const int32_t* const base[], size_t base_stride, uint32_t base_w, uint32_t base_h,
                                         int32_t* const out[], size_t out_stride, int32_t rct_op, int32_t rct_perm, uint32_t flags) {
  JXLH_ON_DEVICE(ctx);
  SqueezeChainIn in;
  if (jxlh_status st = chain_begin(ctx, kPreview, n_planes, n_levels, levels, nullptr, base, base_stride, base_w, base_h, out, out_stride,
                                   rct_op, rct_perm, flags, &in))
    return st;
  return issue_preview(ctx, in, plan_squeeze_preview(in, nullptr), rct_op, rct_perm, flags);
}

// ... per grid cell
jxlh_status jxlh_unsqueeze_chain_preview_tiles(jxlh_ctx* ctx, int32_t n_planes, int32_t n_levels, const jxlh_squeeze_level* levels,
                                               const jxlh_squeeze_tiles* tiles, const int32_t* const base[], size_t base_stride,
                                               uint32_t base_w, uint32_t base_h, int32_t* const out[], size_t out_stride,
                                               int32_t rct_op, int32_t rct_perm, uint32_t flags) {
  JXLH_ON_DEVICE(ctx);
  SqueezeChainIn in;
  if (jxlh_status st = chain_begin(ctx, kPreviewTiles, n_planes, n_levels, levels, tiles, base, base_stride, base_w, base_h, out,
                                   out_stride, rct_op, rct_perm, flags, &in))
    return st;
  return issue_preview(ctx, in, plan_squeeze_preview(in, tiles), rct_op, rct_perm, flags);
}

jxlh_status jxlh_unsqueeze_rct(jxlh_ctx* ctx, int32_t horizontal, const int32_t* const avg[3], size_t avg_stride,
                               const int32_t* const res[3], size_t res_stride, uint32_t out_w, uint32_t out_h,
                               int32_t* const out[3], size_t out_stride, int32_t op, int32_t perm) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !avg || !res || !out || out_stride < out_w || op < 0 || op > 6 || perm < 0 || perm > 5)
    return JXLH_ERR_INVALID_ARGUMENT;
  if (out_w == 0 || out_h == 0) return JXLH_OK;
  const SqueezeExtents e = squeeze_extents(horizontal != 0, out_w, out_h);
  if (avg_stride < e.avg_w || (e.has_res && res_stride < e.res_w)) return JXLH_ERR_INVALID_ARGUMENT;
  const int32_t* rv[3];
  for (int i = 0; i < 3; i++) {
    if (!avg[i] || !out[i] || !is_device_ptr(avg[i]) || !is_device_ptr(out[i])) return JXLH_ERR_INVALID_ARGUMENT;
    if (e.has_res && (!res[i] || !is_device_ptr(res[i]))) return JXLH_ERR_INVALID_ARGUMENT;
    rv[i] = res[i] ? res[i] : avg[i];
  }
  // fused, or (planes of 2^31 samples or more) the two separate passes
  SqueezeLaunch L[2];
  const SqueezeStep st = step_of(horizontal, 3, avg, avg_stride, rv, res_stride, out_w, out_h, out, out_stride);
  const int n = plan_squeeze_step_rct(st, env_is("JXLH_SEPARATE_RCT", '1'), L);
  std::optional<ScopedKernelTimer> t;  // (the fused launch only, as ever)
  if (n == 1) t.emplace(ctx, horizontal ? "k6_unsqueeze_rct_h" : "k6_unsqueeze_rct_v");
  for (int k = 0; k < n; k++) issue_step(ctx->stream, L[k], st, op, perm);
  HIPCHK(ctx, hipGetLastError());
  return JXLH_OK;
}

jxlh_status jxlh_smooth_unsqueeze(jxlh_ctx* ctx, int32_t kind, const int32_t* avg, size_t avg_stride, uint32_t avg_w,
                                  uint32_t avg_h, uint32_t x0, uint32_t y0, int32_t* out, size_t out_stride,
                                  uint32_t out_w, uint32_t out_h) {
  JXLH_ON_DEVICE(ctx);
  // the float -> int conversion of the reference's build target rides in the kind argument
  const bool cvt_rne = kind >= 0 && (kind & JXLH_SMOOTH_CVT_NEAREST_EVEN) != 0;
  if (kind >= 0) kind &= ~JXLH_SMOOTH_CVT_NEAREST_EVEN;
  if (!ctx || !avg || !out || kind < JXLH_SMOOTH_H || kind > JXLH_SMOOTH_2D || avg_w == 0 || avg_h == 0 ||
      avg_stride < avg_w || out_stride < out_w || avg_w > (1u << 30) || avg_h > (1u << 30) || x0 > (1u << 30) ||
      y0 > (1u << 30) || out_w > (1u << 30) || out_h > (1u << 30))
    return JXLH_ERR_INVALID_ARGUMENT;
  const bool fx = kind != JXLH_SMOOTH_V, fy = kind != JXLH_SMOOTH_H;
  if ((fx ? out_w / 2 : out_w) == 0 || (fy ? out_h / 2 : out_h) == 0) return JXLH_OK; /* squeeze.rs:921-923 */
  static const char* const kNames[3] = {"k6_smooth_unsqueeze_h", "k6_smooth_unsqueeze_v", "k6_smooth_unsqueeze_2d"};
  if (is_device_ptr(avg) && is_device_ptr(out)) {
    ScopedKernelTimer t(ctx, kNames[kind]);
    launch_smooth_unsqueeze(ctx->stream, kind, avg, avg_stride, (int)avg_w, (int)avg_h, (int)x0, (int)y0, out,
                            out_stride, (int)out_w, (int)out_h, cvt_rne);
    HIPCHK(ctx, hipGetLastError());
    return JXLH_OK;
  }
  jxlh_status st;
  if ((st = stage_in(ctx, ctx->hook_i[0], avg, avg_stride * avg_h))) return st;
  if ((st = ensure(ctx, ctx->hook_i[2], out_stride * out_h))) return st;
  launch_smooth_unsqueeze(ctx->stream, kind, ctx->hook_i[0].p, avg_stride, (int)avg_w, (int)avg_h, (int)x0, (int)y0,
                          ctx->hook_i[2].p, out_stride, (int)out_w, (int)out_h, cvt_rne);
  HIPCHK(ctx, hipGetLastError());
  /* every sample of the rectangle is written; the stride padding of a host `out` is overwritten with whatever the
   * staging buffer held only if out_stride > out_w -- copy row by row instead */
  if (out_stride == out_w) return stage_out(ctx, out, (const int32_t*)ctx->hook_i[2].p, out_stride * out_h);
  HIPCHK(ctx, hipMemcpy2DAsync(out, out_stride * sizeof(int32_t), ctx->hook_i[2].p, out_stride * sizeof(int32_t),
                               out_w * sizeof(int32_t), out_h, hipMemcpyDeviceToHost, ctx->stream));
  JXLH_SYNC(ctx);
  return JXLH_OK;
}

jxlh_status jxlh_unsqueeze_planes(jxlh_ctx* ctx, int32_t horizontal, int32_t n_planes, const int32_t* const avg[],
                                  size_t avg_stride, const int32_t* const res[], size_t res_stride, uint32_t out_w,
                                  uint32_t out_h, int32_t* const out[], size_t out_stride) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !avg || !res || !out || n_planes < 1 || n_planes > 3 || out_stride < out_w)
    return JXLH_ERR_INVALID_ARGUMENT;
  if (out_w == 0 || out_h == 0) return JXLH_OK;
  if (out_w > kMaxModularDim || out_h > kMaxModularDim) return JXLH_ERR_UNSUPPORTED;
  const SqueezeExtents e = squeeze_extents(horizontal != 0, out_w, out_h);
  if (avg_stride < e.avg_w || (e.has_res && res_stride < e.res_w)) return JXLH_ERR_INVALID_ARGUMENT;
  const int32_t* rv[3];
  for (int i = 0; i < n_planes; i++) {
    if (!avg[i] || !out[i] || !is_device_ptr(avg[i]) || !is_device_ptr(out[i])) return JXLH_ERR_INVALID_ARGUMENT;
    rv[i] = res[i] ? res[i] : avg[i];
    if (e.has_res && (!res[i] || !is_device_ptr(res[i]))) return JXLH_ERR_INVALID_ARGUMENT;
  }
  ScopedKernelTimer t(ctx, horizontal ? "k6_unsqueeze_h" : "k6_unsqueeze_v");
  const SqueezeStep st = step_of(horizontal, n_planes, avg, avg_stride, rv, res_stride, out_w, out_h, out, out_stride);
  launch_unsqueeze(ctx->stream, plan_squeeze_step(st), st);
  HIPCHK(ctx, hipGetLastError());
  return JXLH_OK;
}

}  // extern "C"
