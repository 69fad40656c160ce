// C ABI, Modular transforms: RCT, Palette (plain, delta / predicted, Weighted), Squeeze (steps, fused chains,
// progressive smooth steps) and the bridges from Modular channels to pixels.
#include <algorithm>
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
// what the two chain calls plan from, once the arguments are checked and the arena is there
SqueezeChainIn chain_in(jxlh_ctx* ctx, int n_planes, int n_levels, const jxlh_squeeze_level* levels, const int32_t* const base[],
                        size_t base_stride, uint32_t base_w, uint32_t base_h, int32_t* const out[], size_t out_stride, bool with_rct) {
  SqueezeChainIn in{n_planes, n_levels, levels, base_w, base_h, base_stride, out_stride, {}, {}, (uintptr_t)ctx->hook_i[0].p,
                    with_rct, env_is("JXLH_SEPARATE_RCT", '1'), !env_is("JXLH_CHAIN_FLOW", '0')};
  for (int p = 0; p < n_planes; p++) {
    in.base[p] = (uintptr_t)base[p];
    in.out[p] = (uintptr_t)out[p];
  }
  return in;
}
}  // namespace

extern "C" {

// ---------------------------------------------------------------- Modular
// In-place / out-of-place on the caller's buffers when they are device pointers; host
// pointers are staged through context scratch.
jxlh_status jxlh_rct(jxlh_ctx* ctx, int32_t* p0, int32_t* p1, int32_t* p2, size_t n, int32_t op, int32_t perm) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !p0 || !p1 || !p2 || op < 0 || op > 6 || perm < 0 || perm > 5) return JXLH_ERR_INVALID_ARGUMENT;
  if (n == 0) return JXLH_OK;
  if (is_device_ptr(p0) && is_device_ptr(p1) && is_device_ptr(p2)) {
    ScopedKernelTimer t(ctx, "k4_rct");
    launch_rct(ctx->stream, p0, p1, p2, n, op, perm);
    HIPCHK(ctx, hipGetLastError());
    return JXLH_OK;
  }
  jxlh_status st;
  int32_t* h[3] = {p0, p1, p2};
  for (int c = 0; c < 3; c++)
    if ((st = stage_in(ctx, ctx->hook_i[c], (const int32_t*)h[c], n))) return st;
  launch_rct(ctx->stream, ctx->hook_i[0].p, ctx->hook_i[1].p, ctx->hook_i[2].p, n, op, perm);
  HIPCHK(ctx, hipGetLastError());
  for (int c = 0; c < 3; c++)
    if ((st = stage_out(ctx, h[c], (const int32_t*)ctx->hook_i[c].p, n))) return st;
  return JXLH_OK;
}

jxlh_status jxlh_palette(jxlh_ctx* ctx, const int32_t* index, size_t n, const int32_t* palette, int32_t num_colors,
                         size_t palette_stride, int32_t nb_channels, int32_t bit_depth, int32_t* out) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !index || !palette || !out || num_colors < 0 || nb_channels < 1 || nb_channels > 64 || bit_depth < 1 ||
      bit_depth > 24 || palette_stride < (size_t)num_colors)
    return JXLH_ERR_INVALID_ARGUMENT;
  if (n == 0) return JXLH_OK;
  const size_t pal_n = palette_stride * (size_t)nb_channels;
  if (is_device_ptr(index) && is_device_ptr(palette) && is_device_ptr(out)) {
    ScopedKernelTimer t(ctx, "k5_palette");
    launch_palette(ctx->stream, index, n, palette, num_colors, palette_stride, nb_channels, bit_depth, out);
    HIPCHK(ctx, hipGetLastError());
    return JXLH_OK;
  }
  jxlh_status st;
  if ((st = stage_in(ctx, ctx->hook_i[0], index, n))) return st;
  if ((st = stage_in(ctx, ctx->hook_i[1], palette, pal_n ? pal_n : 1))) return st;
  if ((st = ensure(ctx, ctx->hook_i[2], n * nb_channels))) return st;
  launch_palette(ctx->stream, ctx->hook_i[0].p, n, ctx->hook_i[1].p, num_colors, palette_stride, nb_channels,
                 bit_depth, ctx->hook_i[2].p);
  HIPCHK(ctx, hipGetLastError());
  return stage_out(ctx, out, (const int32_t*)ctx->hook_i[2].p, n * nb_channels);
}

jxlh_status jxlh_palette_strided(jxlh_ctx* ctx, const int32_t* index, size_t n, const int32_t* palette,
                                 int32_t num_colors, size_t palette_stride, int32_t nb_channels, int32_t bit_depth,
                                 int32_t* out, size_t out_channel_stride) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !index || !palette || !out || num_colors < 0 || nb_channels < 1 || nb_channels > 64 || bit_depth < 1 ||
      bit_depth > 24 || palette_stride < (size_t)num_colors || out_channel_stride < n)
    return JXLH_ERR_INVALID_ARGUMENT;
  if (!is_device_ptr(index) || !is_device_ptr(palette) || !is_device_ptr(out)) return JXLH_ERR_INVALID_ARGUMENT;
  if (n == 0) return JXLH_OK;
  ScopedKernelTimer t(ctx, "k5_palette");
  launch_palette(ctx->stream, index, n, palette, num_colors, palette_stride, nb_channels, bit_depth, out,
                 out_channel_stride);
  HIPCHK(ctx, hipGetLastError());
  return JXLH_OK;
}

jxlh_status jxlh_palette_delta(jxlh_ctx* ctx, const int32_t* index, uint32_t w, uint32_t h, const int32_t* palette,
                               int32_t num_colors, int32_t num_deltas, size_t palette_stride, int32_t nb_channels,
                               int32_t bit_depth, int32_t predictor, int32_t* out) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !index || !palette || !out || num_colors < 0 || num_deltas < 0 || nb_channels < 1 || nb_channels > 64 ||
      bit_depth < 1 || bit_depth > 24 || palette_stride < (size_t)num_colors + (size_t)num_deltas || predictor < 0 ||
      predictor > 13 || w > (1u << 20) || h > (1u << 20))
    return JXLH_ERR_INVALID_ARGUMENT;
  if (predictor == 6) return JXLH_ERR_UNSUPPORTED;  // Weighted: its own stateful branch (palette.rs:200-227), host
  if (w == 0 || h == 0) return JXLH_OK;
  const size_t n = (size_t)w * h, pal_n = palette_stride * (size_t)nb_channels;
  if (n * (size_t)nb_channels >= (1ull << 31)) return JXLH_ERR_UNSUPPORTED;
  if (jxlh_status st0 = ensure(ctx, ctx->hook_i[3], (size_t)nb_channels * palette_delta_bands((int)h))) return st0;
  int* progress = reinterpret_cast<int*>(ctx->hook_i[3].p);
  if (is_device_ptr(index) && is_device_ptr(palette) && is_device_ptr(out)) {
    ScopedKernelTimer t(ctx, "k5_palette_delta");
    launch_palette_delta(ctx->stream, index, (int)w, (int)h, palette, num_colors, num_deltas, palette_stride,
                         nb_channels, bit_depth, predictor, out, progress);
    HIPCHK(ctx, hipGetLastError());
    return JXLH_OK;
  }
  jxlh_status st;
  if ((st = stage_in(ctx, ctx->hook_i[0], index, n))) return st;
  if ((st = stage_in(ctx, ctx->hook_i[1], palette, pal_n ? pal_n : 1))) return st;
  if ((st = ensure(ctx, ctx->hook_i[2], n * nb_channels))) return st;
  launch_palette_delta(ctx->stream, ctx->hook_i[0].p, (int)w, (int)h, ctx->hook_i[1].p, num_colors, num_deltas,
                       palette_stride, nb_channels, bit_depth, predictor, ctx->hook_i[2].p, progress);
  HIPCHK(ctx, hipGetLastError());
  return stage_out(ctx, out, (const int32_t*)ctx->hook_i[2].p, n * nb_channels);
}

// ---- Modular channels -> pipeline samples (render/stages/convert.rs)
jxlh_status jxlh_modular_to_rgb8(jxlh_ctx* ctx, const int32_t* const planes[3], size_t stride, uint32_t w, uint32_t h,
                                 int32_t multiplier, int32_t max, uint32_t channels, void* out, size_t bytes_per_row) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !planes || !planes[0] || !planes[1] || !planes[2] || !out || stride < w || (channels != 3 && channels != 4) ||
      bytes_per_row < (size_t)w * channels || max < 0 || max > 255 || w > (1u << 20) || h > (1u << 20))
    return JXLH_ERR_INVALID_ARGUMENT;
  if (w == 0 || h == 0) return JXLH_OK;
  const bool dev_in = is_device_ptr(planes[0]) && is_device_ptr(planes[1]) && is_device_ptr(planes[2]);
  const int32_t* src[3] = {planes[0], planes[1], planes[2]};
  size_t sstride = stride;
  jxlh_status st;
  if (!dev_in) {
    const size_t n = (size_t)stride * h;
    for (int c = 0; c < 3; c++) {
      if ((st = stage_in(ctx, ctx->hook_i[c], planes[c], n))) return st;
      src[c] = ctx->hook_i[c].p;
    }
  }
  ScopedKernelTimer t(ctx, "k_i32_to_rgb8");
  if (is_device_ptr(out)) {
    launch_i32_to_rgb8(ctx->stream, src, sstride, (int)w, (int)h, multiplier, max, (int)channels,
                       static_cast<uint8_t*>(out), bytes_per_row);
    HIPCHK(ctx, hipGetLastError());
    return JXLH_OK;
  }
  const size_t tight = (size_t)w * channels;
  if ((st = ensure(ctx, ctx->rgb8, tight * (size_t)h))) return st;
  launch_i32_to_rgb8(ctx->stream, src, sstride, (int)w, (int)h, multiplier, max, (int)channels, ctx->rgb8.p, tight);
  HIPCHK(ctx, hipGetLastError());
  if ((st = copy2d(ctx, out, bytes_per_row, ctx->rgb8.p, tight, tight, (size_t)h, ctx->stream))) return st;
  JXLH_SYNC(ctx);
  return JXLH_OK;
}

jxlh_status jxlh_modular_to_f32(jxlh_ctx* ctx, const int32_t* in, size_t n, uint32_t bits_per_sample, float* out) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !in || !out || !bit_depth_ok(bits_per_sample, 32)) return JXLH_ERR_INVALID_ARGUMENT;
  if (n == 0) return JXLH_OK;
  const uint32_t bits = bits_per_sample & 0xffu, exp_bits = bits_per_sample >> 8;  // BitDepth::floating_point_sample()
  const float scale = 1.0f / (float)((1ull << bits) - 1);  // convert.rs:528
  auto convert = [&](const int32_t* src, float* dst) {
    if (exp_bits) launch_float_samples_to_f32(ctx->stream, src, n, bits, exp_bits, dst);  // convert.rs:525-526
    else launch_modular_to_f32(ctx->stream, src, n, scale, dst);
  };
  if (is_device_ptr(in) && is_device_ptr(out)) {
    convert(in, out);
    HIPCHK(ctx, hipGetLastError());
    return JXLH_OK;
  }
  jxlh_status st;
  if ((st = stage_in(ctx, ctx->hook_i[0], in, n))) return st;
  if ((st = ensure(ctx, ctx->hook_f[0], n))) return st;
  convert(ctx->hook_i[0].p, ctx->hook_f[0].p);
  HIPCHK(ctx, hipGetLastError());
  return stage_out(ctx, out, (const float*)ctx->hook_f[0].p, n);
}

jxlh_status jxlh_modular_xyb_to_f32(jxlh_ctx* ctx, const int32_t* y, const int32_t* x, const int32_t* b, size_t n,
                                    const float quant_factors[3], float* ox, float* oy, float* ob) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !y || !x || !b || !quant_factors || !ox || !oy || !ob) return JXLH_ERR_INVALID_ARGUMENT;
  if (n == 0) return JXLH_OK;
  const int32_t* in[3] = {y, x, b};
  float* outp[3] = {ox, oy, ob};
  if (is_device_ptr(y) && is_device_ptr(x) && is_device_ptr(b) && is_device_ptr(ox) && is_device_ptr(oy) && is_device_ptr(ob)) {
    launch_modular_xyb_to_f32(ctx->stream, y, x, b, n, quant_factors, ox, oy, ob);
    HIPCHK(ctx, hipGetLastError());
    return JXLH_OK;
  }
  jxlh_status st;
  for (int c = 0; c < 3; c++) {
    if ((st = stage_in(ctx, ctx->hook_i[c], in[c], n))) return st;
    if ((st = ensure(ctx, ctx->hook_f[c], n))) return st;
  }
  launch_modular_xyb_to_f32(ctx->stream, ctx->hook_i[0].p, ctx->hook_i[1].p, ctx->hook_i[2].p, n, quant_factors,
                            ctx->hook_f[0].p, ctx->hook_f[1].p, ctx->hook_f[2].p);
  HIPCHK(ctx, hipGetLastError());
  for (int c = 0; c < 3; c++)
    if ((st = stage_out(ctx, outp[c], (const float*)ctx->hook_f[c].p, n))) return st;
  return JXLH_OK;
}

jxlh_status jxlh_palette_delta_wp(jxlh_ctx* ctx, const int32_t* index, uint32_t w, uint32_t h, const int32_t* palette,
                                  int32_t num_colors, int32_t num_deltas, size_t palette_stride, int32_t nb_channels,
                                  int32_t bit_depth, const jxlh_wp_header* wp, int32_t* out) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !index || !palette || !out || !wp || num_colors < 0 || num_deltas < 0 || nb_channels < 1 ||
      nb_channels > 64 || bit_depth < 1 || bit_depth > 24 ||
      palette_stride < (size_t)num_colors + (size_t)num_deltas || w > (1u << 20) || h > (1u << 20))
    return JXLH_ERR_INVALID_ARGUMENT;
  const uint32_t header[11] = {wp->p1c, wp->p2c, wp->p3ca, wp->p3cb, wp->p3cc, wp->p3cd, wp->p3ce,
                               wp->w0,  wp->w1,  wp->w2,   wp->w3};
  for (int i = 0; i < 11; i++)
    if (header[i] >= (i < 7 ? 32u : 16u)) return JXLH_ERR_INVALID_ARGUMENT;  // Bits(5) / Bits(4) fields
  if (w == 0 || h == 0) return JXLH_OK;
  const size_t n = (size_t)w * h, pal_n = palette_stride * (size_t)nb_channels;
  if (n * (size_t)nb_channels >= (1ull << 31)) return JXLH_ERR_UNSUPPORTED;
  const size_t nbands = (size_t)palette_delta_bands((int)h);
  // progress counters, then the band-edge rows of predictor state (5 rows of w per channel and band)
  const size_t n_prog = (size_t)nb_channels * nbands, n_rows = n_prog * 5 * (size_t)w;
  if (jxlh_status st0 = ensure(ctx, ctx->hook_i[3], n_prog + n_rows)) return st0;
  int* progress = reinterpret_cast<int*>(ctx->hook_i[3].p);
  int32_t* wp_rows = ctx->hook_i[3].p + n_prog;
  if (is_device_ptr(index) && is_device_ptr(palette) && is_device_ptr(out)) {
    ScopedKernelTimer t(ctx, "k5_palette_wp");
    launch_palette_wp(ctx->stream, index, (int)w, (int)h, palette, num_colors, num_deltas, palette_stride, nb_channels,
                      bit_depth, header, out, progress, wp_rows);
    HIPCHK(ctx, hipGetLastError());
    return JXLH_OK;
  }
  jxlh_status st;
  if ((st = stage_in(ctx, ctx->hook_i[0], index, n))) return st;
  if ((st = stage_in(ctx, ctx->hook_i[1], palette, pal_n ? pal_n : 1))) return st;
  if ((st = ensure(ctx, ctx->hook_i[2], n * nb_channels))) return st;
  launch_palette_wp(ctx->stream, ctx->hook_i[0].p, (int)w, (int)h, ctx->hook_i[1].p, num_colors, num_deltas,
                    palette_stride, nb_channels, bit_depth, header, ctx->hook_i[2].p, progress, wp_rows);
  HIPCHK(ctx, hipGetLastError());
  return stage_out(ctx, out, (const int32_t*)ctx->hook_i[2].p, n * nb_channels);
}

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
  const bool with_rct = rct_op >= 0;
  if (!ctx || (with_rct && (n_planes != 3 || rct_op > 6 || rct_perm < 0 || rct_perm > 5))) return JXLH_ERR_INVALID_ARGUMENT;
  jxlh_status st;
  if ((st = check_squeeze_chain(n_planes, n_levels, levels, base, base_stride, base_w, base_h, out, out_stride, is_device_ptr)))
    return st;
  if ((st = ensure(ctx, ctx->hook_i[0], std::max<size_t>(squeeze_arena(n_planes, n_levels, levels).total, 1)))) return st;
  const SqueezeChainIn in = chain_in(ctx, n_planes, n_levels, levels, base, base_stride, base_w, base_h, out, out_stride, with_rct);
  return issue_chain(ctx, in, plan_squeeze_chain(in), rct_op, rct_perm);
}

jxlh_status jxlh_squeeze_preview_kinds(int32_t n_planes, int32_t n_levels, const jxlh_squeeze_level* levels, uint32_t base_w,
                                       uint32_t base_h, uint8_t* kinds, uint8_t* live) {
  if (!kinds) return JXLH_ERR_INVALID_ARGUMENT;
  // the chain's geometry and NULL rules; no planes are named here, so every pointer passes for a device one
  static const int32_t some = 0;
  const int32_t* const base[3] = {&some, &some, &some};
  int32_t* const out[3] = {const_cast<int32_t*>(&some), const_cast<int32_t*>(&some), const_cast<int32_t*>(&some)};
  if (jxlh_status st = check_squeeze_chain(n_planes, n_levels, levels, base, base_w, base_w, base_h, out, (size_t)kMaxModularDim,
                                           [](const void*) { return true; }, true))
    return st;
  squeeze_preview_kinds(n_planes, n_levels, levels, kinds, live);
  return JXLH_OK;
}

// A progressive preview of a whole squeeze transform: validate, plan (squeeze_preview_plan.h), issue -- the regular
// prefix as the chain it is, then one launch group per live level, in stream order.
jxlh_status jxlh_unsqueeze_chain_preview(jxlh_ctx* ctx, int32_t n_planes, int32_t n_levels, const jxlh_squeeze_level* levels,
                                         const int32_t* const base[], size_t base_stride, uint32_t base_w, uint32_t base_h,
                                         int32_t* const out[], size_t out_stride, int32_t rct_op, int32_t rct_perm, uint32_t flags) {
  JXLH_ON_DEVICE(ctx);
  const bool with_rct = rct_op >= 0;
  if (!ctx || (with_rct && (n_planes != 3 || rct_op > 6 || rct_perm < 0 || rct_perm > 5)) ||
      (flags != 0 && flags != JXLH_SMOOTH_CVT_NEAREST_EVEN))
    return JXLH_ERR_INVALID_ARGUMENT;
  jxlh_status st;
  if ((st = check_squeeze_chain(n_planes, n_levels, levels, base, base_stride, base_w, base_h, out, out_stride, is_device_ptr, true)))
    return st;
  if ((st = ensure(ctx, ctx->hook_i[0], std::max<size_t>(squeeze_arena(n_planes, n_levels, levels).total, 1)))) return st;
  const SqueezeChainIn in = chain_in(ctx, n_planes, n_levels, levels, base, base_stride, base_w, base_h, out, out_stride, with_rct);
  const SqueezePreviewPlan plan = plan_squeeze_preview(in);
  if (plan.n_prefix > 0 && (st = issue_chain(ctx, plan.prefix_in, plan.prefix, rct_op, rct_perm))) return st;
  if (plan.n == 0) return JXLH_OK;
  ScopedKernelTimer t(ctx, "k6_unsqueeze_chain_preview");
  for (int k = 0; k < plan.n; k++) {
    const PreviewEntry& e = plan.entry[k];
    const jxlh_squeeze_level& lv = levels[e.level];
    if (e.kind == JXLH_PREVIEW_REGULAR) {
      const SqueezeStep step = squeeze_level_step(in, plan.arena, e.level, e.src, e.dst);
      for (int j = 0; j < e.n_launch; j++) issue_step(ctx->stream, e.launch[j], step, rct_op, rct_perm);
      continue;
    }
    const int32_t* src[3] = {};
    int32_t* dst[3] = {};
    for (int p = 0; p < n_planes; p++) {
      src[p] = (const int32_t*)squeeze_plane_addr(in, plan.arena, e.src, p);
      dst[p] = (int32_t*)squeeze_plane_addr(in, plan.arena, e.dst, p);
    }
    const int kind = e.kind == JXLH_PREVIEW_SMOOTH_2D ? JXLH_SMOOTH_2D : lv.horizontal ? JXLH_SMOOTH_H : JXLH_SMOOTH_V;
    launch_smooth_unsqueeze_planes(ctx->stream, kind, n_planes, src, e.src.stride, (int)e.src_w, (int)e.src_h, dst, e.dst.stride,
                                   (int)lv.out_w, (int)lv.out_h, flags != 0, e.rct ? rct_op : -1, rct_perm);
  }
  HIPCHK(ctx, hipGetLastError());
  return JXLH_OK;
}

jxlh_status jxlh_squeeze_tile_kinds(int32_t n_planes, int32_t n_levels, const jxlh_squeeze_level* levels,
                                    const jxlh_squeeze_tiles* tiles, uint32_t base_w, uint32_t base_h, int32_t level, uint8_t* kinds) {
  if (!kinds) return JXLH_ERR_INVALID_ARGUMENT;
  // as jxlh_squeeze_preview_kinds: no planes are named here, so every pointer passes for a device one
  static const int32_t some = 0;
  const int32_t* const base[3] = {&some, &some, &some};
  int32_t* const out[3] = {const_cast<int32_t*>(&some), const_cast<int32_t*>(&some), const_cast<int32_t*>(&some)};
  if (jxlh_status st = check_squeeze_chain(n_planes, n_levels, levels, base, base_w, base_w, base_h, out, (size_t)kMaxModularDim,
                                           [](const void*) { return true; }, true))
    return st;
  if (jxlh_status st = check_squeeze_tiles(n_levels, levels, tiles)) return st;
  if (level < 0 || level >= n_levels) return JXLH_ERR_INVALID_ARGUMENT;
  squeeze_tile_kinds(n_planes, levels, tiles, level, kinds);
  return JXLH_OK;
}

// A progressive preview per grid cell: validate, plan (squeeze_tiles_plan.h), issue.  With no mixed level the call is
// jxlh_unsqueeze_chain_preview; else the regular prefix as the chain it is, the work lists in one copy, then per needed
// level its whole-level launch or its two list launches, in stream order.
jxlh_status jxlh_unsqueeze_chain_preview_tiles(jxlh_ctx* ctx, int32_t n_planes, int32_t n_levels, const jxlh_squeeze_level* levels,
                                               const jxlh_squeeze_tiles* tiles, const int32_t* const base[], size_t base_stride,
                                               uint32_t base_w, uint32_t base_h, int32_t* const out[], size_t out_stride,
                                               int32_t rct_op, int32_t rct_perm, uint32_t flags) {
  JXLH_ON_DEVICE(ctx);
  const bool with_rct = rct_op >= 0;
  if (!ctx || (with_rct && (n_planes != 3 || rct_op > 6 || rct_perm < 0 || rct_perm > 5)) ||
      (flags != 0 && flags != JXLH_SMOOTH_CVT_NEAREST_EVEN))
    return JXLH_ERR_INVALID_ARGUMENT;
  jxlh_status st;
  if ((st = check_squeeze_chain(n_planes, n_levels, levels, base, base_stride, base_w, base_h, out, out_stride, is_device_ptr, true)))
    return st;
  if ((st = check_squeeze_tiles(n_levels, levels, tiles))) return st;
  if ((st = ensure(ctx, ctx->hook_i[0], std::max<size_t>(squeeze_arena(n_planes, n_levels, levels).total, 1)))) return st;
  const SqueezeChainIn in = chain_in(ctx, n_planes, n_levels, levels, base, base_stride, base_w, base_h, out, out_stride, with_rct);
  const SqueezeTilesPlan plan = plan_squeeze_tiles(in, tiles);
  if (!plan.mixed)
    return jxlh_unsqueeze_chain_preview(ctx, n_planes, n_levels, plan.folded.data(), base, base_stride, base_w, base_h, out, out_stride,
                                        rct_op, rct_perm, flags);
  if (plan.too_large) return JXLH_ERR_UNSUPPORTED;
  // the lists: one pinned block, one copy
  const size_t n_rec = plan.upload_records;
  if ((st = ensure(ctx, ctx->sq_tiles_dev, std::max<size_t>(n_rec, 1)))) return st;
  Pinned<int4>& host = ctx->sq_tiles_host[ctx->sq_tiles_next];
  Fence& copied = ctx->sq_tiles_copied[ctx->sq_tiles_next];
  ctx->sq_tiles_next = (ctx->sq_tiles_next + 1) % jxlh_ctx::kSqTilesRing;
  HIPCHK(ctx, copied.sync());  // the block's previous lists are on the device
  copied.clear();
  if (host.n < n_rec) {
    HIPCHK(ctx, host.reset());
    HIPCHK(ctx, host.alloc(n_rec + n_rec / 2));
  }
  static_assert(sizeof(SqTileSmoothCell) == sizeof(int4) && sizeof(SqTileRun) == sizeof(int4), "the lists are 16-byte records");
  for (const SqTilesEntry& e : plan.entry) {
    if (!e.smooth.empty()) std::memcpy(host.p + e.smooth_off, e.smooth.data(), e.smooth.size() * sizeof(int4));
    if (!e.runs.empty()) std::memcpy(host.p + e.runs_off, e.runs.data(), e.runs.size() * sizeof(int4));
  }
  if (n_rec) {
    HIPCHK(ctx, hipMemcpyAsync(ctx->sq_tiles_dev.p, host.p, n_rec * sizeof(int4), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, copied.record(ctx->stream));
  }
  if (plan.n_prefix > 0 && (st = issue_chain(ctx, plan.prefix_in, plan.prefix, rct_op, rct_perm))) return st;
  // one timer per launch: whole levels under the preview call's name, the list launches under their kernels'
  for (const SqTilesEntry& e : plan.entry) {
    const jxlh_squeeze_level& lv = levels[e.level];
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
    if (!e.smooth.empty()) {
      ScopedKernelTimer t(ctx, "k6_smooth_unsqueeze_cells");
      launch_smooth_unsqueeze_cells(ctx->stream, e.horizontal, n_planes, src, e.src.stride, (int)e.src_w, (int)e.src_h, src2, e.src2.stride,
                                    (int)e.src2_w, (int)e.src2_h, dst, e.dst.stride,
                                    reinterpret_cast<const SqTileSmoothCell*>(ctx->sq_tiles_dev.p + e.smooth_off), (uint32_t)e.smooth.size(),
                                    e.tiles_x, e.tiles_per_cell, flags != 0);
    }
    if (!e.runs.empty()) {
      ScopedKernelTimer t(ctx, "k6_unsqueeze_runs");
      launch_unsqueeze_runs(ctx->stream, step, reinterpret_cast<const SqTileRun*>(ctx->sq_tiles_dev.p + e.runs_off), (uint32_t)e.runs.size(),
                            e.groups_per_run);
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
