// C ABI, Modular transforms: RCT, Palette (plain, delta / predicted, Weighted) and the bridges from Modular channels to
// pixels.  (Squeeze: abi_squeeze.hip.)
#include "jxlh_ctx.h"

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

}  // extern "C"
