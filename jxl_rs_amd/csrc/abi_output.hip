// C ABI, reading a finished frame: f32 planes, the LF image, and the output stages after EPF (XYB / YCbCr -> RGB,
// every transfer function, 8 / 16 bit interleaved), SURVEY.md 8(f) item 2.
#include <algorithm>

#include "jxlh_ctx.h"

extern "C" {

namespace {
SubPlanesDev sub_planes_dev(const jxlh_ctx* ctx) {
  const FrameDev& f = ctx->fd;
  SubPlanesDev sp;
  for (int c = 0; c < 3; c++) {
    const int hs = f.hshift[c], vs = f.vshift[c];
    sp.p[c] = (hs | vs) ? f.tmp[c] : f.planes[c];
    sp.hs[c] = hs;
    sp.vs[c] = vs;
    sp.cw[c] = (f.xsize + (1 << hs) - 1) >> hs;
    sp.ch[c] = (f.ysize + (1 << vs) - 1) >> vs;
  }
  return sp;
}

// Rows [y0, y1) of the result behind the colour stage `d` names, as interleaved 8- / 16-bit samples with an opaque fourth
// one.  16 bit is the identity save (channels 0 1 2, orientation 1, native byte order) of k_save.hip; 8 bit, and a YCbCr
// frame whose chroma is still sub-sampled, have the kernels of k_output.hip.  `out` is row y0.  Unlike jxlh_frame_save
// this serves sharded contexts (a rank converts its band: convert_band_to_output) and results of any size.
jxlh_status read_output(jxlh_ctx* ctx, const jxlh_output_desc* d, uint32_t y0, uint32_t y1, void* out,
                        size_t bytes_per_row, bool wait) {
  if (!ctx || !d || (d->bits != 8 && d->bits != 16)) return JXLH_ERR_INVALID_ARGUMENT;
  SaveLaunch a{};
  if (jxlh_status st = colour_stage(d, &a.mode, &a.xyb, &a.tf)) return st;
  const uint32_t channels = d->channels;
  if (!out || (channels != 3 && channels != 4)) return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->in_frame || !ctx->frame.result[0]) return JXLH_ERR_BAD_STATE;
  if (blended(ctx) && a.mode != kModeNone) return JXLH_ERR_BAD_STATE;  // jxlh_frame_blend has run the colour stage already
  if (y1 > (uint32_t)ctx->res_h) y1 = (uint32_t)ctx->res_h;
  const size_t bps = d->bits / 8, pb = channels * bps;
  if (y0 >= y1 || bytes_per_row < (size_t)ctx->res_w * pb || bytes_per_row % bps != 0 ||
      reinterpret_cast<uintptr_t>(out) % bps != 0)
    return JXLH_ERR_INVALID_ARGUMENT;
  // the labels are the read-outs' names in jxlh_kernel_timing_get (tools and recorded profiles key on them), not kernels
  const OutRect r = {0, y0, (size_t)ctx->res_w, y1 - y0};
  if (ctx->frame.chroma_lazy && a.mode == kModeYcbcr) {
    const SubPlanesDev sp = sub_planes_dev(ctx);
    return write_out(ctx, out, bytes_per_row, pb, r, "k_ycbcr_sub_to_rgb", wait, [&](uint8_t* origin, size_t pitch) {
      launch_ycbcr_sub_to_rgb(ctx->stream, sp, ctx->res_stride, ctx->res_w, (int)y0, (int)(y1 - y0), (int)channels,
                              (int)d->bits, origin, pitch);
    });
  }
  if (d->bits == 8) {  // a kernel of its own: measured faster than the save's identity case at this depth
    materialise_chroma(ctx);
    const float* planes[3] = {ctx->frame.result[0], ctx->frame.result[1], ctx->frame.result[2]};
    return write_out(ctx, out, bytes_per_row, pb, r, "k_xyb_to_rgb8", wait, [&](uint8_t* origin, size_t pitch) {
      launch_xyb_to_rgb8(ctx->stream, planes, ctx->res_stride, ctx->res_w, (int)y0, (int)(y1 - y0), a.mode, a.xyb, a.tf,
                         (int)channels, origin, pitch);
    });
  }
  // 16 bit: the identity save
  jxlh_save_desc save = {};
  save.n_channels = 3;
  for (uint32_t k = 0; k < 3; k++) save.channels[k] = k;
  save.fill_opaque_alpha = channels == 4;
  save.format = JXLH_SAVE_U16;
  save.bit_depth = 16;
  save.orientation = 1;
  void* image = reinterpret_cast<void*>(reinterpret_cast<uintptr_t>(out) - (size_t)y0 * bytes_per_row);
  return save_result_rows(ctx, a, &save, nullptr, nullptr, y0, y1, image, bytes_per_row, "k_xyb_to_rgb16", wait);
}

// the dedicated entry points are read_output with a descriptor of their own: XYB + sRGB (p) or YCbCr (no p)
jxlh_status read_fixed(jxlh_ctx* ctx, const jxlh_xyb_params* p, uint32_t bits, uint32_t channels, uint32_t y0, uint32_t y1,
                       void* out, size_t bytes_per_row, bool wait = true) {
  jxlh_output_desc d = {};
  d.color = p ? JXLH_COLOR_XYB : JXLH_COLOR_YCBCR;
  d.transfer = JXLH_TF_SRGB;
  if (p) d.xyb = *p;
  d.bits = bits;
  d.channels = channels;
  return read_output(ctx, &d, y0, y1, out, bytes_per_row, wait);
}
}  // namespace

jxlh_status jxlh_frame_read_rgb8(jxlh_ctx* ctx, const jxlh_xyb_params* p, uint32_t channels, uint32_t y0,
                                 uint32_t y1, void* out, size_t bytes_per_row) {
  JXLH_ON_DEVICE(ctx);
  if (!p) return JXLH_ERR_INVALID_ARGUMENT;
  return read_fixed(ctx, p, 8, channels, y0, y1, out, bytes_per_row);
}
jxlh_status jxlh_frame_read_rgb8_async(jxlh_ctx* ctx, const jxlh_xyb_params* p, uint32_t channels, uint32_t y0,
                                       uint32_t y1, void* out, size_t bytes_per_row) {
  JXLH_ON_DEVICE(ctx);
  if (!p) return JXLH_ERR_INVALID_ARGUMENT;
  return read_fixed(ctx, p, 8, channels, y0, y1, out, bytes_per_row, /*wait=*/false);
}
jxlh_status jxlh_frame_read_rgb16(jxlh_ctx* ctx, const jxlh_xyb_params* p, uint32_t channels, uint32_t y0,
                                  uint32_t y1, void* out, size_t bytes_per_row) {
  JXLH_ON_DEVICE(ctx);
  if (!p) return JXLH_ERR_INVALID_ARGUMENT;
  return read_fixed(ctx, p, 16, channels, y0, y1, out, bytes_per_row);
}
jxlh_status jxlh_frame_read_ycbcr_rgb8(jxlh_ctx* ctx, uint32_t channels, uint32_t y0, uint32_t y1, void* out,
                                       size_t bytes_per_row) {
  JXLH_ON_DEVICE(ctx);
  return read_fixed(ctx, nullptr, 8, channels, y0, y1, out, bytes_per_row);
}
jxlh_status jxlh_frame_read_ycbcr_rgb16(jxlh_ctx* ctx, uint32_t channels, uint32_t y0, uint32_t y1, void* out,
                                        size_t bytes_per_row) {
  JXLH_ON_DEVICE(ctx);
  return read_fixed(ctx, nullptr, 16, channels, y0, y1, out, bytes_per_row);
}

}  // extern "C"
// comm.hip: a rank's band of the converted image into its rows of `out` (device memory), queued on the context's stream
jxlh_status jxlh_host::convert_band_to_output(jxlh_ctx* ctx, const jxlh_output_desc* d, uint32_t y0, uint32_t y1, void* out,
                                   size_t bytes_per_row) {
  if (y0 >= y1) return JXLH_OK;
  if (!is_device_ptr(out)) return JXLH_ERR_INVALID_ARGUMENT;
  return read_output(ctx, d, y0, y1, static_cast<char*>(out) + (size_t)y0 * bytes_per_row, bytes_per_row, /*wait=*/false);
}

extern "C" {
jxlh_status jxlh_frame_read_output(jxlh_ctx* ctx, const jxlh_output_desc* d, uint32_t y0, uint32_t y1, void* out,
                                   size_t bytes_per_row) {
  JXLH_ON_DEVICE(ctx);
  return read_output(ctx, d, y0, y1, out, bytes_per_row, /*wait=*/true);
}
jxlh_status jxlh_frame_read_output_async(jxlh_ctx* ctx, const jxlh_output_desc* d, uint32_t y0, uint32_t y1, void* out,
                                         size_t bytes_per_row) {
  JXLH_ON_DEVICE(ctx);
  return read_output(ctx, d, y0, y1, out, bytes_per_row, /*wait=*/false);
}

jxlh_status jxlh_frame_read_planes(jxlh_ctx* ctx, const jxlh_plane out[3]) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !out) return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->in_frame || !ctx->frame.result[0]) return JXLH_ERR_BAD_STATE;
  materialise_chroma(ctx);
  for (int c = 0; c < 3; c++) {
    if (!out[c].ptr || out[c].bytes_per_row < (size_t)ctx->res_w * sizeof(float) || out[c].num_rows < (size_t)ctx->res_h ||
        out[c].bytes_between_rows < out[c].bytes_per_row)
      return JXLH_ERR_INVALID_ARGUMENT;
    jxlh_status st = copy2d(ctx, out[c].ptr, out[c].bytes_between_rows, ctx->frame.result[c],
                            ctx->res_stride * sizeof(float), (size_t)ctx->res_w * sizeof(float), ctx->res_h, ctx->stream);
    if (st != JXLH_OK) return st;
  }
  return jxlh_ctx_sync(ctx);
}

namespace {
// the rect [x0, x0 + w) x [y0, y0 + h) of the finished planes, cut at the result's right / bottom edge
jxlh_status read_planes_rect(jxlh_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const jxlh_plane out[3],
                             bool wait) {
  if (!ctx || !out || w == 0 || h == 0) return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->in_frame || !ctx->frame.result[0]) return JXLH_ERR_BAD_STATE;
  if (x0 >= (uint32_t)ctx->res_w || y0 >= (uint32_t)ctx->res_h) return JXLH_ERR_INVALID_ARGUMENT;
  const size_t cw = std::min<size_t>(w, (size_t)ctx->res_w - x0), ch = std::min<size_t>(h, (size_t)ctx->res_h - y0);
  for (int c = 0; c < 3; c++)
    if (!out[c].ptr || out[c].bytes_per_row < cw * sizeof(float) || out[c].num_rows < ch ||
        out[c].bytes_between_rows < out[c].bytes_per_row)
      return JXLH_ERR_INVALID_ARGUMENT;
  materialise_chroma(ctx);
  for (int c = 0; c < 3; c++) {
    const float* src = ctx->frame.result[c] + (size_t)y0 * ctx->res_stride + x0;
    if (jxlh_status st = copy2d(ctx, out[c].ptr, out[c].bytes_between_rows, src, ctx->res_stride * sizeof(float),
                                cw * sizeof(float), ch, ctx->stream))
      return st;
  }
  return wait ? jxlh_ctx_sync(ctx) : JXLH_OK;
}
}  // namespace

jxlh_status jxlh_frame_read_planes_rect(jxlh_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                        const jxlh_plane out[3]) {
  JXLH_ON_DEVICE(ctx);
  return read_planes_rect(ctx, x0, y0, w, h, out, /*wait=*/true);
}
jxlh_status jxlh_frame_read_planes_rect_async(jxlh_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                              const jxlh_plane out[3]) {
  JXLH_ON_DEVICE(ctx);
  return read_planes_rect(ctx, x0, y0, w, h, out, /*wait=*/false);
}

jxlh_status jxlh_frame_device_planes(jxlh_ctx* ctx, float* planes[3], size_t* stride) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !planes) return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->in_frame || !ctx->frame.result[0]) return JXLH_ERR_BAD_STATE;
  materialise_chroma(ctx);
  for (int c = 0; c < 3; c++) planes[c] = ctx->frame.result[c];
  if (stride) *stride = ctx->res_stride;
  return JXLH_OK;
}

jxlh_status jxlh_frame_read_lf(jxlh_ctx* ctx, float* x, float* y, float* b, size_t stride) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !x || !y || !b) return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->in_frame || ctx->modular) return JXLH_ERR_BAD_STATE;
  const FrameDev& f = ctx->fd;
  if (stride < (size_t)f.xblocks) return JXLH_ERR_INVALID_ARGUMENT;
  float* dst[3] = {x, y, b};
  for (int c = 0; c < 3; c++) {
    jxlh_status st = copy2d(ctx, dst[c], stride * sizeof(float), f.lf[c], f.xblocks * sizeof(float),
                            f.xblocks * sizeof(float), f.yblocks, ctx->stream);
    if (st != JXLH_OK) return st;
  }
  JXLH_SYNC(ctx);
  return JXLH_OK;
}

}  // extern "C"
