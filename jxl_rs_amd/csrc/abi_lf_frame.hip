// C ABI of LF frames (frames with lf_level != 0, the layers of a progressive_dc file):
//   the four LF slots of DecoderState::lf_frames (frame/mod.rs:120,136,399-401) next to the reference slots:
//     jxlh_ctx_set_lf_frame / jxlh_frame_save_lf / jxlh_ctx_clear_lf_frame;
//   a VarDCT frame with USE_LF_FRAME taking a slot as its LF image (frame/decode.rs:172-178,737-743):
//     jxlh_frame_set_lf_from_slot -- no LF of its own, no adaptive LF smoothing (frame_header.rs:496-500);
//   the full-size preview of slot 0 (frame/lf_preview.rs): jxlh_lf_preview, one launch of k_lf_preview.hip.
#include <algorithm>

#include "jxlh_ctx.h"

namespace jxlh_host {

namespace {

constexpr uint32_t kMaxSide = 1u << 20;

// the slot holds w x h, reallocating only when it grows
jxlh_status slot_reserve(jxlh_ctx* ctx, jxlh_ctx::LfSlot& s, uint32_t w, uint32_t h, size_t* stride) {
  *stride = round_up(w, 64);
  return ensure(ctx, s.buf, *stride * h * 3);
}

void slot_commit(jxlh_ctx::LfSlot& s, uint32_t w, uint32_t h, size_t stride) {
  s.set = true;
  s.w = w;
  s.h = h;
  s.stride = stride;
}

jxlh_status lf_preview(jxlh_ctx* ctx, uint32_t slot, uint32_t image_w, uint32_t image_h, uint32_t x0, uint32_t y0,
                       uint32_t w, uint32_t h, const jxlh_output_desc* colour, const jxlh_save_desc* save, void* out,
                       size_t bytes_per_row, bool wait) {
  if (!ctx || !save || !out || slot >= JXLH_NUM_LF_FRAMES) return JXLH_ERR_INVALID_ARGUMENT;
  if (comm_nranks(ctx) > 1) return JXLH_ERR_UNSUPPORTED;
  jxlh_save_desc desc = *save;
  desc.f16_clamp = 0;  // ConvertF32ToF16Stage::new(0): the clamp fields are not read, not even checked
  const jxlh_save_desc* d = &desc;
  if (jxlh_status st = save_check_desc(d, 3)) return st;
  const bool rgb = d->channels[0] == 0 && d->channels[1] == 1 && d->channels[2] == 2;
  const bool bgr = d->channels[0] == 2 && d->channels[1] == 1 && d->channels[2] == 0;
  if (d->n_channels != 3 || !(rgb || bgr) || d->premultiply || d->n_spot) return JXLH_ERR_INVALID_ARGUMENT;
  LfPreviewLaunch a{};
  if (jxlh_status st = colour_stage(colour, &a.mode, &a.xyb, &a.tf)) return st;
  // the cases in which the reference shows no preview (lf_preview.rs: Ok(false))
  if (!colour || colour->color != JXLH_COLOR_XYB || a.mode == kTfLinear) return JXLH_ERR_UNSUPPORTED;
  const jxlh_ctx::LfSlot& s = ctx->lf_slots[slot];
  if (!s.set || image_w == 0 || image_h == 0 || s.w != (image_w + 7) / 8 || s.h != (image_h + 7) / 8)
    return JXLH_ERR_INVALID_ARGUMENT;
  if ((uint64_t)x0 + w > s.w || (uint64_t)y0 + h > s.h) return JXLH_ERR_INVALID_ARGUMENT;
  if (jxlh_status st = save_check_out(d, image_w, image_h, out, bytes_per_row)) return st;
  if ((uint64_t)image_w * image_h >= (1ull << 31)) return JXLH_ERR_UNSUPPORTED;
  if (w == 0 || h == 0) return JXLH_OK;
  // checked: from here on only the device can fail
  if (jxlh_status st = upload_upsampling_kernels(ctx, 8)) return st;
  for (int c = 0; c < 3; c++) a.plane[c] = s.buf.p + (size_t)c * s.stride * s.h;
  a.stride = (uint32_t)s.stride;
  a.sw = (int)s.w;
  a.sh = (int)s.h;
  a.x0 = (int)x0;
  a.y0 = (int)y0;
  a.w = (int)w;
  a.h = (int)h;
  a.iw = (int)image_w;
  a.ih = (int)image_h;
  a.kernels = ctx->ups_kernels.p;
  save_format(d, a);
  a.spp = d->fill_opaque_alpha ? 4 : 3;
  a.bgr = bgr;
  // the rectangle of the oriented image the rect's pixels land in
  const size_t ix0 = (size_t)x0 * 8, iy0 = (size_t)y0 * 8;
  const size_t ix1 = std::min<size_t>(((size_t)x0 + w) * 8, image_w), iy1 = std::min<size_t>(((size_t)y0 + h) * 8, image_h);
  OutRect r;
  r.x0 = a.flip_x ? (a.transpose ? image_h - iy1 : image_w - ix1) : (a.transpose ? iy0 : ix0);
  r.y0 = a.flip_y ? (a.transpose ? image_w - ix1 : image_h - iy1) : (a.transpose ? ix0 : iy0);
  r.w = a.transpose ? iy1 - iy0 : ix1 - ix0;
  r.h = a.transpose ? ix1 - ix0 : iy1 - iy0;
  const size_t pb = (size_t)a.spp * (size_t)save_sample_bytes(d->format);
  if (jxlh_status st = write_out(ctx, static_cast<uint8_t*>(out) + r.y0 * bytes_per_row + r.x0 * pb, bytes_per_row, pb, r,
                                 "k_lf_preview", /*wait=*/false, [&](uint8_t* origin, size_t pitch) {
                                   a.out = origin;
                                   a.out_stride = pitch;
                                   launch_lf_preview(ctx->stream, a);
                                 }))
    return st;
  if (wait) JXLH_SYNC(ctx);  // a device destination included
  return JXLH_OK;
}

}  // namespace

}  // namespace jxlh_host

extern "C" {

jxlh_status jxlh_ctx_set_lf_frame(jxlh_ctx* ctx, uint32_t slot, uint32_t w, uint32_t h, const float* x, const float* y,
                                  const float* b, size_t stride) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || slot >= JXLH_NUM_LF_FRAMES || !x || !y || !b || w == 0 || h == 0 || w > kMaxSide || h > kMaxSide ||
      stride < w)
    return JXLH_ERR_INVALID_ARGUMENT;
  if (comm_nranks(ctx) > 1) return JXLH_ERR_UNSUPPORTED;
  jxlh_ctx::LfSlot& s = ctx->lf_slots[slot];
  size_t dstride;
  if (jxlh_status st = slot_reserve(ctx, s, w, h, &dstride)) return st;
  const float* src[3] = {x, y, b};
  for (int c = 0; c < 3; c++)
    if (jxlh_status st = copy2d(ctx, s.buf.p + (size_t)c * dstride * h, dstride * sizeof(float), src[c],
                                stride * sizeof(float), (size_t)w * sizeof(float), h, ctx->stream))
      return st;
  JXLH_SYNC(ctx);  // the caller's planes may be reused as soon as the call returns
  slot_commit(s, w, h, dstride);
  return JXLH_OK;
}

jxlh_status jxlh_frame_save_lf(jxlh_ctx* ctx, uint32_t slot) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || slot >= JXLH_NUM_LF_FRAMES) return JXLH_ERR_INVALID_ARGUMENT;
  if (comm_nranks(ctx) > 1) return JXLH_ERR_UNSUPPORTED;
  if (!ctx->in_frame || !ctx->frame.rendered || !ctx->frame.result[0] || blended(ctx)) return JXLH_ERR_BAD_STATE;
  materialise_chroma(ctx);
  const uint32_t w = (uint32_t)ctx->res_w, h = (uint32_t)ctx->res_h;
  jxlh_ctx::LfSlot& s = ctx->lf_slots[slot];
  size_t dstride;
  if (jxlh_status st = slot_reserve(ctx, s, w, h, &dstride)) return st;
  for (int c = 0; c < 3; c++)
    HIPCHK(ctx, hipMemcpy2DAsync(s.buf.p + (size_t)c * dstride * h, dstride * sizeof(float), ctx->frame.result[c],
                                 ctx->res_stride * sizeof(float), (size_t)w * sizeof(float), h, hipMemcpyDeviceToDevice,
                                 ctx->stream));
  slot_commit(s, w, h, dstride);
  return JXLH_OK;
}

jxlh_status jxlh_ctx_clear_lf_frame(jxlh_ctx* ctx, uint32_t slot) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || slot >= JXLH_NUM_LF_FRAMES) return JXLH_ERR_INVALID_ARGUMENT;
  jxlh_ctx::LfSlot& s = ctx->lf_slots[slot];
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // (a queued copy or preview may still read the slot)
  (void)s.buf.reset();
  s = jxlh_ctx::LfSlot{};
  return JXLH_OK;
}

jxlh_status jxlh_frame_set_lf_from_slot(jxlh_ctx* ctx, uint32_t slot) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || slot >= JXLH_NUM_LF_FRAMES) return JXLH_ERR_INVALID_ARGUMENT;
  if (comm_nranks(ctx) > 1) return JXLH_ERR_UNSUPPORTED;
  if (!ctx->in_frame || ctx->modular || ctx->frame.lf_from_caller) return JXLH_ERR_BAD_STATE;
  const FrameDev& f = ctx->fd;
  if (f.subsampled) return JXLH_ERR_UNSUPPORTED;  // size_blocks rounds past the LF frame's size
  const jxlh_ctx::LfSlot& s = ctx->lf_slots[slot];
  if (!s.set || s.w != (uint32_t)f.xblocks || s.h != (uint32_t)f.yblocks) return JXLH_ERR_INVALID_ARGUMENT;
  for (int c = 0; c < 3; c++)
    HIPCHK(ctx, hipMemcpy2DAsync(ctx->lf_raw[c].p, (size_t)f.xblocks * sizeof(float), s.buf.p + (size_t)c * s.stride * s.h,
                                 s.stride * sizeof(float), (size_t)f.xblocks * sizeof(float), (size_t)f.yblocks,
                                 hipMemcpyDeviceToDevice, ctx->stream));
  ctx->frame.lf_from_slot = true;
  ctx->frame.lf_smoothed = false;
  for (int c = 0; c < 3; c++) ctx->fd.lf[c] = ctx->lf_raw[c].p;
  return JXLH_OK;
}

jxlh_status jxlh_lf_preview(jxlh_ctx* ctx, uint32_t slot, uint32_t image_w, uint32_t image_h, uint32_t x0, uint32_t y0,
                            uint32_t w, uint32_t h, const jxlh_output_desc* colour, const jxlh_save_desc* save, void* out,
                            size_t bytes_per_row) {
  JXLH_ON_DEVICE(ctx);
  return lf_preview(ctx, slot, image_w, image_h, x0, y0, w, h, colour, save, out, bytes_per_row, /*wait=*/true);
}

jxlh_status jxlh_lf_preview_async(jxlh_ctx* ctx, uint32_t slot, uint32_t image_w, uint32_t image_h, uint32_t x0,
                                  uint32_t y0, uint32_t w, uint32_t h, const jxlh_output_desc* colour,
                                  const jxlh_save_desc* save, void* out, size_t bytes_per_row) {
  JXLH_ON_DEVICE(ctx);
  return lf_preview(ctx, slot, image_w, image_h, x0, y0, w, h, colour, save, out, bytes_per_row, /*wait=*/false);
}

}  // extern "C"
