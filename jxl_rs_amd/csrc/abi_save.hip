// C ABI of the save tail (frame/render.rs:793-903): spot colours, premultiplication, the conversions to u8 / u16 / f16 /
// f32 at any bit depth and the save stage with its channel order, endianness, opaque-alpha fill and orientation, behind
// the frame's colour stage.  jxlh_frame_save runs it on the frame's result, jxlh_stage_save on caller planes; both launch
// k_save.hip.  jxlh_frame_save_rects / jxlh_stage_save_rects are the same two for a list of source rectangles
// (save_rects_plan.h decides, k_save_rects.hip runs it in one launch); jxlh_changed_rects is that header's host function.
#include <algorithm>
#include <cmath>

#include "../../include/jxl_hip_dev.h"
#include "jxlh_ctx.h"

namespace jxlh_host {

namespace {

uint32_t samples_per_pixel(const jxlh_save_desc* d) { return d->n_channels + (d->fill_opaque_alpha ? 1 : 0); }
bool is_extra(uint32_t ch, uint32_t n_planes) { return ch >= 3 && ch < n_planes; }

}  // namespace

// the descriptor's own checks; n_planes: pipeline channels that exist (3 + JXLH_MAX_EXTRA_CHANNELS for a frame)
jxlh_status save_check_desc(const jxlh_save_desc* d, uint32_t n_planes) {
  if (!d || d->n_channels == 0 || d->n_channels > 4 || samples_per_pixel(d) > 4) return JXLH_ERR_INVALID_ARGUMENT;
  for (uint32_t k = 0; k < d->n_channels; k++)
    if (d->channels[k] >= n_planes) return JXLH_ERR_INVALID_ARGUMENT;
  if (d->format > JXLH_SAVE_F32 || d->orientation < 1 || d->orientation > 8) return JXLH_ERR_INVALID_ARGUMENT;
  if (d->format == JXLH_SAVE_U8 && (d->bit_depth < 1 || d->bit_depth > 8)) return JXLH_ERR_INVALID_ARGUMENT;
  if (d->format == JXLH_SAVE_U16 && (d->bit_depth < 1 || d->bit_depth > 16)) return JXLH_ERR_INVALID_ARGUMENT;
  if (d->f16_clamp && !(d->f16_clamp_min <= d->f16_clamp_max)) return JXLH_ERR_INVALID_ARGUMENT;  // NaN bounds included
  if (d->premultiply && !is_extra(d->premultiply_alpha_channel, n_planes)) return JXLH_ERR_INVALID_ARGUMENT;
  if (d->n_spot > JXLH_MAX_EXTRA_CHANNELS) return JXLH_ERR_INVALID_ARGUMENT;
  for (uint32_t i = 0; i < d->n_spot; i++)
    if (d->spot[i].ec >= JXLH_MAX_EXTRA_CHANNELS || !is_extra(3 + d->spot[i].ec, n_planes)) return JXLH_ERR_INVALID_ARGUMENT;
  return JXLH_OK;
}

// `out` and its pitch against the oriented image of a w x h source
jxlh_status save_check_out(const jxlh_save_desc* d, uint32_t w, uint32_t h, const void* out, size_t bytes_per_row) {
  const size_t bps = (size_t)save_sample_bytes(d->format);
  const size_t row = (size_t)(d->orientation >= 5 ? h : w) * samples_per_pixel(d) * bps;
  if (!out || bytes_per_row < row || bytes_per_row % bps != 0 || reinterpret_cast<uintptr_t>(out) % bps != 0)
    return JXLH_ERR_INVALID_ARGUMENT;
  return JXLH_OK;
}

jxlh_status colour_stage(const jxlh_output_desc* colour, int* mode, XybParamsDev* xyb, TfParamsDev* tf) {
  *mode = kModeNone;
  if (!colour) return JXLH_OK;
  switch (colour->color) {
    case JXLH_COLOR_XYB:
      if (colour->transfer > JXLH_TF_GAMMA) return JXLH_ERR_INVALID_ARGUMENT;
      *mode = (int)colour->transfer;  // JXLH_TF_* share the values of the internal modes
      for (int i = 0; i < 9; i++) xyb->mat[i] = colour->xyb.opsin_inverse_matrix[i];
      for (int i = 0; i < 3; i++) {
        xyb->bias_cbrt[i] = colour->xyb.bias_cbrt[i];
        xyb->scaled_bias[i] = colour->xyb.scaled_bias[i];
      }
      xyb->intensity_scale = colour->xyb.intensity_scale;
      break;
    case JXLH_COLOR_YCBCR: *mode = kModeYcbcr; break;
    case JXLH_COLOR_NONE: break;
    default: return JXLH_ERR_INVALID_ARGUMENT;
  }
  tf->param = colour->tf_param;
  for (int i = 0; i < 3; i++) tf->lum[i] = colour->hlg_luminance_rgb[i];
  return JXLH_OK;
}

namespace {

// everything of the launch the (checked) descriptor decides; plane(ch) / stride(ch) resolve a pipeline channel
template <class PlaneOf, class StrideOf>
void fill_desc(const jxlh_save_desc* d, PlaneOf plane, StrideOf stride, SaveLaunch& a) {
  save_format(d, a);
  a.spp = (int)samples_per_pixel(d);
  a.colour = 0;
  for (uint32_t k = 0; k < 4; k++) {
    a.ch[k] = kSaveFill;
    a.smp_plane[k] = nullptr;
    a.smp_stride[k] = 0;
    if (k >= d->n_channels) continue;
    a.ch[k] = (int)d->channels[k];
    if (d->channels[k] < 3) {
      a.colour = 1;
    } else {
      a.smp_plane[k] = plane(d->channels[k]);
      a.smp_stride[k] = stride(d->channels[k]);
    }
  }
  for (int c = 0; c < 3; c++) {
    a.plane[c] = plane(c);
    a.stride[c] = stride(c);
  }
  // spot colours and premultiplication act on the colour channels only: an extra-channel save carries none of them
  a.n_spot = a.colour ? (int)d->n_spot : 0;
  for (int i = 0; i < a.n_spot; i++) {
    a.spot_plane[i] = plane(3 + d->spot[i].ec);
    a.spot_stride[i] = stride(3 + d->spot[i].ec);
    for (int k = 0; k < 4; k++) a.spot[i][k] = d->spot[i].rgba[k];
  }
  const bool premul = a.colour && d->premultiply;
  a.premul_plane = premul ? plane(d->premultiply_alpha_channel) : nullptr;
  a.premul_stride = premul ? stride(d->premultiply_alpha_channel) : 0;
  a.clamp = d->format == JXLH_SAVE_F16 && d->f16_clamp;
  a.clamp_min = d->f16_clamp_min;
  a.clamp_max = d->f16_clamp_max;
}

// Launches `a` (everything but out / out_stride filled) for source rows [a.y0, a.y0 + a.rows) into the oriented image at
// `image`: the band's rectangle there is whole rows of it for orientations 1-4, a column range of every row for 5-8.
jxlh_status launch_to(jxlh_ctx* ctx, SaveLaunch& a, void* image, size_t bytes_per_row, const char* label, bool wait) {
  const size_t pb = (size_t)a.spp * (size_t)save_sample_bytes((uint32_t)a.format);
  const int y1 = a.y0 + a.rows;
  const OutRect r = a.transpose ? OutRect{(size_t)(a.flip_x ? a.h - y1 : a.y0), 0, (size_t)a.rows, (size_t)a.w}
                                : OutRect{0, (size_t)(a.flip_y ? a.h - y1 : a.y0), (size_t)a.w, (size_t)a.rows};
  void* dst = reinterpret_cast<void*>(reinterpret_cast<uintptr_t>(image) + r.y0 * bytes_per_row + r.x0 * pb);
  return write_out(ctx, dst, bytes_per_row, pb, r, label, wait, [&](uint8_t* origin, size_t pitch) {
    a.out = origin;
    a.out_stride = pitch;
    launch_save(ctx->stream, a);
  });
}

// the frame's result and the extra channels the save names as the launch reads them, and the result's geometry
void fill_result_launch(jxlh_ctx* ctx, SaveLaunch& a, const jxlh_save_desc* d, const float* const* ec_plane,
                        const uint32_t* ec_stride) {
  fill_desc(
      d, [&](uint32_t ch) { return ch < 3 ? (const float*)ctx->frame.result[ch] : ec_plane[ch - 3]; },
      [&](uint32_t ch) { return ch < 3 ? (uint32_t)ctx->res_stride : ec_stride[ch - 3]; }, a);
  a.w = ctx->res_w;
  a.h = ctx->res_h;
  a.y0 = a.rows = 0;
  a.dx = a.dy = 0;
}

// The rect-list tail (save_rects_plan.h decides, this issues): the work list goes up on the stream, ONE launch writes
// every rect -- into the caller's device image, or into the rects' packed blocks of ctx->rgb8, which then leave with one
// 2-D copy of exactly the pixel bytes per rect.  `a`: everything but out filled.
jxlh_status issue_save_rects(jxlh_ctx* ctx, SaveLaunch& a, SaveRectsPlan& plan, bool staged, void* image,
                             size_t bytes_per_row, bool wait) {
  if (plan.work.empty()) return JXLH_OK;
  const size_t pb = (size_t)a.spp * (size_t)save_sample_bytes((uint32_t)a.format);
  const uint32_t n = (uint32_t)plan.work.size();
  if (staged)
    if (jxlh_status st = ensure(ctx, ctx->rgb8, (size_t)plan.staging_bytes)) return st;
  if (jxlh_status st = ensure(ctx, ctx->save_rects_dev, n)) return st;
  HIPCHK(ctx, ctx->save_rects_copied.sync());  // the pinned block's previous list is on its way
  ctx->save_rects_copied.clear();
  if (ctx->save_rects_host.n < n) {
    HIPCHK(ctx, ctx->save_rects_host.reset());
    HIPCHK(ctx, ctx->save_rects_host.alloc(n + n / 2));
  }
  std::memcpy(ctx->save_rects_host.p, plan.work.data(), n * sizeof(SaveRectWork));
  HIPCHK(ctx, hipMemcpyAsync(ctx->save_rects_dev.p, ctx->save_rects_host.p, n * sizeof(SaveRectWork), hipMemcpyHostToDevice,
                             ctx->stream));
  HIPCHK(ctx, ctx->save_rects_copied.record(ctx->stream));
  a.out = staged ? ctx->rgb8.p : static_cast<uint8_t*>(image);
  a.out_stride = 0;  // every rect carries its own
  {
    ScopedKernelTimer t(ctx, "k_save_rects");
    launch_save_rects(ctx->stream, a, ctx->save_rects_dev.p, n, plan.groups);
  }
  HIPCHK(ctx, hipGetLastError());
  if (!staged) return JXLH_OK;
  for (const SaveRectOut& o : plan.out) {
    void* dst = reinterpret_cast<void*>(reinterpret_cast<uintptr_t>(image) + o.oy0 * bytes_per_row + o.ox0 * pb);
    if (jxlh_status st = copy2d(ctx, dst, bytes_per_row, ctx->rgb8.p + o.stage_off, o.stage_pitch, o.row_bytes, o.oh,
                                ctx->stream))
      return st;
  }
  if (wait) JXLH_SYNC(ctx);
  return JXLH_OK;
}

// jxlh_frame_save (rects == nullptr && !by_rects: rows [y0, y1)) and jxlh_frame_save_rects (by_rects: the list)
jxlh_status frame_save(jxlh_ctx* ctx, const jxlh_output_desc* colour, const jxlh_save_desc* d, uint32_t y0, uint32_t y1,
                       void* out, size_t bytes_per_row, bool wait, bool by_rects = false, const jxlh_rect* rects = nullptr,
                       uint32_t n_rects = 0) {
  if (!ctx || !d || !out) return JXLH_ERR_INVALID_ARGUMENT;
  if (by_rects && (n_rects > JXLH_MAX_SAVE_RECTS || (n_rects && !rects))) return JXLH_ERR_INVALID_ARGUMENT;
  if (comm_nranks(ctx) > 1) return JXLH_ERR_UNSUPPORTED;  // a rank holds only its band
  if (jxlh_status st = save_check_desc(d, 3 + JXLH_MAX_EXTRA_CHANNELS)) return st;
  SaveLaunch a{};
  if (jxlh_status st = colour_stage(colour, &a.mode, &a.xyb, &a.tf)) return st;
  if (!ctx->in_frame || !ctx->frame.result[0]) return JXLH_ERR_BAD_STATE;
  if (blended(ctx) && a.mode != kModeNone) return JXLH_ERR_BAD_STATE;  // jxlh_frame_blend has run the colour stage already
  const uint32_t w = (uint32_t)ctx->res_w, h = (uint32_t)ctx->res_h;
  if (by_rects) {
    if (jxlh_status st = check_save_rects(rects, n_rects, w, h)) return st;
  } else {
    if (y1 > h) y1 = h;
    if (y0 >= y1) return JXLH_ERR_INVALID_ARGUMENT;
  }
  if (jxlh_status st = save_check_out(d, w, h, out, bytes_per_row)) return st;
  if ((uint64_t)w * h >= (1ull << 31)) return JXLH_ERR_UNSUPPORTED;
  // the extra channels the save reads, as jxlh_frame_read_extra_channel resolves them
  const float* ec_plane[JXLH_MAX_EXTRA_CHANNELS] = {};
  uint32_t ec_stride[JXLH_MAX_EXTRA_CHANNELS] = {};
  auto resolve = [&](uint32_t ch) -> jxlh_status {
    if (ch < 3) return JXLH_OK;
    const uint32_t ec = ch - 3;
    const jxlh_ctx::ExtraChannel& e = ctx->extra[ec];
    if (!e.set || !e.done) return JXLH_ERR_BAD_STATE;
    if (blended(ctx)) {  // the composed channel, image-sized
      if (ec >= ctx->frame.blend_nec) return JXLH_ERR_BAD_STATE;
      ec_plane[ec] = ctx->blend_canvas.p + (size_t)(3 + ec) * ctx->res_stride * h;
      ec_stride[ec] = (uint32_t)ctx->res_stride;
      return JXLH_OK;
    }
    if (e.out_w != w || e.out_h != h) return JXLH_ERR_BAD_STATE;  // it does not cover the result
    ec_plane[ec] = e.pat_ready ? e.pat.p : e.up > 1 ? e.out.p : e.f32.p;
    ec_stride[ec] = (uint32_t)e.out_stride;
    return JXLH_OK;
  };
  bool colour_named = false;
  for (uint32_t k = 0; k < d->n_channels; k++) {
    colour_named |= d->channels[k] < 3;
    if (jxlh_status st = resolve(d->channels[k])) return st;
  }
  if (colour_named) {
    if (d->premultiply)
      if (jxlh_status st = resolve(d->premultiply_alpha_channel)) return st;
    for (uint32_t i = 0; i < d->n_spot; i++)
      if (jxlh_status st = resolve(3 + d->spot[i].ec)) return st;
  }
  if (!by_rects) return save_result_rows(ctx, a, d, ec_plane, ec_stride, y0, y1, out, bytes_per_row, "k_save", wait);
  const bool staged = !is_device_ptr(out);
  SaveRectsPlan plan = plan_save_rects(rects, n_rects, w, h, d->orientation,
                                       samples_per_pixel(d) * (uint32_t)save_sample_bytes(d->format), staged, bytes_per_row);
  if (plan.status != JXLH_OK) return plan.status;
  if (plan.work.empty()) return JXLH_OK;  // nothing to write: nothing enqueued
  materialise_chroma(ctx);
  fill_result_launch(ctx, a, d, ec_plane, ec_stride);
  return issue_save_rects(ctx, a, plan, staged, out, bytes_per_row, wait);
}

}  // namespace

// checked: from here on only the device can fail.  launch_save's own precondition is ceil(w / 1024) * rows < 2^31
// workgroups (fewer for the tiles of orientations 5-8).  The save entry points have refused w * h >= 2^31; a read-out
// comes with any result: ceil(w / 1024) * h <= w * h / 1024 + h, where h <= 2^23 (a side of 2^20, upsampled eight times)
// and w * h < 2^35 for three f32 planes that exist in device memory -- below 2^26
jxlh_status save_result_rows(jxlh_ctx* ctx, SaveLaunch& a, const jxlh_save_desc* d, const float* const* ec_plane,
                             const uint32_t* ec_stride, uint32_t y0, uint32_t y1, void* image, size_t bytes_per_row,
                             const char* label, bool wait) {
  materialise_chroma(ctx);
  fill_desc(
      d, [&](uint32_t ch) { return ch < 3 ? (const float*)ctx->frame.result[ch] : ec_plane[ch - 3]; },
      [&](uint32_t ch) { return ch < 3 ? (uint32_t)ctx->res_stride : ec_stride[ch - 3]; }, a);
  a.w = ctx->res_w;
  a.h = ctx->res_h;
  a.y0 = (int)y0;
  a.rows = (int)(y1 - y0);
  a.dx = a.dy = 0;
  return launch_to(ctx, a, image, bytes_per_row, label, wait);
}

}  // namespace jxlh_host

extern "C" {

// jxl_hip_dev.h
jxlh_status jxlh_save_tile_layout(uint32_t pixel_bytes, uint32_t* columns, uint32_t* rows) {
  if (pixel_bytes < 1 || pixel_bytes > 16 || !columns || !rows) return JXLH_ERR_INVALID_ARGUMENT;
  *columns = (uint32_t)kSaveTile;
  *rows = (uint32_t)save_tile_rows((int)pixel_bytes);
  return JXLH_OK;
}

jxlh_status jxlh_frame_save(jxlh_ctx* ctx, const jxlh_output_desc* colour, const jxlh_save_desc* save, uint32_t y0,
                            uint32_t y1, void* out, size_t bytes_per_row) {
  JXLH_ON_DEVICE(ctx);
  return frame_save(ctx, colour, save, y0, y1, out, bytes_per_row, /*wait=*/true);
}

jxlh_status jxlh_frame_save_async(jxlh_ctx* ctx, const jxlh_output_desc* colour, const jxlh_save_desc* save, uint32_t y0,
                                  uint32_t y1, void* out, size_t bytes_per_row) {
  JXLH_ON_DEVICE(ctx);
  return frame_save(ctx, colour, save, y0, y1, out, bytes_per_row, /*wait=*/false);
}

jxlh_status jxlh_frame_save_rects(jxlh_ctx* ctx, const jxlh_output_desc* colour, const jxlh_save_desc* save,
                                  const jxlh_rect* rects, uint32_t n, void* out, size_t bytes_per_row) {
  JXLH_ON_DEVICE(ctx);
  return frame_save(ctx, colour, save, 0, 0, out, bytes_per_row, /*wait=*/true, /*by_rects=*/true, rects, n);
}

jxlh_status jxlh_frame_save_rects_async(jxlh_ctx* ctx, const jxlh_output_desc* colour, const jxlh_save_desc* save,
                                        const jxlh_rect* rects, uint32_t n, void* out, size_t bytes_per_row) {
  JXLH_ON_DEVICE(ctx);
  return frame_save(ctx, colour, save, 0, 0, out, bytes_per_row, /*wait=*/false, /*by_rects=*/true, rects, n);
}

// pure host code (save_rects_plan.h)
jxlh_status jxlh_changed_rects(const jxlh_frame_params* p, const uint32_t* group_ids, uint32_t count, jxlh_rect* rects,
                               uint32_t cap, uint32_t* n) {
  if (!p || !n || (count && !group_ids) || (cap && !rects)) return JXLH_ERR_INVALID_ARGUMENT;
  std::vector<jxlh_rect> need;
  if (jxlh_status st = plan_changed_rects(*p, group_ids, count, need)) return st;
  *n = (uint32_t)need.size();
  if (need.size() > cap) return JXLH_ERR_INVALID_ARGUMENT;
  std::copy(need.begin(), need.end(), rects);
  return JXLH_OK;
}

// pure host code (repaint_plan.h)
jxlh_status jxlh_repaint_changed_rects(const jxlh_frame_params* p, const uint32_t* group_ids, uint32_t count,
                                       jxlh_rect* rects, uint32_t cap, uint32_t* n) {
  if (!p || !n || (count && !group_ids) || (cap && !rects)) return JXLH_ERR_INVALID_ARGUMENT;
  std::vector<jxlh_rect> need;
  if (jxlh_status st = plan_repaint_changed_rects(*p, group_ids, count, need)) return st;
  *n = (uint32_t)need.size();
  if (need.size() > cap) return JXLH_ERR_INVALID_ARGUMENT;
  std::copy(need.begin(), need.end(), rects);
  return JXLH_OK;
}

// jxlh_stage_save (rows [y0, y1)) and jxlh_stage_save_rects (by_rects: the list)
static jxlh_status stage_save(jxlh_ctx* ctx, const jxlh_output_desc* colour, const jxlh_save_desc* d,
                              const float* const planes[], uint32_t n_planes, uint32_t w, uint32_t h, size_t stride,
                              uint32_t frame_x0, uint32_t frame_y0, uint32_t y0, uint32_t y1, void* out,
                              size_t bytes_per_row, bool by_rects, const jxlh_rect* rects, uint32_t n_rects) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !d || !planes || !out || w == 0 || h == 0 || stride < w || stride > 0xffffffffu)
    return JXLH_ERR_INVALID_ARGUMENT;
  if (by_rects && (n_rects > JXLH_MAX_SAVE_RECTS || (n_rects && !rects))) return JXLH_ERR_INVALID_ARGUMENT;
  if (n_planes < 3 || n_planes > 3 + JXLH_MAX_EXTRA_CHANNELS) return JXLH_ERR_INVALID_ARGUMENT;
  for (uint32_t c = 0; c < n_planes; c++)
    if (!planes[c]) return JXLH_ERR_INVALID_ARGUMENT;
  if (jxlh_status st = save_check_desc(d, n_planes)) return st;
  SaveLaunch a{};
  if (jxlh_status st = colour_stage(colour, &a.mode, &a.xyb, &a.tf)) return st;
  if (by_rects) {
    if (jxlh_status st = check_save_rects(rects, n_rects, w, h)) return st;
  } else {
    if (y1 > h) y1 = h;
    if (y0 >= y1) return JXLH_ERR_INVALID_ARGUMENT;
  }
  if (jxlh_status st = save_check_out(d, w, h, out, bytes_per_row)) return st;
  if ((uint64_t)w * h >= (1ull << 31)) return JXLH_ERR_UNSUPPORTED;
  const bool staged_out = by_rects && !is_device_ptr(out);
  SaveRectsPlan plan;
  if (by_rects) {
    plan = plan_save_rects(rects, n_rects, w, h, d->orientation,
                           (d->n_channels + (d->fill_opaque_alpha ? 1 : 0)) * (uint32_t)save_sample_bytes(d->format),
                           staged_out, bytes_per_row);
    if (plan.status != JXLH_OK) return plan.status;
    if (plan.work.empty()) return JXLH_OK;  // nothing to write: nothing enqueued
  }
  // host planes are staged whole, rows 16-byte aligned; device planes are read where they are
  const size_t sstride = round_up(w, 4), splane = sstride * h;
  bool all_device = true;
  for (uint32_t c = 0; c < n_planes; c++) all_device &= is_device_ptr(planes[c]);
  if (!all_device) {
    if (jxlh_status st = ensure(ctx, ctx->save_hook_in, splane * n_planes)) return st;
    for (uint32_t c = 0; c < n_planes; c++)
      if (jxlh_status st = copy2d(ctx, ctx->save_hook_in.p + c * splane, sstride * sizeof(float), planes[c],
                                  stride * sizeof(float), (size_t)w * sizeof(float), h, ctx->stream))
        return st;
  }
  fill_desc(
      d, [&](uint32_t ch) { return all_device ? planes[ch] : (const float*)(ctx->save_hook_in.p + ch * splane); },
      [&](uint32_t) { return (uint32_t)(all_device ? stride : sstride); }, a);
  a.w = (int)w;
  a.h = (int)h;
  a.y0 = (int)y0;
  a.rows = (int)(y1 - y0);
  a.dx = (int)(frame_x0 & 31);  // the table is 32 x 32
  a.dy = (int)(frame_y0 & 31);
  if (by_rects) {
    if (jxlh_status st = issue_save_rects(ctx, a, plan, staged_out, out, bytes_per_row, /*wait=*/false)) return st;
  } else {
    if (jxlh_status st = launch_to(ctx, a, out, bytes_per_row, "k_save", /*wait=*/false)) return st;
  }
  JXLH_SYNC(ctx);
  return JXLH_OK;
}

jxlh_status jxlh_stage_save(jxlh_ctx* ctx, const jxlh_output_desc* colour, const jxlh_save_desc* d,
                            const float* const planes[], uint32_t n_planes, uint32_t w, uint32_t h, size_t stride,
                            uint32_t frame_x0, uint32_t frame_y0, uint32_t y0, uint32_t y1, void* out,
                            size_t bytes_per_row) {
  return stage_save(ctx, colour, d, planes, n_planes, w, h, stride, frame_x0, frame_y0, y0, y1, out, bytes_per_row,
                    /*by_rects=*/false, nullptr, 0);
}

jxlh_status jxlh_stage_save_rects(jxlh_ctx* ctx, const jxlh_output_desc* colour, const jxlh_save_desc* d,
                                  const float* const planes[], uint32_t n_planes, uint32_t w, uint32_t h, size_t stride,
                                  uint32_t frame_x0, uint32_t frame_y0, const jxlh_rect* rects, uint32_t n, void* out,
                                  size_t bytes_per_row) {
  return stage_save(ctx, colour, d, planes, n_planes, w, h, stride, frame_x0, frame_y0, 0, 0, out, bytes_per_row,
                    /*by_rects=*/true, rects, n);
}

}  // extern "C"
