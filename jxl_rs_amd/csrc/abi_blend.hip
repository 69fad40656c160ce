// C ABI of frame blending: BlendingStage + ExtendToImageDimensionsStage (jxl/src/render/stages/blending.rs, extend.rs)
// behind the frame's colour stage, as frame/render.rs:754-791 chains them.  jxlh_frame_blend composes the current frame's
// result onto an image-sized canvas that becomes the frame's result; jxlh_stage_blend runs the same kernel (k_blend.hip)
// on caller planes.  jxlh_frame_blend_rects / jxlh_stage_blend_rects recompose only a list of image rectangles of a
// canvas that holds a composition already (k_blend_rects.hip, blend_rects_plan.h); jxlh_blend_image_rects is host code.
#include <algorithm>

#include "blend_device.h"
#include "jxlh_ctx.h"

namespace jxlh_host {

namespace {

// the descriptor's own checks (no frame or plane involved), and the source slots against the image
jxlh_status check_desc(const jxlh_ctx* ctx, const jxlh_blend_desc* d) {
  if (!d || d->num_ec > JXLH_MAX_EXTRA_CHANNELS) return JXLH_ERR_INVALID_ARGUMENT;
  if (d->image_w == 0 || d->image_h == 0 || (uint64_t)d->image_w * d->image_h >= (1ull << 31))
    return JXLH_ERR_INVALID_ARGUMENT;
  for (uint32_t k = 0; k <= d->num_ec; k++) {
    const jxlh_blending_info& b = k == 0 ? d->color : d->ec[k - 1];
    if (b.mode > JXLH_BLEND_MUL || b.source >= JXLH_MAX_REFERENCE_FRAMES) return JXLH_ERR_INVALID_ARGUMENT;
    // the reference's header check (frame_header.rs, test_invalid_blending_alpha_channel); not read for other modes
    const bool alpha_mode = b.mode == JXLH_BLEND_BLEND || b.mode == JXLH_BLEND_ALPHA_WEIGHTED_ADD;
    if (alpha_mode && d->num_ec > 0 && b.alpha_channel >= d->num_ec) return JXLH_ERR_INVALID_ARGUMENT;
    const jxlh_ctx::RefSlot& r = ctx->refs[b.source];
    if (r.set && (r.w < d->image_w || r.h < d->image_h || r.n_channels != 3 + d->num_ec)) return JXLH_ERR_INVALID_ARGUMENT;
  }
  return JXLH_OK;
}

// From<&BlendingInfo> for PatchBlending (blending.rs:41-56)
uint32_t map_blending(const jxlh_blending_info& b, uint32_t num_ec) {
  static const uint32_t mode[5] = {kBlendNone, kBlendAdd, kBlendBelow, kBlendAddBelow, kBlendMul};
  const bool alpha_mode = b.mode == JXLH_BLEND_BLEND || b.mode == JXLH_BLEND_ALPHA_WEIGHTED_ADD;
  return pack_blending(mode[b.mode], alpha_mode && num_ec > 0 ? b.alpha_channel : 0, b.clamp != 0);
}

// everything of the launch the descriptor and the slots decide (checked by check_desc)
void fill_desc(const jxlh_ctx* ctx, const jxlh_blend_desc* d, BlendLaunch& a) {
  // an origin beyond +-2^30 leaves the frame wholly outside the image, and so does the clamped one
  a.x0 = std::min(std::max(d->x0, -(1 << 30)), 1 << 30);
  a.y0 = std::min(std::max(d->y0, -(1 << 30)), 1 << 30);
  a.iw = (int)d->image_w;
  a.ih = (int)d->image_h;
  a.ec_alpha = a.ec_assoc = 0;
  for (uint32_t k = 0; k <= d->num_ec; k++) a.blend[k] = map_blending(k == 0 ? d->color : d->ec[k - 1], d->num_ec);
  for (uint32_t i = 0; i < d->num_ec; i++) {
    if (d->ec_flags[i] & JXLH_EC_ALPHA) a.ec_alpha |= 1u << i;
    if (d->ec_flags[i] & JXLH_EC_ALPHA_ASSOCIATED) a.ec_assoc |= 1u << i;
  }
  for (uint32_t c = 0; c < 3 + d->num_ec; c++) {
    const jxlh_ctx::RefSlot& r = ctx->refs[c < 3 ? d->color.source : d->ec[c - 3].source];
    a.src[c] = r.set ? r.buf.p + (size_t)c * r.stride * r.h : nullptr;
    a.src_stride[c] = r.set ? (uint32_t)r.stride : 0;
  }
}

// the kernel works in int: sides up to 2^30 (the codestream's own limit) keep every x0 + w and tile edge below 2^31
bool sides_ok(const jxlh_blend_desc* d, uint32_t w, uint32_t h) {
  const uint32_t lim = 1u << 30;
  return d->image_w <= lim && d->image_h <= lim && w <= lim && h <= lim;
}

// the fields of two descriptors the blend reads (check_desc has passed both), equal: what map_blending and fill_desc
// take from them
bool same_composition(const jxlh_blend_desc& p, const jxlh_blend_desc& q) {
  if (p.x0 != q.x0 || p.y0 != q.y0 || p.image_w != q.image_w || p.image_h != q.image_h || p.num_ec != q.num_ec) return false;
  for (uint32_t k = 0; k <= p.num_ec; k++) {
    const jxlh_blending_info& a = k == 0 ? p.color : p.ec[k - 1];
    const jxlh_blending_info& b = k == 0 ? q.color : q.ec[k - 1];
    if (a.mode != b.mode || (a.clamp != 0) != (b.clamp != 0) || a.source != b.source) return false;
    const bool alpha_mode = a.mode == JXLH_BLEND_BLEND || a.mode == JXLH_BLEND_ALPHA_WEIGHTED_ADD;
    if (alpha_mode && p.num_ec > 0 && a.alpha_channel != b.alpha_channel) return false;
  }
  const uint32_t bits = JXLH_EC_ALPHA | JXLH_EC_ALPHA_ASSOCIATED;
  for (uint32_t i = 0; i < p.num_ec; i++)
    if ((p.ec_flags[i] & bits) != (q.ec_flags[i] & bits)) return false;
  return true;
}

// The rect-list tail (blend_rects_plan.h decides, this issues): the work list goes up on the stream from a pinned block
// of the ring, ONE launch rewrites every rect in a.out.  An empty plan enqueues nothing.
jxlh_status issue_blend_rects(jxlh_ctx* ctx, int nec, const BlendLaunch& a, const BlendRectsPlan& plan) {
  if (plan.work.empty()) return JXLH_OK;
  const uint32_t n = (uint32_t)plan.work.size();
  if (jxlh_status st = ensure(ctx, ctx->blend_rects_dev, n)) return st;
  Pinned<BlendRectWork>& host = ctx->blend_rects_host[ctx->blend_rects_next];
  Fence& copied = ctx->blend_rects_copied[ctx->blend_rects_next];
  ctx->blend_rects_next = (ctx->blend_rects_next + 1) % jxlh_ctx::kBlendRectsRing;
  HIPCHK(ctx, copied.sync());  // the block's previous list is on the device
  copied.clear();
  if (host.n < n) {
    HIPCHK(ctx, host.reset());
    HIPCHK(ctx, host.alloc(n + n / 2));
  }
  std::memcpy(host.p, plan.work.data(), n * sizeof(BlendRectWork));
  HIPCHK(ctx, hipMemcpyAsync(ctx->blend_rects_dev.p, host.p, n * sizeof(BlendRectWork), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, copied.record(ctx->stream));
  {
    ScopedKernelTimer t(ctx, "k_blend_rects");
    launch_blend_rects(ctx->stream, nec, a, ctx->blend_rects_dev.p, n, plan.groups);
  }
  HIPCHK(ctx, hipGetLastError());
  return JXLH_OK;
}

// jxlh_frame_blend (by_rects false: the whole image) and jxlh_frame_blend_rects (the list, onto the kept composition)
jxlh_status frame_blend(jxlh_ctx* ctx, const jxlh_blend_desc* d, const jxlh_output_desc* colour, bool by_rects,
                        const jxlh_rect* rects, uint32_t n_rects) {
  if (!ctx || !d) return JXLH_ERR_INVALID_ARGUMENT;
  if (comm_nranks(ctx) > 1) return JXLH_ERR_UNSUPPORTED;  // a rank holds only its band
  if (!ctx->in_frame || !ctx->frame.rendered || !ctx->frame.result[0]) return JXLH_ERR_BAD_STATE;
  if (jxlh_status st = check_desc(ctx, d)) return st;
  BlendLaunch a{};
  if (jxlh_status st = colour_stage(colour, &a.mode, &a.xyb, &a.tf)) return st;
  // the frame's own planes: the render's result, also when an earlier composition has taken its place
  const bool again = blended(ctx);
  float* fr[3];
  for (int c = 0; c < 3; c++) fr[c] = again ? ctx->frame.blend_frame[c] : ctx->frame.result[c];
  const int fw = again ? ctx->frame.blend_fw : ctx->res_w, fh = again ? ctx->frame.blend_fh : ctx->res_h;
  const size_t fstride = again ? ctx->frame.blend_fstride : ctx->res_stride;
  if (!sides_ok(d, (uint32_t)fw, (uint32_t)fh)) return JXLH_ERR_UNSUPPORTED;
  // the extra channels handed over: 0 .. nec - 1, converted, at the frame's size (as jxlh_frame_save_reference)
  uint32_t nec = 0;
  while (nec < JXLH_MAX_EXTRA_CHANNELS && ctx->extra[nec].set) nec++;
  for (uint32_t i = nec; i < JXLH_MAX_EXTRA_CHANNELS; i++)
    if (ctx->extra[i].set) return JXLH_ERR_UNSUPPORTED;
  if (d->num_ec != nec) return JXLH_ERR_INVALID_ARGUMENT;
  for (uint32_t i = 0; i < nec; i++) {
    const jxlh_ctx::ExtraChannel& e = ctx->extra[i];
    if (!e.done) return JXLH_ERR_BAD_STATE;
    if (e.out_w != (uint32_t)fw || e.out_h != (uint32_t)fh) return JXLH_ERR_UNSUPPORTED;
  }
  const size_t ostride = round_up(d->image_w, 64), plane = ostride * d->image_h;
  BlendRectsPlan plan;
  if (by_rects) {
    // the composition the rects are recomposed in: this frame's, of the same geometry, still in the canvas
    const FrameState& f = ctx->frame;
    if (!f.blend_kept || !ctx->blend_canvas.p) return JXLH_ERR_BAD_STATE;
    if (!same_composition(f.blend_kept_desc, *d) || f.blend_kept_mode != a.mode) return JXLH_ERR_INVALID_ARGUMENT;
    if (a.mode != kModeNone && (std::memcmp(&f.blend_kept_xyb, &a.xyb, sizeof(a.xyb)) != 0 ||
                                std::memcmp(&f.blend_kept_tf, &a.tf, sizeof(a.tf)) != 0))
      return JXLH_ERR_INVALID_ARGUMENT;
    if (f.blend_fw != fw || f.blend_fh != fh || f.blend_nec != nec || ctx->blend_canvas.n < plane * (3 + nec))
      return JXLH_ERR_BAD_STATE;  // (cannot happen inside one frame: the same descriptor met another result)
    if (jxlh_status st = check_blend_rects(rects, n_rects, d->image_w, d->image_h)) return st;
    plan = plan_blend_rects(rects, n_rects, d->image_w, d->image_h);
    if (plan.status != JXLH_OK) return plan.status;
  }
  // checked: from here on only the device can fail
  if (!again) materialise_chroma(ctx);
  fill_desc(ctx, d, a);
  a.fw = fw;
  a.fh = fh;
  for (int c = 0; c < 3; c++) {
    a.frame[c] = fr[c];
    a.frame_stride[c] = (uint32_t)fstride;
  }
  for (uint32_t i = 0; i < nec; i++) {
    const jxlh_ctx::ExtraChannel& e = ctx->extra[i];
    a.frame[3 + i] = e.pat_ready ? e.pat.p : e.up > 1 ? e.out.p : e.f32.p;
    a.frame_stride[3 + i] = (uint32_t)e.out_stride;
  }
  if (!by_rects && ctx->blend_canvas.n < plane * (3 + nec)) {  // the canvas is about to be replaced
    ctx->frame.blend_kept = false;
    if (again) {  // un-blend first
      for (int c = 0; c < 3; c++) ctx->frame.result[c] = fr[c];
      ctx->res_w = fw;
      ctx->res_h = fh;
      ctx->res_stride = fstride;
    }
  }
  if (!by_rects)
    if (jxlh_status st = ensure(ctx, ctx->blend_canvas, plane * (3 + nec))) return st;
  for (uint32_t c = 0; c < 3 + nec; c++) a.out[c] = ctx->blend_canvas.p + c * plane;
  a.out_stride = (uint32_t)ostride;
  if (by_rects) {
    if (jxlh_status st = issue_blend_rects(ctx, (int)nec, a, plan)) return st;
  } else {
    {
      ScopedKernelTimer t(ctx, "k_blend");
      launch_blend(ctx->stream, (int)nec, a);
    }
    HIPCHK(ctx, hipGetLastError());
  }
  for (int c = 0; c < 3; c++) {
    ctx->frame.blend_frame[c] = fr[c];
    ctx->frame.result[c] = a.out[c];
  }
  ctx->frame.blend_fw = fw;
  ctx->frame.blend_fh = fh;
  ctx->frame.blend_fstride = fstride;
  ctx->frame.blend_nec = nec;
  ctx->res_w = (int)d->image_w;
  ctx->res_h = (int)d->image_h;
  ctx->res_stride = ostride;
  if (!by_rects) {  // the record jxlh_frame_blend_rects asks for
    ctx->frame.blend_kept = true;
    ctx->frame.blend_kept_desc = *d;
    ctx->frame.blend_kept_mode = a.mode;
    ctx->frame.blend_kept_xyb = a.xyb;
    ctx->frame.blend_kept_tf = a.tf;
  }
  return JXLH_OK;
}

}  // namespace

}  // namespace jxlh_host

extern "C" {

jxlh_status jxlh_frame_blend(jxlh_ctx* ctx, const jxlh_blend_desc* d, const jxlh_output_desc* colour) {
  JXLH_ON_DEVICE(ctx);
  return frame_blend(ctx, d, colour, /*by_rects=*/false, nullptr, 0);
}

jxlh_status jxlh_frame_blend_rects(jxlh_ctx* ctx, const jxlh_blend_desc* d, const jxlh_output_desc* colour,
                                   const jxlh_rect* rects, uint32_t n) {
  JXLH_ON_DEVICE(ctx);
  return frame_blend(ctx, d, colour, /*by_rects=*/true, rects, n);
}

// pure host code (blend_rects_plan.h)
jxlh_status jxlh_blend_image_rects(const jxlh_blend_desc* d, uint32_t frame_w, uint32_t frame_h, const jxlh_rect* frame_rects,
                                   uint32_t n, jxlh_rect* image_rects, uint32_t cap, uint32_t* n_out) {
  if (!d || !n_out || (n && !frame_rects) || (cap && !image_rects)) return JXLH_ERR_INVALID_ARGUMENT;
  std::vector<jxlh_rect> need;
  map_blend_image_rects(d->x0, d->y0, d->image_w, d->image_h, frame_w, frame_h, frame_rects, n, need);
  *n_out = (uint32_t)need.size();
  if (need.size() > cap) return JXLH_ERR_INVALID_ARGUMENT;
  std::copy(need.begin(), need.end(), image_rects);
  return JXLH_OK;
}

jxlh_status jxlh_stage_blend(jxlh_ctx* ctx, const jxlh_blend_desc* d, const float* const frame[], uint32_t n_channels,
                             uint32_t w, uint32_t h, size_t stride, float* const out[], size_t out_stride) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !d || !frame || !out || w == 0 || h == 0 || stride < w) return JXLH_ERR_INVALID_ARGUMENT;
  if (jxlh_status st = check_desc(ctx, d)) return st;
  if (n_channels != 3 + d->num_ec || out_stride < d->image_w) return JXLH_ERR_INVALID_ARGUMENT;
  for (uint32_t c = 0; c < n_channels; c++)
    if (!frame[c] || !out[c]) return JXLH_ERR_INVALID_ARGUMENT;
  if ((uint64_t)w * h >= (1ull << 31) || !sides_ok(d, w, h)) return JXLH_ERR_UNSUPPORTED;
  const size_t fplane = (size_t)w * h;
  const size_t ostride = round_up(d->image_w, 64), oplane = ostride * d->image_h;
  if (jxlh_status st = ensure(ctx, ctx->blend_hook_in, fplane * n_channels)) return st;
  if (jxlh_status st = ensure(ctx, ctx->blend_hook_out, oplane * n_channels)) return st;
  BlendLaunch a{};
  a.mode = kModeNone;
  fill_desc(ctx, d, a);
  a.fw = (int)w;
  a.fh = (int)h;
  a.out_stride = (uint32_t)ostride;
  for (uint32_t c = 0; c < n_channels; c++) {
    float* in = ctx->blend_hook_in.p + c * fplane;
    if (jxlh_status st = copy2d(ctx, in, (size_t)w * sizeof(float), frame[c], stride * sizeof(float),
                                (size_t)w * sizeof(float), h, ctx->stream))
      return st;
    a.frame[c] = in;
    a.frame_stride[c] = w;
    a.out[c] = ctx->blend_hook_out.p + c * oplane;
  }
  {
    ScopedKernelTimer t(ctx, "k_blend");
    launch_blend(ctx->stream, (int)d->num_ec, a);
  }
  HIPCHK(ctx, hipGetLastError());
  for (uint32_t c = 0; c < n_channels; c++)
    if (jxlh_status st = copy2d(ctx, out[c], out_stride * sizeof(float), a.out[c], ostride * sizeof(float),
                                (size_t)d->image_w * sizeof(float), d->image_h, ctx->stream))
      return st;
  JXLH_SYNC(ctx);
  return JXLH_OK;
}

jxlh_status jxlh_stage_blend_rects(jxlh_ctx* ctx, const jxlh_blend_desc* d, const float* const frame[], uint32_t n_channels,
                                   uint32_t w, uint32_t h, size_t stride, const jxlh_rect* rects, uint32_t n,
                                   float* const out[], size_t out_stride) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !d || !frame || !out || w == 0 || h == 0 || stride < w) return JXLH_ERR_INVALID_ARGUMENT;
  if (jxlh_status st = check_desc(ctx, d)) return st;
  if (n_channels != 3 + d->num_ec || out_stride < d->image_w) return JXLH_ERR_INVALID_ARGUMENT;
  for (uint32_t c = 0; c < n_channels; c++)
    if (!frame[c] || !out[c]) return JXLH_ERR_INVALID_ARGUMENT;
  if ((uint64_t)w * h >= (1ull << 31) || !sides_ok(d, w, h)) return JXLH_ERR_UNSUPPORTED;
  if (jxlh_status st = check_blend_rects(rects, n, d->image_w, d->image_h)) return st;
  const BlendRectsPlan plan = plan_blend_rects(rects, n, d->image_w, d->image_h);
  if (plan.status != JXLH_OK) return plan.status;
  if (plan.work.empty()) return JXLH_OK;  // nothing to rewrite: nothing enqueued
  // device planes whose rows a lane's 16-byte store can address are rewritten where they are; others are staged whole
  bool in_place = out_stride % 4 == 0 && out_stride <= 0xffffffffu;
  for (uint32_t c = 0; c < n_channels; c++)
    in_place = in_place && reinterpret_cast<uintptr_t>(out[c]) % 16 == 0 && is_device_ptr(out[c]);
  const size_t fplane = (size_t)w * h;
  const size_t ostride = round_up(d->image_w, 64), oplane = ostride * d->image_h;
  if (jxlh_status st = ensure(ctx, ctx->blend_hook_in, fplane * n_channels)) return st;
  if (!in_place)
    if (jxlh_status st = ensure(ctx, ctx->blend_hook_out, oplane * n_channels)) return st;
  BlendLaunch a{};
  a.mode = kModeNone;
  fill_desc(ctx, d, a);
  a.fw = (int)w;
  a.fh = (int)h;
  a.out_stride = (uint32_t)(in_place ? out_stride : ostride);
  for (uint32_t c = 0; c < n_channels; c++) {
    float* in = ctx->blend_hook_in.p + c * fplane;
    if (jxlh_status st = copy2d(ctx, in, (size_t)w * sizeof(float), frame[c], stride * sizeof(float),
                                (size_t)w * sizeof(float), h, ctx->stream))
      return st;
    a.frame[c] = in;
    a.frame_stride[c] = w;
    a.out[c] = in_place ? out[c] : ctx->blend_hook_out.p + c * oplane;
    if (!in_place)
      if (jxlh_status st = copy2d(ctx, a.out[c], ostride * sizeof(float), out[c], out_stride * sizeof(float),
                                  (size_t)d->image_w * sizeof(float), d->image_h, ctx->stream))
        return st;
  }
  if (jxlh_status st = issue_blend_rects(ctx, (int)d->num_ec, a, plan)) return st;
  if (!in_place)
    for (uint32_t c = 0; c < n_channels; c++)
      if (jxlh_status st = copy2d(ctx, out[c], out_stride * sizeof(float), a.out[c], ostride * sizeof(float),
                                  (size_t)d->image_w * sizeof(float), d->image_h, ctx->stream))
        return st;
  JXLH_SYNC(ctx);
  return JXLH_OK;
}

}  // extern "C"
