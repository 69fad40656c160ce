// C ABI, extra channels by rect (include/jxl_hip_extra_rects.h): jxlh_frame_begin_extra_channel, the rect hand-over
// jxlh_frame_set_extra_channel_rects / _async and the host function jxlh_extra_channel_changed_rects.
// ec_rects_plan.h decides (checks, scatter layout, dirty tiles, the changed-rects rule), this issues: at most one
// copy of the host block's span and one k_ec_scatter launch per call.  The conversion of what became dirty belongs to
// the next run (run_extra_channel_rects, frame_run.hip).
#include "jxlh_ctx.h"

namespace jxlh_host {
namespace {

EcCallState ec_call_state(const jxlh_ctx* ctx) {
  EcCallState s;
  s.in_frame = ctx->in_frame;
  s.sharded = ctx->comm != nullptr;
  for (int i = 0; i < JXLH_MAX_EXTRA_CHANNELS; i++) {
    s.ch[i].set = ctx->extra[i].set;
    s.ch[i].w = ctx->extra[i].w;
    s.ch[i].h = ctx->extra[i].h;
  }
  return s;
}

jxlh_status set_rects(jxlh_ctx* ctx, const int32_t* samples, uint64_t n_samples, const jxlh_ec_rect* rects, uint32_t n,
                      uint32_t* first_bad, bool wait) {
  if (!ctx) return JXLH_ERR_INVALID_ARGUMENT;
  const EcCallState state = ec_call_state(ctx);
  std::string why;
  if (jxlh_status st = check_ec_rects(state, samples != nullptr, n_samples, rects, n, first_bad, &why)) {
    if (!why.empty()) ctx->last_error = "jxlh_frame_set_extra_channel_rects: " + why;
    return st;
  }
  const bool staged = n && !is_device_ptr(samples);
  EcScatterPlan plan = plan_ec_scatter(state, rects, n, staged, (uint64_t)reinterpret_cast<uintptr_t>(samples));
  if (plan.descs.empty()) return JXLH_OK;  // nothing to write: nothing enqueued
  const size_t nd = plan.descs.size();
  if (jxlh_status st = ensure(ctx, ctx->ec_scatter_dev, nd)) return st;
  const int32_t* src = samples;
  if (staged) {
    const size_t span = (size_t)(plan.span_hi - plan.span_lo);
    if (jxlh_status st = ensure(ctx, ctx->ec_block, span)) return st;
    src = ctx->ec_block.p;
  }
  HIPCHK(ctx, ctx->ec_scatter_copied.sync());  // the pinned block's previous list is on its way
  ctx->ec_scatter_copied.clear();
  if (ctx->ec_scatter_host.n < nd) {
    HIPCHK(ctx, ctx->ec_scatter_host.reset());
    HIPCHK(ctx, ctx->ec_scatter_host.alloc(nd + nd / 2));
  }
  // from here on the call happens: the channels' state first, so that a device error leaves them "not rendered"
  EcPlanes planes{};
  for (int i = 0; i < JXLH_MAX_EXTRA_CHANNELS; i++) planes.raw[i] = ctx->extra[i].raw.p;
  for (const EcScatterDesc& d : plan.descs) {
    jxlh_ctx::ExtraChannel& e = ctx->extra[d.ec];
    EcGrid& g = ctx->ec_plan.ch[d.ec];
    if (!e.rect) {  // a whole-plane channel takes rect state: what a run finished of it stays finished
      e.rect = true;
      g.reset(e.w, e.h, e.up);
      if (!e.done) g.mark_all();
    }
    const uint32_t y0 = (uint32_t)(d.dst_off / e.w), x0 = (uint32_t)(d.dst_off % e.w);
    g.mark(x0, y0, d.w, d.h);
    e.done = false;
  }
  if (staged)  // (the rects may leave gaps: the span is what ONE copy moves)
    HIPCHK(ctx, hipMemcpyAsync(ctx->ec_block.p, samples + plan.span_lo, (size_t)(plan.span_hi - plan.span_lo) * sizeof(int32_t),
                               hipMemcpyHostToDevice, ctx->stream));
  std::memcpy(ctx->ec_scatter_host.p, plan.descs.data(), nd * sizeof(EcScatterDesc));
  HIPCHK(ctx, hipMemcpyAsync(ctx->ec_scatter_dev.p, ctx->ec_scatter_host.p, nd * sizeof(EcScatterDesc), hipMemcpyHostToDevice,
                             ctx->stream));
  HIPCHK(ctx, ctx->ec_scatter_copied.record(ctx->stream));
  {
    ScopedKernelTimer t(ctx, "k_ec_scatter");
    launch_ec_scatter(ctx->stream, src, ctx->ec_scatter_dev.p, (uint32_t)nd, plan.pieces, planes);
  }
  HIPCHK(ctx, hipGetLastError());
  if (wait) JXLH_SYNC(ctx);  // the caller's block may be reused as soon as the call returns
  return JXLH_OK;
}

}  // namespace
}  // namespace jxlh_host

extern "C" {

jxlh_status jxlh_frame_begin_extra_channel(jxlh_ctx* ctx, uint32_t ec, uint32_t w, uint32_t h, uint32_t bits_per_sample,
                                           uint32_t ec_upsampling) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || ec >= JXLH_MAX_EXTRA_CHANNELS || w == 0 || h == 0 || !bit_depth_ok(bits_per_sample, 31) ||
      !ec_factor_ok(ec_upsampling))
    return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->in_frame) return JXLH_ERR_BAD_STATE;
  if ((uint64_t)w * h >= (1ull << 31) || ctx->comm) return JXLH_ERR_UNSUPPORTED;
  jxlh_ctx::ExtraChannel& e = ctx->extra[ec];
  if (e.set) return JXLH_ERR_BAD_STATE;  // begun or handed over whole in this frame already
  if (jxlh_status st = ensure(ctx, e.raw, (size_t)w * h)) return st;
  // samples never set read as zero, as the rows of a Modular frame do
  HIPCHK(ctx, hipMemsetAsync(e.raw.p, 0, (size_t)w * h * sizeof(int32_t), ctx->stream));
  e.w = w;
  e.h = h;
  e.bits = bits_per_sample;
  e.up = ec_upsampling;
  e.set = true;
  e.done = false;
  e.pat_ready = false;
  e.rect = true;
  ctx->ec_plan.ch[ec].reset(w, h, ec_upsampling);
  ctx->ec_plan.ch[ec].mark_all();
  return JXLH_OK;
}

jxlh_status jxlh_frame_set_extra_channel_rects(jxlh_ctx* ctx, const int32_t* samples, uint64_t n_samples,
                                               const jxlh_ec_rect* rects, uint32_t n, uint32_t* first_bad) {
  JXLH_ON_DEVICE(ctx);
  return set_rects(ctx, samples, n_samples, rects, n, first_bad, /*wait=*/true);
}

jxlh_status jxlh_frame_set_extra_channel_rects_async(jxlh_ctx* ctx, const int32_t* samples, uint64_t n_samples,
                                                     const jxlh_ec_rect* rects, uint32_t n, uint32_t* first_bad) {
  JXLH_ON_DEVICE(ctx);
  return set_rects(ctx, samples, n_samples, rects, n, first_bad, /*wait=*/false);
}

// pure host code (ec_rects_plan.h)
jxlh_status jxlh_extra_channel_changed_rects(uint32_t w, uint32_t h, uint32_t ec_upsampling, uint32_t res_w,
                                             uint32_t res_h, const jxlh_rect* src, uint32_t n_src, jxlh_rect* out,
                                             uint32_t cap, uint32_t* n) {
  if (!n || (n_src && !src) || (cap && !out)) return JXLH_ERR_INVALID_ARGUMENT;
  std::vector<jxlh_rect> need;
  if (jxlh_status st = plan_ec_changed_rects(w, h, ec_upsampling, res_w, res_h, src, n_src, need)) return st;
  *n = (uint32_t)need.size();
  if (need.size() > cap) return JXLH_ERR_INVALID_ARGUMENT;
  std::copy(need.begin(), need.end(), out);
  return JXLH_OK;
}

}  // extern "C"
