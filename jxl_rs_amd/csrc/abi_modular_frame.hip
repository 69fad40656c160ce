// C ABI, Modular frames (JXLH_FRAME_MODULAR): a lossless or lossy-Modular frame as a frame of the context.  The i32
// samples the inverse transforms left go in rect by rect (jxlh_frame_set_modular_channels); jxlh_frame_run takes a
// band of them into the frame layout (k_modular_intake: the conversion stages that open the reference's render list,
// frame/render.rs:554-563), and from there the frame is a VarDCT frame's: chroma upsampling, Gaborish / EPF with the
// constant sigma of features/epf.rs:81-84, run_post_stages, and every call that reads ctx->frame.result / ctx->extra.
#include <algorithm>

#include "jxlh_ctx.h"

namespace jxlh_host {

// jxlh_frame_begin's commit of a Modular frame, behind the plan, the per-frame state and the geometry (ctx->params,
// ctx->fd): the buffers at the plan's sizes
jxlh_status modular_frame_begin(jxlh_ctx* ctx, const FramePlan& pl) {
  FrameDev& f = ctx->fd;
  const jxlh_frame_params& p = ctx->params;
  jxlh_status st;
  for (int c = 0; c < 3; c++) {
    if ((st = ensure(ctx, ctx->planes[c], pl.planes_n)) != JXLH_OK) return st;
    if ((st = ensure(ctx, ctx->tmp[c], pl.tmp_n)) != JXLH_OK) return st;
    if ((st = ensure(ctx, ctx->mod_src[c], pl.mod_src_n)) != JXLH_OK) return st;
  }
  if ((st = ensure(ctx, ctx->sigma, pl.sigma_n)) != JXLH_OK) return st;
  if ((st = ensure(ctx, ctx->error_flag, 1)) != JXLH_OK) return st;
  HIPCHK(ctx, hipMemsetAsync(ctx->error_flag.p, 0, sizeof(int), ctx->stream));
  // rows never set read as zero samples
  for (int c = 0; c < 3; c++)
    HIPCHK(ctx, hipMemsetAsync(ctx->mod_src[c].p, 0, pl.mod_src_n * sizeof(int32_t), ctx->stream));
  for (int c = 0; c < 3; c++) {
    f.planes[c] = ctx->planes[c].p;
    f.tmp[c] = ctx->tmp[c].p;
  }
  f.inv_sigma = ctx->sigma.p;
  f.tiled = 0;
  set_filter_params(f, p);
  // SigmaSource::Constant (features/epf.rs:81-84): one value for every block, once per frame
  if (f.epf_iters > 0) launch_fill_f32(ctx->stream, ctx->sigma.p, pl.sigma_n, kInvSigmaNum / p.epf_sigma_for_modular);
  HIPCHK(ctx, hipGetLastError());
  return JXLH_OK;
}

// jxlh_frame_run of a Modular frame on 256-row bands [group_row0, group_row1) (clamped and checked by the caller)
jxlh_status modular_frame_run(jxlh_ctx* ctx, uint32_t group_row0, uint32_t group_row1) {
  if (jxlh_status st = patches_check_run(ctx)) return st;
  // (a band whose halo rows would undo the neighbouring band's finished rows is rendered whole: run_plan.h)
  const RunPlan plan = plan_run(run_inputs(ctx), (int)group_row0, (int)group_row1);
  return modular_frame_issue(ctx, plan, plan.y_lo, plan.y_hi, nullptr);
}

jxlh_status modular_frame_issue(jxlh_ctx* ctx, const RunPlan& plan, int y_lo, int y_hi, const PostRepaint* repaint) {
  FrameDev& f = ctx->fd;
  const jxlh_frame_params& p = ctx->params;
  f.tiled = plan.tiled ? 1 : 0;  // the intake writes raster planes
  ctx->frame.strip_ran = false;
  ctx->frame.chroma_lazy = plan.chroma_lazy;
  const int ya = plan.intake_y0, yb = plan.intake_y1;
  {
    IntakeLaunch a{};
    const uint32_t fmt = ctx->frame.mod_format ? ctx->frame.mod_format : 8u;  // (no rect was set: zero samples in any format)
    const uint32_t depth = fmt & 0xffffu;
    a.form = (fmt & JXLH_MODULAR_XYB) ? kIntakeXyb : (depth >> 8) ? kIntakeFloat : kIntakeInt;
    a.bits = depth & 0xffu;
    a.exp_bits = depth >> 8;
    a.src_stride = a.dst_stride = (uint32_t)f.plane_stride;
    for (int c = 0; c < 3; c++) {
      const int hs = f.hshift[c], vs = f.vshift[c];
      a.src[c] = ctx->mod_src[c].p;
      a.w[c] = (f.xsize + (1 << hs) - 1) >> hs;
      const int ch = (f.ysize + (1 << vs) - 1) >> vs;
      // a sub-sampled channel goes where K1 puts it: tmp[c], for run_chroma_upsample_rows; the vertical upsampling reads one
      // row of the channel beyond the rows it produces
      a.dst[c] = (hs | vs) ? f.tmp[c] : f.planes[c];
      a.y0[c] = vs ? std::max(0, (ya >> vs) - 1) : ya;
      a.y1[c] = vs ? std::min(ch, ((yb + 1) >> vs) + 1) : yb;
      a.scale[c] = a.form == kIntakeXyb ? p.lf_quant_factors[c] : 1.0f / (float)((1ull << a.bits) - 1);
    }
    ScopedKernelTimer t(ctx, "k_modular_intake");
    launch_modular_intake(ctx->stream, a);
  }
  if (f.subsampled) run_chroma_upsample_rows(ctx, ya, yb);  // frame/render.rs:569-576, in front of the filters
  if (plan.whole) ctx->frame.rendered = true;
  return run_stages_rows(ctx, plan.stages, y_lo, y_hi, plan.whole, repaint);
}

}  // namespace jxlh_host

extern "C" {

jxlh_status jxlh_frame_set_modular_channels(jxlh_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                            const int32_t* c0, const int32_t* c1, const int32_t* c2, size_t stride,
                                            uint32_t sample_format) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !c0 || !c1 || !c2 || stride < w) return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->in_frame || !ctx->modular) return JXLH_ERR_BAD_STATE;
  const FrameDev& f = ctx->fd;
  const bool xyb = (sample_format & JXLH_MODULAR_XYB) != 0;
  const uint32_t depth = sample_format & ~(uint32_t)JXLH_MODULAR_XYB;
  // (the XYB form does not read the bit depth: it may be left out)
  if (!(xyb && depth == 0) && !bit_depth_ok(depth, 31)) return JXLH_ERR_INVALID_ARGUMENT;
  if (xyb && f.subsampled) return JXLH_ERR_INVALID_ARGUMENT;
  if (ctx->frame.mod_format && ctx->frame.mod_format != sample_format) return JXLH_ERR_INVALID_ARGUMENT;
  if ((uint64_t)x0 + w > (uint64_t)f.xsize || (uint64_t)y0 + h > (uint64_t)f.ysize) return JXLH_ERR_INVALID_ARGUMENT;
  int maxhs = 0, maxvs = 0;
  for (int c = 0; c < 3; c++) {
    maxhs |= f.hshift[c];
    maxvs |= f.vshift[c];
  }
  if ((x0 & ((1u << maxhs) - 1)) || (y0 & ((1u << maxvs) - 1))) return JXLH_ERR_INVALID_ARGUMENT;
  if (w == 0 || h == 0) return JXLH_OK;
  const int32_t* src[3] = {c0, c1, c2};
  for (int c = 0; c < 3; c++) {
    const int hs = f.hshift[c], vs = f.vshift[c];
    const size_t cw = ((size_t)w + (1u << hs) - 1) >> hs, ch = ((size_t)h + (1u << vs) - 1) >> vs;
    int32_t* dst = ctx->mod_src[c].p + (size_t)(y0 >> vs) * f.plane_stride + (x0 >> hs);
    if (jxlh_status st = copy2d(ctx, dst, f.plane_stride * sizeof(int32_t), src[c], stride * sizeof(int32_t),
                                cw * sizeof(int32_t), ch, ctx->stream))
      return st;
  }
  JXLH_SYNC(ctx);  // like the other setters: the caller's buffers may be reused as soon as the call returns
  ctx->frame.mod_format = sample_format;
  return JXLH_OK;
}

}  // extern "C"
