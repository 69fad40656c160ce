// C ABI of the splines stage: the frame's segments (bounds worked out and batches planned once per set call,
// splines_host.h), the stage hook, the host-only builder from the bitstream's form, and the piece of the frame pipeline
// that launches k_splines (run_post_stages, frame_run.hip).
#include <algorithm>

#include "../../include/jxl_hip_dev.h"
#include "jxlh_ctx.h"

namespace jxlh_host {

namespace {

// the batches of the current segments for a w x h plane
void plan(jxlh_ctx* ctx, int w, int h) {
  if (ctx->spline_plan_w == w && ctx->spline_plan_h == h && !ctx->spline_first.empty()) return;
  spline_plan_batches(ctx->spline_desc_host.data(), ctx->frame.spline_n, w, h, ctx->spline_budget, ctx->spline_first);
  ctx->spline_plan_w = w;
  ctx->spline_plan_h = h;
  ctx->frame.spline_resident = -1;
}

// batch b's bin list on the device.  A set that fits one batch keeps its list from call to call; with more batches each
// one is binned and uploaded when its turn comes, so the device never holds more than one batch's entries.
jxlh_status bins_on_device(jxlh_ctx* ctx, int b, int w, int h) {
  if (ctx->frame.spline_resident == b) return JXLH_OK;
  ctx->frame.spline_resident = -1;
  // (the list a queued launch reads is replaced in stream order; the host copy must outlive its upload)
  spline_build_bins(ctx->spline_desc_host.data(), ctx->spline_first[b], ctx->spline_first[b + 1], w, h, ctx->spline_bins);
  const std::vector<uint32_t>& words = ctx->spline_bins.words;
  if (jxlh_status st = ensure(ctx, ctx->spline_bins_dev, words.size())) return st;
  HIPCHK(ctx, hipMemcpyAsync(ctx->spline_bins_dev.p, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                             ctx->stream));
  JXLH_SYNC(ctx);
  ctx->frame.spline_resident = b;
  return JXLH_OK;
}

}  // namespace

jxlh_status run_splines(jxlh_ctx* ctx, float* const cur[3], size_t stride, int w, int h, int y_lo, int y_hi) {
  y_lo = std::max(0, y_lo);
  y_hi = std::min(h, y_hi);
  if (ctx->frame.spline_n == 0 || y_lo >= y_hi) return JXLH_OK;
  plan(ctx, w, h);
  SplineLaunch a{};
  for (int c = 0; c < 3; c++) a.col[c] = cur[c];
  a.stride = stride;
  a.w = w;
  a.h = h;
  a.y0 = y_lo;
  a.y1 = y_hi;
  const int nb = (int)ctx->spline_first.size() - 1;
  for (int b = 0; b < nb; b++) {
    if (jxlh_status st = bins_on_device(ctx, b, w, h)) return st;
    const SplineBins& bins = ctx->spline_bins;
    const uint32_t first = bins.row_first[y_lo / kSplineBinH], last = bins.row_first[(y_hi - 1) / kSplineBinH + 1];
    if (first >= last) continue;
    a.ntx = bins.ntx;
    a.bin0 = first;
    const uint32_t* words = ctx->spline_bins_dev.p;
    ScopedKernelTimer t(ctx, "k_splines");
    launch_splines(ctx->stream, a, last - first, words, words + bins.nbins, words + 2 * (size_t)bins.nbins + 1,
                   ctx->spline_desc.p);
  }
  HIPCHK(ctx, hipGetLastError());
  return JXLH_OK;
}

}  // namespace jxlh_host

extern "C" {

jxlh_status jxlh_frame_set_splines(jxlh_ctx* ctx, const jxlh_spline_segment* segments, uint32_t n) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx) return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->in_frame) return JXLH_ERR_BAD_STATE;
  if (n > 0 && !segments) return JXLH_ERR_INVALID_ARGUMENT;
  ctx->frame.spline_n = 0;
  ctx->spline_first.clear();
  ctx->frame.spline_resident = -1;
  ctx->spline_desc_host.resize(n);
  if (n == 0) return JXLH_OK;
  for (uint32_t i = 0; i < n; i++) ctx->spline_desc_host[i] = spline_dev(segments[i]);
  if (jxlh_status st = ensure(ctx, ctx->spline_desc, n)) return st;
  HIPCHK(ctx, hipMemcpyAsync(ctx->spline_desc.p, ctx->spline_desc_host.data(), n * sizeof(SplineDev),
                             hipMemcpyHostToDevice, ctx->stream));
  JXLH_SYNC(ctx);
  ctx->frame.spline_n = n;
  // binned once per set call for the frame's size (a set of several batches: their ranges; the lists follow per draw)
  plan(ctx, ctx->fd.xsize, ctx->fd.ysize);
  if (ctx->spline_first.size() == 2) return bins_on_device(ctx, 0, ctx->fd.xsize, ctx->fd.ysize);
  return JXLH_OK;
}

jxlh_status jxlh_stage_splines(jxlh_ctx* ctx, float* const planes[3], uint32_t w, uint32_t h, size_t stride) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !planes || w == 0 || h == 0 || stride < w) return JXLH_ERR_INVALID_ARGUMENT;
  for (int c = 0; c < 3; c++)
    if (!planes[c]) return JXLH_ERR_INVALID_ARGUMENT;
  if ((uint64_t)stride * h >= (1ull << 31) || w >= kSplineMaxAxis || h >= kSplineMaxAxis) return JXLH_ERR_UNSUPPORTED;
  if (ctx->frame.spline_n == 0) return JXLH_OK;
  // the rows' first w values travel; what lies beyond them is neither read nor written
  const size_t dstride = round_up(w, 64), plane = dstride * h;
  if (jxlh_status st = ensure(ctx, ctx->spline_hook, plane * 3)) return st;
  float* hp = ctx->spline_hook.p;
  for (int c = 0; c < 3; c++)
    if (jxlh_status st = copy2d(ctx, hp + c * plane, dstride * sizeof(float), planes[c], stride * sizeof(float),
                                (size_t)w * sizeof(float), h, ctx->stream))
      return st;
  float* cur[3] = {hp, hp + plane, hp + 2 * plane};
  if (jxlh_status st = run_splines(ctx, cur, dstride, (int)w, (int)h, 0, (int)h)) return st;
  for (int c = 0; c < 3; c++)
    if (jxlh_status st = copy2d(ctx, planes[c], stride * sizeof(float), hp + c * plane, dstride * sizeof(float),
                                (size_t)w * sizeof(float), h, ctx->stream))
      return st;
  JXLH_SYNC(ctx);
  return JXLH_OK;
}

jxlh_status jxlh_splines_build_segments(const jxlh_quantized_spline* splines, uint32_t n,
                                        int32_t quantization_adjustment, float y_to_x_lf, float y_to_b_lf,
                                        uint64_t image_xsize, uint64_t image_ysize, uint32_t high_precision,
                                        jxlh_spline_segment* out, size_t capacity, size_t* count) {
  if (!count || (n > 0 && !splines)) return JXLH_ERR_INVALID_ARGUMENT;
  std::vector<jxlh_spline_segment> seg;
  try {
    if (!spline_build_segments(splines, n, quantization_adjustment, y_to_x_lf, y_to_b_lf, image_xsize, image_ysize,
                               high_precision != 0, seg))
      return JXLH_ERR_INVALID_ARGUMENT;
  } catch (const std::bad_alloc&) {
    return JXLH_ERR_OUT_OF_MEMORY;
  }
  *count = seg.size();
  if (!out) return JXLH_OK;
  if (seg.size() > capacity) return JXLH_ERR_INVALID_ARGUMENT;
  if (!seg.empty()) memcpy(out, seg.data(), seg.size() * sizeof(jxlh_spline_segment));
  return JXLH_OK;
}

// dev hook (jxl_hip_dev.h)
jxlh_status jxlh_splines_set_batch_budget(jxlh_ctx* ctx, uint64_t entries) {
  if (!ctx) return JXLH_ERR_INVALID_ARGUMENT;
  ctx->spline_budget = entries ? entries : kSplineDefaultBudget;
  ctx->spline_first.clear();  // planned again by the next draw
  ctx->frame.spline_resident = -1;
  return JXLH_OK;
}

jxlh_status jxlh_splines_bin_layout(uint32_t* columns, uint32_t* rows) {
  if (!columns || !rows) return JXLH_ERR_INVALID_ARGUMENT;
  *columns = kSplineBinW;
  *rows = kSplineBinH;
  return JXLH_OK;
}

}  // extern "C"
