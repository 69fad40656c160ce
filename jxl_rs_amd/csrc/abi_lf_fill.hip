// C ABI, groups whose HF has not arrived (jxl_hip.h "GROUPS WITHOUT HF"): jxlh_frame_set_groups_lf_only marks them, and
// jxlh_frame_run / jxlh_frame_rerender_groups (frame_run.hip) hand a marked group to the fill kernel (k_lf_fill.hip)
// instead of the transforms -- upsample_lf_group of the reference (frame/decode.rs:51-158, taken at :744-752).  The marks
// live beside the coefficient epoch (CoeffEpoch::lf_only, under sp_mutex): a submission on any slot thread clears its
// group's mark where it records the submission.
#include <algorithm>

#include "jxlh_ctx.h"

namespace jxlh_host {

bool lf_only_snapshot(jxlh_ctx* ctx) {
  std::lock_guard<std::mutex> lock(ctx->sp_mutex);
  if (ctx->epoch.n_lf_only == 0) {
    ctx->lf_only_run.clear();
    return false;
  }
  ctx->lf_only_run = ctx->epoch.lf_only;
  return true;
}

jxlh_status lf_split_groups(jxlh_ctx* ctx, const std::vector<int>& groups, int* n_k1, int* n_fill) {
  std::vector<int>& up = ctx->lf_split_upload;
  const std::vector<uint8_t>& marks = ctx->lf_only_run;  // (empty: no group is marked)
  up.clear();
  for (int g : groups)
    if (marks.empty() || !marks[(size_t)g]) up.push_back(g);
  *n_k1 = (int)up.size();
  for (int g : groups)
    if (!marks.empty() && marks[(size_t)g]) up.push_back(g);
  *n_fill = (int)up.size() - *n_k1;
  if (up.empty()) return JXLH_OK;
  if (jxlh_status st = ensure(ctx, ctx->rerender_list, up.size())) return st;
  HIPCHK(ctx, hipMemcpyAsync(ctx->rerender_list.p, up.data(), up.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  return JXLH_OK;
}

jxlh_status run_lf_fill(jxlh_ctx* ctx, const FrameDev& f, const int* groups_dev, int n) {
  if (n <= 0) return JXLH_OK;
  // the frame's own factor (upsampling == 2 / 4) and an extra channel's select their kernels again before they use
  // them; whoever reads ctx->ups_kernels without selecting still finds what it left there
  float* const selected = ctx->ups_kernels.p;
  if (jxlh_status st = upload_upsampling_kernels(ctx, 8)) return st;
  const float* k8 = ctx->ups_kernels.p;
  ctx->ups_kernels.p = selected;
  ScopedKernelTimer t(ctx, "k_lf_fill");
  launch_lf_fill(ctx->stream, f, k8, groups_dev, n);
  return JXLH_OK;
}

}  // namespace jxlh_host

extern "C" {

jxlh_status jxlh_frame_set_groups_lf_only(jxlh_ctx* ctx, const uint32_t* group_ids, uint32_t count) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || (count && !group_ids)) return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->in_frame || ctx->modular) return JXLH_ERR_BAD_STATE;
  // (the reference's own fill of a sub-sampled frame sizes the LF rect with hshift where it means vshift,
  // frame/decode.rs:88-89: nothing sound to match; a rank of a sharded frame holds only its band of the planes)
  if (ctx->fd.subsampled || comm_nranks(ctx) > 1) return JXLH_ERR_UNSUPPORTED;
  for (uint32_t i = 0; i < count; i++)
    if (group_ids[i] >= ctx->ngroups) return JXLH_ERR_INVALID_ARGUMENT;
  if (count == 0) return JXLH_OK;
  std::lock_guard<std::mutex> lock(ctx->sp_mutex);
  for (uint32_t i = 0; i < count; i++) ctx->epoch.mark_lf_only(group_ids[i]);
  return JXLH_OK;
}

}  // extern "C"
