// C ABI of the MI355X JPEG XL reconstruction path (include/jxl_hip.h), a frame's opening and its inputs:
// jxlh_frame_begin (check, plan -- frame_plan.h --, commit), the dequantisation tables, the LF and HF-meta setters, the
// upsampling weights, the extra channels.  The context's own lifetime is abi_ctx.hip, the run frame_run.hip.
//
// Sequencing mirrors the reference's frame flow: decode_lf_group ->
// set_lf* / set_hf_meta; decode_hf_global -> set_dequant_tables; decode_hf_group ->
// submit_group (async H2D on the caller's slot stream, overlapping the host's entropy decode
// of the next group); finalize_lf + render -> frame_run.
#include <algorithm>

#include "jxlh_ctx.h"

namespace jxlh_host {
// the restoration filter's header fields in the form the kernels take them
void set_filter_params(FrameDev& f, const jxlh_frame_params& p) {
  for (int c = 0; c < 3; c++) {  // GaborishStage::new, gaborish.rs:20-27
    const float total = 1.0f + p.gab_w1[c] * 4.0f + p.gab_w2[c] * 4.0f;
    f.gab_k[c][0] = 1.0f / total;
    f.gab_k[c][1] = p.gab_w1[c] / total;
    f.gab_k[c][2] = p.gab_w2[c] / total;
    f.epf_channel_scale[c] = p.epf_channel_scale[c];
  }
  const float sigma_scale[3] = {p.epf_pass0_sigma_scale, 1.0f, p.epf_pass2_sigma_scale};  // render.rs:599-621
  for (int s = 0; s < 3; s++) {
    f.epf_sm[s] = sigma_scale[s] * 1.65f;  // epf1.rs:67-68
    f.epf_bsm[s] = f.epf_sm[s] * p.epf_border_sad_mul;
  }
  f.epf_iters = (int)p.epf_iters;
  f.gab = (int)p.gab;
}

// The per-frame state every jxlh_frame_begin starts from: FrameState's defaults, and the steps that are no plain value.
static void start_frame(jxlh_ctx* ctx) {
  ctx->frame = FrameState{};
  for (auto& e : ctx->extra) e.set = e.done = e.pat_ready = e.rect = false;
  for (auto& g : ctx->ec_plan.ch) g.clear();  // the rect state of the extra channels is per frame
  for (auto& s : ctx->slots) s.used = false;
  ctx->patch_desc_host.clear();  // the patch dictionary is per frame (the reference slots are not)
  ctx->spline_desc_host.clear();  // ... and so are the splines
  ctx->lf_only_run.clear();
  std::lock_guard<std::mutex> lock(ctx->sp_mutex);
  ctx->epoch.reset(ctx->ngroups);
  ctx->epoch.clear_lf_only();  // jxlh_frame_set_groups_lf_only: per-frame state
}

// jxlh_frame_begin behind the plan: the context takes the frame.  Buffers may have been replaced when it fails.
static jxlh_status commit_frame(jxlh_ctx* ctx, const jxlh_frame_params& p, const FramePlan& pl) {
  ctx->params = p;
  ctx->ngroups = pl.ngroups;
  ctx->modular = pl.modular;
  ctx->params_direct_ok = pl.params_direct_ok;
  start_frame(ctx);
  FrameDev& f = ctx->fd;
  std::memset(&f, 0, sizeof f);
  f.xsize = (int)p.xsize;
  f.ysize = (int)p.ysize;
  f.xblocks = pl.xblocks;
  f.yblocks = pl.yblocks;
  f.subsampled = pl.subsampled;
  for (int c = 0; c < 3; c++) {
    f.hshift[c] = pl.hshift[c];
    f.vshift[c] = pl.vshift[c];
  }
  f.xgroups = pl.xgroups;
  f.ygroups = pl.ygroups;
  f.cmap_stride = pl.cmap_stride;
  f.plane_stride = pl.plane_stride;
  f.scrap_off = pl.scrap_off;
  if (pl.modular) return modular_frame_begin(ctx, pl);  // no coefficient buffer, LF planes, HF-meta maps or work list
  jxlh_status st;
  // jxlh_ctx_tune_placement: the large buffers of a context that has none yet are picked from several candidate sets
  if (ctx->placement_trials > 1 && !ctx->planes[0].p && !ctx->tmp[0].p && !ctx->coeffs.p)
    if ((st = choose_placement(ctx, pl)) != JXLH_OK) return st;
  for (int c = 0; c < 3; c++) {
    if ((st = ensure(ctx, ctx->planes[c], pl.planes_n)) != JXLH_OK) return st;
    if ((st = ensure(ctx, ctx->tmp[c], pl.tmp_n)) != JXLH_OK) return st;
    if ((st = ensure(ctx, ctx->lf_raw[c], pl.lf_n)) != JXLH_OK) return st;
    if ((st = ensure(ctx, ctx->lf_sm[c], pl.lf_n)) != JXLH_OK) return st;
  }
  if ((st = ensure(ctx, ctx->sigma, pl.sigma_n)) != JXLH_OK) return st;
  if ((st = ensure(ctx, ctx->coeffs, pl.coeffs_n)) != JXLH_OK) return st;
  if ((st = ensure(ctx, ctx->raw_quant, pl.raw_quant_n)) != JXLH_OK) return st;
  if ((st = ensure(ctx, ctx->transform_map, pl.map_n)) != JXLH_OK) return st;
  if ((st = ensure(ctx, ctx->epf_map, pl.map_n)) != JXLH_OK) return st;
  if ((st = ensure(ctx, ctx->ytox, pl.cmap_n)) != JXLH_OK) return st;
  if ((st = ensure(ctx, ctx->ytob, pl.cmap_n)) != JXLH_OK) return st;
  if ((st = ensure(ctx, ctx->error_flag, 1)) != JXLH_OK) return st;
  {
    // a new allocation starts out as whatever the memory held, and a new layout puts the fallback flags on bytes of other
    // regions: either could equal a launch's epoch (launch_vardct_groups)
    const uint8_t* const wl_p = ctx->worklist.p;
    const size_t wl_n = ctx->worklist.n;
    if ((st = ensure(ctx, ctx->worklist, vardct_worklist_bytes(f))) != JXLH_OK) return st;
    if (ctx->worklist.p != wl_p || ctx->worklist.n != wl_n || ctx->worklist_nblocks != pl.nblocks) {
      vardct_worklist_clear_flags(ctx->stream, ctx->worklist.p, pl.nblocks);
      ctx->worklist_nblocks = pl.nblocks;
    }
  }
  vardct_worklist_reset(ctx->stream, ctx->worklist.p, &ctx->k1_launches);
  HIPCHK(ctx, hipMemsetAsync(ctx->error_flag.p, 0, sizeof(int), ctx->stream));
  // rects the caller never sets read as "not the first block of a varblock" (no work item, no stale map bytes of
  // an earlier frame reaching K1)
  HIPCHK(ctx, hipMemsetAsync(ctx->transform_map.p, 0, pl.map_n, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(ctx->raw_quant.p, 0, pl.raw_quant_n * sizeof(int32_t), ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(ctx->epf_map.p, 0, pl.map_n, ctx->stream));
  for (int c = 0; c < 3; c++) {
    f.planes[c] = ctx->planes[c].p;
    f.tmp[c] = ctx->tmp[c].p;
    f.lf[c] = ctx->lf_raw[c].p;
  }
  f.coeffs = ctx->coeffs.p;
  f.transform_map = ctx->transform_map.p;
  f.raw_quant = ctx->raw_quant.p;
  f.epf_map = ctx->epf_map.p;
  f.ytox = ctx->ytox.p;
  f.ytob = ctx->ytob.p;
  f.inv_sigma = ctx->sigma.p;
  f.inv_global_scale = pl.inv_global_scale;
  f.x_dm = pl.x_dm;
  f.b_dm = pl.b_dm;
  for (int i = 0; i < 4; i++) f.quant_biases[i] = p.quant_biases[i];
  f.color_factor = (float)p.color_factor;
  f.base_x = p.base_correlation_x;
  f.base_b = p.base_correlation_b;
  set_filter_params(f, p);
  // dequant tables persist across frames until replaced (library tables are per-decoder,
  // quant_weights.rs:356-374)
  ctx->tables_set = ctx->tables.p != nullptr && ctx->tables_set;
  if (ctx->tables_set) {
    f.tables = ctx->tables.p;
    f.tables_ok = ctx->tables_ok.p;
    for (int q = 0; q < JXLH_NUM_QUANT_TABLES; q++) f.table_offset[q] = ctx->table_offset[q];
  }
  f.se_direct_ok = ctx->params_direct_ok && ctx->tables_set && ctx->tables_ok_host != 0;
  return JXLH_OK;
}
}  // namespace jxlh_host

extern "C" {

// Check, plan, commit.  A begin the plan refuses leaves the context untouched: the previous frame stays complete and
// usable.  A commit that fails (an allocation, a HIP call) may already have replaced buffers: the context is then in no
// frame, and every frame call answers JXLH_ERR_BAD_STATE until a begin succeeds.
jxlh_status jxlh_frame_begin(jxlh_ctx* ctx, const jxlh_frame_params* p) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !p || p->abi_version != JXLH_ABI_VERSION) return JXLH_ERR_INVALID_ARGUMENT;
  static const bool no_direct_entries = [] {  // A/B runs of whole suites
    const char* e = getenv("JXLH_NO_DIRECT_ENTRIES");
    return e && *e && *e != '0';
  }();
  const FramePlan plan = plan_frame(*p, comm_nranks(ctx), no_direct_entries);
  if (plan.status != JXLH_OK) return plan.status;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const jxlh_status st = commit_frame(ctx, *p, plan);
  ctx->in_frame = st == JXLH_OK;
  return st;
}

jxlh_status jxlh_set_upsampling_weights(jxlh_ctx* ctx, const float* weights2, const float* weights4,
                                        const float* weights8) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx) return JXLH_ERR_INVALID_ARGUMENT;
  const float* src[3] = {weights2, weights4, weights8};
  const size_t cnt[3] = {15, 55, 210};
  for (int i = 0; i < 3; i++) {
    if (src[i]) ctx->ups_weights[i].assign(src[i], src[i] + cnt[i]);
    else ctx->ups_weights[i].clear();
    ctx->ups_valid[i] = false;
  }
  return JXLH_OK;
}

jxlh_status jxlh_frame_set_dequant_tables(jxlh_ctx* ctx, const float* const tables[JXLH_NUM_QUANT_TABLES],
                                          const size_t n[JXLH_NUM_QUANT_TABLES]) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !tables || !n) return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->in_frame) return JXLH_ERR_BAD_STATE;
  size_t total = 0;
  for (int q = 0; q < JXLH_NUM_QUANT_TABLES; q++) {
    if (!tables[q] || n[q] != (size_t)quant_table_size(q)) return JXLH_ERR_INVALID_ARGUMENT;
    total += 3 * n[q];
  }
  jxlh_status st = ensure(ctx, ctx->tables, total);
  if (st != JXLH_OK) return st;
  size_t off = 0;
  for (int q = 0; q < JXLH_NUM_QUANT_TABLES; q++) {
    ctx->fd.table_offset[q] = (int)off;
    ctx->table_offset[q] = (int)off;
    HIPCHK(ctx, hipMemcpyAsync(ctx->tables.p + off, tables[q], 3 * n[q] * sizeof(float), hipMemcpyDefault,
                               ctx->stream));
    off += 3 * n[q];
  }
  ctx->fd.tables = ctx->tables.p;
  if (jxlh_status st2 = ensure(ctx, ctx->tables_ok, 1)) return st2;
  launch_check_tables(ctx->stream, ctx->tables.p, total, ctx->tables_ok.p);
  ctx->fd.tables_ok = ctx->tables_ok.p;
  ctx->tables_ok_host = 0;
  HIPCHK(ctx, hipMemcpyAsync(&ctx->tables_ok_host, ctx->tables_ok.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ctx->tables_set = true;
  // like the other setters: the caller's buffers may be reused (or freed) as soon as the call returns
  JXLH_SYNC(ctx);
  ctx->fd.se_direct_ok = ctx->params_direct_ok && ctx->tables_ok_host != 0;
  return JXLH_OK;
}

static bool rect_ok(const jxlh_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h) {
  return (uint64_t)x0 + w <= (uint64_t)ctx->fd.xblocks && (uint64_t)y0 + h <= (uint64_t)ctx->fd.yblocks;
}

jxlh_status jxlh_frame_set_lf_quantized(jxlh_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                        const int32_t* qy, const int32_t* qx, const int32_t* qb, size_t stride,
                                        uint32_t extra_precision) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !qy || !qx || !qb || stride < w || extra_precision > 3) return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->in_frame || ctx->modular || ctx->frame.lf_from_slot) return JXLH_ERR_BAD_STATE;
  if (!rect_ok(ctx, x0, y0, w, h)) return JXLH_ERR_INVALID_ARGUMENT;
  if (w == 0 || h == 0) return JXLH_OK;
  ctx->frame.lf_from_caller = true;
  const size_t n = (size_t)w * h;
  jxlh_status st = ensure(ctx, ctx->lfq, 3 * n);
  if (st != JXLH_OK) return st;
  // the scratch is reused by the next call: order uploads and kernel on the main stream
  const int32_t* src[3] = {qy, qx, qb};
  for (int c = 0; c < 3; c++) {
    st = copy2d(ctx, ctx->lfq.p + c * n, w * sizeof(int32_t), src[c], stride * sizeof(int32_t), w * sizeof(int32_t), h,
                ctx->stream);
    if (st != JXLH_OK) return st;
  }
  const jxlh_frame_params& p = ctx->params;
  // dequant_lf, modular/mod.rs:849-879
  const float inv_quant_lf = (float)(1 << 16) / ((float)p.global_scale * (float)p.quant_lf);
  const float mul = 1.0f / (float)(1u << extra_precision);
  const float fac_x = (p.lf_quant_factors[0] * inv_quant_lf) * mul;
  const float fac_y = (p.lf_quant_factors[1] * inv_quant_lf) * mul;
  const float fac_b = (p.lf_quant_factors[2] * inv_quant_lf) * mul;
  const float cfl_x = p.base_correlation_x + (float)p.ytox_lf / (float)p.color_factor;
  const float cfl_b = p.base_correlation_b + (float)p.ytob_lf / (float)p.color_factor;
  const size_t off = (size_t)y0 * ctx->fd.xblocks + x0;
  {
    ScopedKernelTimer t(ctx, "k0a_dequant_lf");
    if (ctx->fd.subsampled)  // !is444(): no chroma-from-luma; the samples beyond (size >> shift) are don't-cares
      launch_dequant_lf_plain(ctx->stream, ctx->lfq.p, ctx->lfq.p + n, ctx->lfq.p + 2 * n, w, ctx->lf_raw[0].p + off,
                              ctx->lf_raw[1].p + off, ctx->lf_raw[2].p + off, ctx->fd.xblocks, (int)w, (int)h, fac_x,
                              fac_y, fac_b);
    else
      launch_dequant_lf(ctx->stream, ctx->lfq.p, ctx->lfq.p + n, ctx->lfq.p + 2 * n, w, ctx->lf_raw[0].p + off,
                        ctx->lf_raw[1].p + off, ctx->lf_raw[2].p + off, ctx->fd.xblocks, (int)w, (int)h, fac_x, fac_y,
                        fac_b, cfl_x, cfl_b);
  }
  HIPCHK(ctx, hipGetLastError());
  // the host buffers may be reused by the caller as soon as we return
  JXLH_SYNC(ctx);
  ctx->frame.lf_smoothed = false;
  return JXLH_OK;
}

jxlh_status jxlh_frame_set_lf(jxlh_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const float* x,
                              const float* y, const float* b, size_t stride) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !x || !y || !b || stride < w) return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->in_frame || ctx->modular || ctx->frame.lf_from_slot) return JXLH_ERR_BAD_STATE;
  if (!rect_ok(ctx, x0, y0, w, h)) return JXLH_ERR_INVALID_ARGUMENT;
  if (w == 0 || h == 0) return JXLH_OK;  // nothing written: the frame may still take a slot
  ctx->frame.lf_from_caller = true;
  const float* src[3] = {x, y, b};
  const size_t off = (size_t)y0 * ctx->fd.xblocks + x0;
  for (int c = 0; c < 3; c++) {
    jxlh_status st = copy2d(ctx, ctx->lf_raw[c].p + off, ctx->fd.xblocks * sizeof(float), src[c],
                            stride * sizeof(float), w * sizeof(float), h, ctx->stream);
    if (st != JXLH_OK) return st;
  }
  JXLH_SYNC(ctx);
  ctx->frame.lf_smoothed = false;
  return JXLH_OK;
}

jxlh_status jxlh_frame_set_hf_meta(jxlh_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                   const uint8_t* transform_map, const int32_t* raw_quant, const uint8_t* epf_map,
                                   size_t map_stride, const int8_t* ytox, const int8_t* ytob, size_t cmap_stride) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !transform_map || !raw_quant || !epf_map || !ytox || !ytob || map_stride < w)
    return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->in_frame || ctx->modular) return JXLH_ERR_BAD_STATE;
  if (!rect_ok(ctx, x0, y0, w, h) || (x0 % 8) || (y0 % 8)) return JXLH_ERR_INVALID_ARGUMENT;
  const size_t cw = (w + 7) / 8, ch = (h + 7) / 8;
  if (cmap_stride < cw) return JXLH_ERR_INVALID_ARGUMENT;
  const size_t off = (size_t)y0 * ctx->fd.xblocks + x0;
  const size_t coff = (size_t)(y0 / 8) * ctx->fd.cmap_stride + x0 / 8;
  // which of the rarely used transform families the frame holds at all (their kernels are not even launched for a
  // frame without them: four empty launches cost ~20 us of a 0.45 ms K1).  A map that arrives in device memory is not
  // inspected: both families are then assumed present.
  if (is_device_ptr(transform_map)) {
    ctx->frame.strip_all_closed = false;
  } else if (ctx->frame.strip_all_closed) {
    // is every varblock a DCT with sides <= 32 inside one 32x32 quadrant of its 64x64 tile?  (rects start on tile
    // boundaries: x0, y0 % 8 == 0)
    bool closed = true;
    for (uint32_t y = 0; y < h && closed; y++) {
      const uint8_t* row = transform_map + (size_t)y * map_stride;
      for (uint32_t x = 0; x < w; x++) {
        if (row[x] < 128) continue;
        const int t = row[x] & 127;
        if (t >= JXLH_NUM_TRANSFORMS || t == 1 || t == 2 || t == 3 || t >= 12 ||
            (x & 3) + (uint32_t)covered_x(t) > 4 || (y & 3) + (uint32_t)covered_y(t) > 4) {
          closed = false;
          break;
        }
      }
    }
    ctx->frame.strip_all_closed = closed;
  }
  if (is_device_ptr(transform_map)) {
    ctx->frame.has_special = ctx->frame.has_large = true;
  } else if (!(ctx->frame.has_special && ctx->frame.has_large)) {
    bool sp = false, lg = false;
    for (uint32_t y = 0; y < h; y++) {
      const uint8_t* row = transform_map + (size_t)y * map_stride;
      for (uint32_t x = 0; x < w; x++) {
        const uint8_t t = row[x] & 127;
        lg |= t >= 18;
        sp |= (t >= 1 && t <= 3) || (t >= 12 && t <= 17);
      }
    }
    ctx->frame.has_special |= sp;
    ctx->frame.has_large |= lg;
  }
  jxlh_status st;
  if ((st = copy2d(ctx, ctx->transform_map.p + off, ctx->fd.xblocks, transform_map, map_stride, w, h, ctx->stream)))
    return st;
  if ((st = copy2d(ctx, ctx->epf_map.p + off, ctx->fd.xblocks, epf_map, map_stride, w, h, ctx->stream))) return st;
  if ((st = copy2d(ctx, ctx->raw_quant.p + off, ctx->fd.xblocks * sizeof(int32_t), raw_quant,
                   map_stride * sizeof(int32_t), w * sizeof(int32_t), h, ctx->stream)))
    return st;
  if ((st = copy2d(ctx, ctx->ytox.p + coff, ctx->fd.cmap_stride, ytox, cmap_stride, cw, ch, ctx->stream))) return st;
  if ((st = copy2d(ctx, ctx->ytob.p + coff, ctx->fd.cmap_stride, ytob, cmap_stride, cw, ch, ctx->stream))) return st;
  JXLH_SYNC(ctx);
  return JXLH_OK;
}

}  // extern "C"

namespace jxlh_host {
namespace {
#include "upsampling_weights.inc"
// Upsample::new (render/stages/upsample.rs:31-66): the 15 / 55 / 210 weights are the upper triangle of the
// symmetric top-left quadrant of the (5n/2 x 2)^2 kernel image; expands to n*n kernels of 5x5 taps
void expand_upsampling_kernels(int n, const float* weights, float* flat) {
  const int half = n / 2, last = n - 1;
  for (int i = 0; i < 5 * half; i++) {
    for (int j = 0; j < 5 * half; j++) {
      const int y = std::min(i, j), x = std::max(i, j);
      const float wv = weights[5 * half * y - y * (y - 1) / 2 + x - y];
      const int oy = j / 5, ox = i / 5, ky = j % 5, kx = i % 5;
      flat[(oy * n + ox) * 25 + ky * 5 + kx] = wv;
      flat[((last - oy) * n + ox) * 25 + (4 - ky) * 5 + kx] = wv;
      flat[(oy * n + (last - ox)) * 25 + ky * 5 + (4 - kx)] = wv;
      flat[((last - oy) * n + (last - ox)) * 25 + (4 - ky) * 5 + (4 - kx)] = wv;
    }
  }
}
}  // namespace

jxlh_status upload_upsampling_kernels(jxlh_ctx* ctx, int n) {
  const int slot = n == 2 ? 0 : n == 4 ? 1 : 2;
  const float* dflt = n == 2 ? kDefaultUpsamplingWeights2 : n == 4 ? kDefaultUpsamplingWeights4 : kDefaultUpsamplingWeights8;
  if (!ctx->ups_valid[slot]) {
    const float* w = ctx->ups_weights[slot].empty() ? dflt : ctx->ups_weights[slot].data();
    std::vector<float> flat((size_t)n * n * 25);
    expand_upsampling_kernels(n, w, flat.data());
    if (jxlh_status st = ensure(ctx, ctx->ups_kernels_n[slot], flat.size())) return st;
    // pageable source: the copy is staged by the runtime before the call returns
    HIPCHK(ctx, hipMemcpyAsync(ctx->ups_kernels_n[slot].p, flat.data(), flat.size() * sizeof(float), hipMemcpyHostToDevice,
                               ctx->stream));
    JXLH_SYNC(ctx);
    ctx->ups_valid[slot] = true;
  }
  ctx->ups_kernels.p = ctx->ups_kernels_n[slot].p;  // one buffer per factor: an extra channel's factor may differ from the frame's
  return JXLH_OK;
}

}  // namespace jxlh_host

extern "C" {

jxlh_status jxlh_frame_set_extra_channel(jxlh_ctx* ctx, uint32_t ec, const int32_t* samples, size_t stride, uint32_t w,
                                         uint32_t h, uint32_t bits_per_sample, uint32_t ec_upsampling) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !samples || ec >= JXLH_MAX_EXTRA_CHANNELS || w == 0 || h == 0 || stride < w ||
      !bit_depth_ok(bits_per_sample, 31) ||
      (ec_upsampling != 1 && ec_upsampling != 2 && ec_upsampling != 4 && ec_upsampling != 8))
    return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->in_frame) return JXLH_ERR_BAD_STATE;
  if ((uint64_t)w * h >= (1ull << 31)) return JXLH_ERR_UNSUPPORTED;
  jxlh_ctx::ExtraChannel& e = ctx->extra[ec];
  if (jxlh_status st = ensure(ctx, e.raw, (size_t)w * h)) return st;
  if (jxlh_status st = copy2d(ctx, e.raw.p, (size_t)w * sizeof(int32_t), samples, stride * sizeof(int32_t),
                              (size_t)w * sizeof(int32_t), h, ctx->stream))
    return st;
  JXLH_SYNC(ctx);  // the caller's buffer may be reused as soon as the call returns
  e.w = w;
  e.h = h;
  e.bits = bits_per_sample;
  e.up = ec_upsampling;
  e.set = true;
  e.done = false;
  e.rect = false;  // a whole-plane channel (again): the next run converts all of it
  ctx->ec_plan.ch[ec].clear();
  return JXLH_OK;
}

jxlh_status jxlh_frame_read_extra_channel(jxlh_ctx* ctx, uint32_t ec, const jxlh_plane* out) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !out || ec >= JXLH_MAX_EXTRA_CHANNELS) return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->in_frame) return JXLH_ERR_BAD_STATE;
  const jxlh_ctx::ExtraChannel& e = ctx->extra[ec];
  if (!e.set || !e.done) return JXLH_ERR_BAD_STATE;  // handed over but no jxlh_frame_run since
  if (blended(ctx)) {  // the composed channel, image-sized (jxlh_frame_blend)
    if (ec >= ctx->frame.blend_nec) return JXLH_ERR_BAD_STATE;
    const size_t w = (size_t)ctx->res_w, h = (size_t)ctx->res_h;
    if (!out->ptr || out->bytes_per_row < w * sizeof(float) || out->num_rows < h ||
        out->bytes_between_rows < out->bytes_per_row)
      return JXLH_ERR_INVALID_ARGUMENT;
    if (jxlh_status st = copy2d(ctx, out->ptr, out->bytes_between_rows, ctx->blend_canvas.p + (3 + ec) * ctx->res_stride * h,
                                ctx->res_stride * sizeof(float), w * sizeof(float), h, ctx->stream))
      return st;
    return jxlh_ctx_sync(ctx);
  }
  if (!out->ptr || out->bytes_per_row < (size_t)e.out_w * sizeof(float) || out->num_rows < e.out_h ||
      out->bytes_between_rows < out->bytes_per_row)
    return JXLH_ERR_INVALID_ARGUMENT;
  const float* src = e.pat_ready ? e.pat.p : e.up > 1 ? e.out.p : e.f32.p;  // (with the frame's patches drawn in)
  if (jxlh_status st = copy2d(ctx, out->ptr, out->bytes_between_rows, src, e.out_stride * sizeof(float),
                              (size_t)e.out_w * sizeof(float), e.out_h, ctx->stream))
    return st;
  return jxlh_ctx_sync(ctx);
}

}  // extern "C"
