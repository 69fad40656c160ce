// C ABI of the MI355X JPEG XL reconstruction path (include/jxl_hip.h): context, device
// memory, streams, uploads and kernel sequencing.  No compute happens on the host here and
// there is no CPU fallback: every entry point either launches HIP kernels or fails.
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
}  // namespace jxlh_host

extern "C" {

uint32_t jxlh_abi_version(void) { return JXLH_ABI_VERSION; }
int32_t jxlh_covered_blocks_x(int32_t t) { return (t >= 0 && t < 27) ? covered_x(t) : -1; }
int32_t jxlh_covered_blocks_y(int32_t t) { return (t >= 0 && t < 27) ? covered_y(t) : -1; }
int32_t jxlh_quant_table_for_type(int32_t t) { return (t >= 0 && t < 27) ? quant_table_for_type(t) : -1; }
int32_t jxlh_quant_table_size(int32_t q) { return (q >= 0 && q < 17) ? quant_table_size(q) : -1; }

const char* jxlh_status_string(jxlh_status s) {
  switch (s) {
    case JXLH_OK: return "ok";
    case JXLH_ERR_INVALID_ARGUMENT: return "invalid argument";
    case JXLH_ERR_OUT_OF_MEMORY: return "out of device memory";
    case JXLH_ERR_DEVICE: return "HIP runtime error";
    case JXLH_ERR_BAD_STATE: return "call order violated";
    case JXLH_ERR_INVALID_TRANSFORM: return "invalid VarDCT transform id";
    case JXLH_ERR_UNSUPPORTED: return "unsupported on the device path";
    case JXLH_ERR_INVALID_BLOCK_SIZE: return "varblock larger than 8x8 in a chroma-subsampled frame";
    case JXLH_ERR_BLOCK_OUT_OF_BOUNDS: return "varblock crosses its group or the frame edge";
    default: return "unknown status";
  }
}

const char* jxlh_last_error(const jxlh_ctx* ctx) { return ctx ? ctx->last_error.c_str() : ""; }

jxlh_status jxlh_default_frame_params(jxlh_frame_params* p, uint32_t xsize, uint32_t ysize) {
  if (!p) return JXLH_ERR_INVALID_ARGUMENT;
  std::memset(p, 0, sizeof *p);
  p->abi_version = JXLH_ABI_VERSION;
  p->xsize = xsize;
  p->ysize = ysize;
  p->global_scale = 21845;  // not a header default; a typical d1 value
  p->quant_lf = 16;         // QuantizerParams::read default branch (quantizer.rs:67)
  p->lf_quant_factors[0] = 1.0f / 4096.0f;  // quant_weights.rs:24-30
  p->lf_quant_factors[1] = 1.0f / 512.0f;
  p->lf_quant_factors[2] = 1.0f / 256.0f;
  p->quant_biases[0] = 1.0f - 0.05465007330715401f;  // headers/transform_data.rs:30-31
  p->quant_biases[1] = 1.0f - 0.07005449891748593f;
  p->quant_biases[2] = 1.0f - 0.049935103337343655f;
  p->quant_biases[3] = 0.145f;
  p->x_qm_scale = 3;  // frame_header.rs:308-315
  p->b_qm_scale = 2;
  p->color_factor = 84;  // color_correlation_map.rs:18, :31-40
  p->base_correlation_x = 0.0f;
  p->base_correlation_b = 1.0f;
  p->gab = 1;  // frame_header.rs:150-177
  for (int c = 0; c < 3; c++) {
    p->gab_w1[c] = 0.115169525f;
    p->gab_w2[c] = 0.061248592f;
  }
  p->epf_iters = 2;
  for (int i = 0; i < 8; i++) p->epf_sharp_lut[i] = (float)i / 7.0f;
  p->epf_sharp_lut[7] = 1.0f;
  p->epf_channel_scale[0] = 40.0f;
  p->epf_channel_scale[1] = 5.0f;
  p->epf_channel_scale[2] = 3.5f;
  p->epf_quant_mul = 0.46f;
  p->epf_pass0_sigma_scale = 0.9f;
  p->epf_pass2_sigma_scale = 6.5f;
  p->epf_border_sad_mul = 2.0f / 3.0f;
  p->do_lf_smoothing = 1;
  p->epf_sigma_for_modular = 1.0f;  // RestorationFilter default (headers/frame_header.rs:229-231)
  return JXLH_OK;
}

jxlh_status jxlh_ctx_create(int32_t device_ordinal, int32_t n_slots, jxlh_ctx** out) {
  if (!out || n_slots < 1 || n_slots > 1024) return JXLH_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device_ordinal < 0 || device_ordinal >= ndev)
    return JXLH_ERR_DEVICE;
  jxlh_ctx* ctx = new (std::nothrow) jxlh_ctx();
  if (!ctx) return JXLH_ERR_OUT_OF_MEMORY;
  ctx->device = device_ordinal;
  // Stream priorities: all streams in the default class.  The runtime maps the streams of one class onto a handful of
  // hardware queues (GPU_MAX_HW_QUEUES, 4), least-used first, and two streams on one queue execute in order: with two
  // contexts of THREE slot streams each the two main streams land on one queue and the frames no longer overlap (8K d1,
  // two frames in flight: 0.74 ms per frame instead of 0.65-0.67; one or two slot streams per context do not collide).
  // Putting the main streams into the high class (or the slot streams) removes that collision (0.67) but makes the
  // PCIe-inclusive legs 1.2-1.7x SLOWER (the unpack kernels on the other class's queues are starved or pre-empt the
  // transforms): measured round 5, profiles/r05_a_stream_queues.txt.  JXLH_STREAM_PRIORITY="<main>,<slot>" selects other
  // classes for A/B runs (hipDeviceGetStreamPriorityRange: -1 high, 0 default, 1 low).
  static const struct Prio { int main_p, slot_p; } prio = [] {
    Prio p{0, 0};
    if (const char* e = getenv("JXLH_STREAM_PRIORITY")) (void)sscanf(e, "%d,%d", &p.main_p, &p.slot_p);
    return p;
  }();
  // JXLH_STREAM_CU_MASK="0x....,0x....,...": test hook -- the context's MAIN stream is created with that CU mask
  // (hipExtStreamCreateWithCUMask; 32 CUs per word): soaks of the dataflow squeeze launch run with fewer CU slots than
  // the launch has tickets, and with its workgroups confined to some XCDs
  std::vector<uint32_t> cu_mask;
  if (const char* e = getenv("JXLH_STREAM_CU_MASK")) {
    for (const char* q = e; *q;) {
      char* end = nullptr;
      cu_mask.push_back((uint32_t)strtoul(q, &end, 0));
      if (end == q) {
        cu_mask.clear();
        break;
      }
      q = *end == ',' ? end + 1 : end;
    }
  }
  if (hipSetDevice(device_ordinal) != hipSuccess ||
      ctx->stream.create(prio.main_p, cu_mask.data(), (uint32_t)cu_mask.size()) != hipSuccess ||
      ctx->t0.create(true) != hipSuccess || ctx->t1.create(true) != hipSuccess) {
    jxlh_ctx_destroy(ctx);
    return JXLH_ERR_DEVICE;
  }
  ctx->slots.resize(n_slots);
  for (auto& s : ctx->slots) {
    if (s.stream.create(prio.slot_p) != hipSuccess || s.done.create() != hipSuccess || s.copied.ev.create() != hipSuccess) {
      jxlh_ctx_destroy(ctx);
      return JXLH_ERR_DEVICE;
    }
  }
  *out = ctx;
  return JXLH_OK;
}

void jxlh_ctx_destroy(jxlh_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  drain_timers(ctx);
  comm_release(ctx);  // (talks to the peers: the one explicit step)
  delete ctx;  // every device resource goes with the member that owns it (device_owned.h)
}

jxlh_status jxlh_alloc_pinned(jxlh_ctx* ctx, size_t bytes, void** out) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !out) return JXLH_ERR_INVALID_ARGUMENT;
  HIPCHK(ctx, hipHostMalloc(out, bytes, hipHostMallocDefault));
  return JXLH_OK;
}

jxlh_status jxlh_free_pinned(jxlh_ctx* ctx, void* p) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx) return JXLH_ERR_INVALID_ARGUMENT;
  if (p) HIPCHK(ctx, hipHostFree(p));
  return JXLH_OK;
}

// Where the driver places a context's large buffers decides how fast the transforms and the filters run on them: the
// same kernels on the same data are up to 10 % apart between two contexts of one process, persistently, while copies
// between the buffers run alike (profiles/r06_q_context_placement.txt).  With jxlh_ctx_tune_placement(ctx, n) the first
// allocation of {three planes, three filter planes, coefficient buffer} becomes a pick among n candidate sets, rated by
// two byte movers with the streams of the 8x8 transform class and of the filters (k_probe.hip); the candidates are held
// until the pick (so that they ARE different placements), then all but the best are freed.  Setup cost: n x ~2.6 GB of
// transient device memory at 8192^2 and a few ms per candidate; a candidate that cannot be allocated ends the trials.
static jxlh_status choose_placement(jxlh_ctx* ctx, size_t plane_n, size_t tmp_n, size_t coeff_n, size_t probe_elems) {
  struct Cand {
    DevBuf<float> planes[3], tmp[3];
    DevBuf<int32_t> coeffs;
    float k1 = 0.f, filt = 0.f;
  };
  std::vector<Cand> cands;
  ctx->placement_report.clear();
  // `trials` candidates, and up to as many again while none of them stands out (the k1-like ratings of the two classes
  // are ~10 % apart and the slow one is ~6 % wide: a best one within 7 % of the worst means every candidate so far is slow)
  const int max_trials = std::min(64, 2 * ctx->placement_trials);
  for (int t = 0; t < max_trials; t++) {
    if (t >= ctx->placement_trials) {
      float lo = cands[0].k1, hi = cands[0].k1;
      for (const Cand& o : cands) lo = std::min(lo, o.k1), hi = std::max(hi, o.k1);
      if (lo <= 0.93f * hi) break;
    }
    Cand c;
    bool ok = true;
    for (int i = 0; i < 3 && ok; i++) {  // (the order of the plain path below)
      ok = c.planes[i].alloc(plane_n) == hipSuccess && c.tmp[i].alloc(tmp_n) == hipSuccess;
    }
    ok = ok && c.coeffs.alloc(coeff_n) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();  // out of memory: the candidates so far are the choice
      break;
    }
    float* const planes[3] = {c.planes[0].p, c.planes[1].p, c.planes[2].p};
    float* const tmp[3] = {c.tmp[0].p, c.tmp[1].p, c.tmp[2].p};
    if (jxlh_status st = probe_placement(ctx, c.coeffs.p, ctx->ngroups, planes, tmp, probe_elems & ~(size_t)511, &c.k1, &c.filt))
      return st;
    ctx->placement_report.push_back(c.k1);
    ctx->placement_report.push_back(c.filt);
    cands.push_back(std::move(c));
  }
  if (cands.empty()) return JXLH_OK;  // (the plain path reports the allocation failure)
  // the real K1 follows its mover closely (0.283 -> 0.351 ms, 0.303-0.311 -> 0.380-0.387), the filters theirs loosely
  // (slope ~0.3: profiles/r06_q_context_placement.txt): four parts k1-like to one part filter-like
  auto score = [](const Cand& c) { return 4.f * c.k1 + c.filt; };
  size_t best = 0;
  for (size_t i = 1; i < cands.size(); i++)
    if (score(cands[i]) < score(cands[best])) best = i;
  ctx->placement_pick = (int)best;
  for (int i = 0; i < 3; i++) {  // (the other candidates go with `cands`)
    ctx->planes[i] = std::move(cands[best].planes[i]);
    ctx->tmp[i] = std::move(cands[best].tmp[i]);
  }
  ctx->coeffs = std::move(cands[best].coeffs);
  return JXLH_OK;
}

jxlh_status jxlh_frame_begin(jxlh_ctx* ctx, const jxlh_frame_params* p) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !p || p->abi_version != JXLH_ABI_VERSION) return JXLH_ERR_INVALID_ARGUMENT;
  if (p->xsize == 0 || p->ysize == 0 || p->xsize > (1u << 20) || p->ysize > (1u << 20) || p->global_scale == 0 ||
      p->quant_lf == 0 || p->color_factor == 0 || p->epf_iters > 3)
    return JXLH_ERR_INVALID_ARGUMENT;
  // chroma subsampling (JPEG recompressions): jpeg_upsampling gives shifts of 0 or 1 per axis and channel,
  // relative to the most finely sampled channel (headers/frame_header.rs:252-253, :501-512)
  if (p->upsampling > 1 && p->upsampling != 2 && p->upsampling != 4 && p->upsampling != 8) return JXLH_ERR_INVALID_ARGUMENT;
  if (p->upsampling > 1) {  // FrameHeader::size() = ceil(size_upsampled / upsampling) (headers/frame_header.rs:555-561)
    const uint32_t n = p->upsampling;
    if (p->xsize_upsampled > p->xsize * n || p->ysize_upsampled > p->ysize * n ||
        (p->xsize_upsampled && (p->xsize_upsampled + n - 1) / n != p->xsize) ||
        (p->ysize_upsampled && (p->ysize_upsampled + n - 1) / n != p->ysize))
      return JXLH_ERR_INVALID_ARGUMENT;
  }
  uint32_t maxhs = 0, maxvs = 0;
  for (int c = 0; c < 3; c++) {
    if (p->hshift[c] > 1 || p->vshift[c] > 1) return JXLH_ERR_INVALID_ARGUMENT;
    maxhs |= p->hshift[c];
    maxvs |= p->vshift[c];
  }
  const bool modular = (p->flags & JXLH_FRAME_MODULAR) != 0;
  if (modular) {  // SigmaSource::Constant divides by it (features/epf.rs:81-84); a rank would hold only its band
    if (p->epf_iters > 0 && !(p->epf_sigma_for_modular > 0.0f)) return JXLH_ERR_INVALID_ARGUMENT;
    if (comm_nranks(ctx) > 1) return JXLH_ERR_UNSUPPORTED;
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  ctx->params = *p;
  FrameDev& f = ctx->fd;
  std::memset(&f, 0, sizeof f);
  f.xsize = (int)p->xsize;
  f.ysize = (int)p->ysize;
  // FrameHeader::size_blocks (headers/frame_header.rs:564-569): whole blocks of the coarsest channel
  f.xblocks = (int)(((p->xsize + (8u << maxhs) - 1) / (8u << maxhs)) << maxhs);
  f.yblocks = (int)(((p->ysize + (8u << maxvs) - 1) / (8u << maxvs)) << maxvs);
  f.subsampled = (maxhs | maxvs) != 0;
  for (int c = 0; c < 3; c++) {
    f.hshift[c] = (int)p->hshift[c];
    f.vshift[c] = (int)p->vshift[c];
  }
  f.xgroups = (int)((p->xsize + kGroupDim - 1) / kGroupDim);
  f.ygroups = (int)((p->ysize + kGroupDim - 1) / kGroupDim);
  f.cmap_stride = (f.xblocks + 7) / 8;
  f.plane_stride = round_up((size_t)f.xblocks * 8, 64);
  const size_t plane_elems = f.plane_stride * (size_t)f.yblocks * 8;
  // a sharded frame is all-gathered in place with equal counts per rank: room for nranks whole bands
  const size_t gather_elems = (size_t)comm_nranks(ctx) * comm_rows_per_rank(ctx, f.ygroups) * kGroupDim * f.plane_stride;
  // K1 uses 32-bit pixel and coefficient offsets
  // planes are addressed with 32-bit BYTE offsets in the filter kernels, coefficients with 32-bit indices
  // (a Modular frame has no coefficients)
  if (plane_elems >= (1ull << 30) || (!modular && (size_t)f.xgroups * f.ygroups * 3 * kGroupArea >= (1ull << 31)))
    return JXLH_ERR_UNSUPPORTED;
  ctx->ngroups = (size_t)f.xgroups * f.ygroups;
  {
    std::lock_guard<std::mutex> lock(ctx->sp_mutex);
    ctx->epoch.reset(ctx->ngroups);
    ctx->epoch.clear_lf_only();  // jxlh_frame_set_groups_lf_only: per-frame state
  }
  ctx->lf_only_run.clear();
  ctx->modular = modular;
  if (modular) return modular_frame_begin(ctx);  // no coefficient buffer, LF planes, HF-meta maps or work list
  const size_t nblocks = (size_t)f.xblocks * f.yblocks;
  const size_t ncmap = (size_t)f.cmap_stride * ((f.yblocks + 7) / 8);
  jxlh_status st;
  // jxlh_ctx_tune_placement: the large buffers of a context that has none yet are picked from several candidate sets
  if (ctx->placement_trials > 1 && !ctx->planes[0].p && !ctx->tmp[0].p && !ctx->coeffs.p)
    if ((st = choose_placement(ctx, std::max(plane_elems, gather_elems), std::max(plane_elems + 8 * f.plane_stride, gather_elems),
                               ctx->ngroups * 3 * kGroupArea, plane_elems)) != JXLH_OK)
      return st;
  for (int c = 0; c < 3; c++) {
    if ((st = ensure(ctx, ctx->planes[c], std::max(plane_elems, gather_elems))) != JXLH_OK) return st;
    // + one block row: the scrap tile K1 stores the blocks a sub-sampled channel does not hold into
    if ((st = ensure(ctx, ctx->tmp[c], std::max(plane_elems + 8 * f.plane_stride, gather_elems))) != JXLH_OK) return st;
    if ((st = ensure(ctx, ctx->lf_raw[c], nblocks)) != JXLH_OK) return st;
    if ((st = ensure(ctx, ctx->lf_sm[c], nblocks)) != JXLH_OK) return st;
  }
  if ((st = ensure(ctx, ctx->sigma, nblocks)) != JXLH_OK) return st;
  if ((st = ensure(ctx, ctx->coeffs, ctx->ngroups * 3 * kGroupArea)) != JXLH_OK) return st;
  if ((st = ensure(ctx, ctx->raw_quant, nblocks)) != JXLH_OK) return st;
  if ((st = ensure(ctx, ctx->transform_map, nblocks)) != JXLH_OK) return st;
  if ((st = ensure(ctx, ctx->epf_map, nblocks)) != JXLH_OK) return st;
  if ((st = ensure(ctx, ctx->ytox, ncmap)) != JXLH_OK) return st;
  if ((st = ensure(ctx, ctx->ytob, ncmap)) != JXLH_OK) return st;
  if ((st = ensure(ctx, ctx->error_flag, 1)) != JXLH_OK) return st;
  {
    // a new allocation starts out as whatever the memory held, and a new layout puts the fallback flags on bytes of other
    // regions: either could equal a launch's epoch (launch_vardct_groups)
    const uint8_t* const wl_p = ctx->worklist.p;
    const size_t wl_n = ctx->worklist.n;
    if ((st = ensure(ctx, ctx->worklist, vardct_worklist_bytes(f))) != JXLH_OK) return st;
    if (ctx->worklist.p != wl_p || ctx->worklist.n != wl_n || ctx->worklist_nblocks != nblocks) {
      vardct_worklist_clear_flags(ctx->stream, ctx->worklist.p, nblocks);
      ctx->worklist_nblocks = nblocks;
    }
  }
  vardct_worklist_reset(ctx->stream, ctx->worklist.p, &ctx->k1_launches);
  HIPCHK(ctx, hipMemsetAsync(ctx->error_flag.p, 0, sizeof(int), ctx->stream));
  // rects the caller never sets read as "not the first block of a varblock" (no work item, no stale map bytes of
  // an earlier frame reaching K1)
  HIPCHK(ctx, hipMemsetAsync(ctx->transform_map.p, 0, nblocks, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(ctx->raw_quant.p, 0, nblocks * sizeof(int32_t), ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(ctx->epf_map.p, 0, nblocks, ctx->stream));
  for (int c = 0; c < 3; c++) {
    f.planes[c] = ctx->planes[c].p;
    f.tmp[c] = ctx->tmp[c].p;
    f.lf[c] = ctx->lf_raw[c].p;
  }
  f.scrap_off = (int)plane_elems;
  f.coeffs = ctx->coeffs.p;
  f.transform_map = ctx->transform_map.p;
  f.raw_quant = ctx->raw_quant.p;
  f.epf_map = ctx->epf_map.p;
  f.ytox = ctx->ytox.p;
  f.ytob = ctx->ytob.p;
  f.inv_sigma = ctx->sigma.p;
  // scalars, evaluated like the reference does on the host
  f.inv_global_scale = (float)(1 << 16) / (float)p->global_scale;        // quantizer.rs:79-81
  f.x_dm = powf(1.0f / 1.25f, (float)p->x_qm_scale - 2.0f);              // group.rs:395
  f.b_dm = powf(1.0f / 1.25f, (float)p->b_qm_scale - 2.0f);              // group.rs:396
  for (int i = 0; i < 4; i++) f.quant_biases[i] = p->quant_biases[i];
  f.color_factor = (float)p->color_factor;
  f.base_x = p->base_correlation_x;
  f.base_b = p->base_correlation_b;
  set_filter_params(f, *p);
  ctx->in_frame = true;
  // dequant tables persist across frames until replaced (library tables are per-decoder,
  // quant_weights.rs:356-374)
  ctx->tables_set = ctx->tables.p != nullptr && ctx->tables_set;
  if (ctx->tables_set) {
    f.tables = ctx->tables.p;
    f.tables_ok = ctx->tables_ok.p;
    for (int q = 0; q < JXLH_NUM_QUANT_TABLES; q++) f.table_offset[q] = ctx->table_offset[q];
  }
  {
    auto fin = [](float v) { return v == v && v > -3.0e38f && v < 3.0e38f; };
    auto bias_ok = [](float v) { return v >= 1e-6f && v <= 1e6f; };
    f.se_direct_ok = bias_ok(p->quant_biases[0]) && bias_ok(p->quant_biases[1]) && bias_ok(p->quant_biases[2]) &&
                     fin(p->quant_biases[3]) && fin(f.base_x) && fin(f.base_b) && !(p->flags & JXLH_FRAME_DENSE_DEQUANT);
    // ... and the table adjust_quant_bias is read from must hold no zero (AdjTable::nofast; same IEEE operations here)
    for (int i = 2; i < 128 && f.se_direct_ok; i++)
      if ((float)i - p->quant_biases[3] / (float)i == 0.0f) f.se_direct_ok = 0;
    static const bool off = [] { const char* e = getenv("JXLH_NO_DIRECT_ENTRIES"); return e && *e && *e != '0'; }();
    if (off) f.se_direct_ok = 0;  // A/B runs of whole suites
    ctx->params_direct_ok = f.se_direct_ok != 0;
    f.se_direct_ok = ctx->params_direct_ok && ctx->tables_set && ctx->tables_ok_host != 0;
  }
  reset_frame_state(ctx);
  return JXLH_OK;
}

}  // extern "C"

namespace jxlh_host {
// the per-frame state every jxlh_frame_begin starts from
void reset_frame_state(jxlh_ctx* ctx) {
  ctx->lf_smoothed = false;
  ctx->lf_from_slot = ctx->lf_from_caller = false;
  ctx->rendered = false;
  ctx->has_special = ctx->has_large = false;
  ctx->strip_all_closed = true;
  ctx->strip_ran = false;
  for (auto& e : ctx->extra) e.set = e.done = e.pat_ready = false;
  // the patch dictionary is per frame (the reference slots are not)
  ctx->patch_n = ctx->patch_nec = 0;
  ctx->patch_slots_used = 0;
  ctx->patch_ec_stale = true;
  ctx->patch_desc_host.clear();
  ctx->spline_n = 0;  // ... and so are the splines
  ctx->spline_desc_host.clear();
  for (auto& s : ctx->slots) s.used = false;
  for (int c = 0; c < 3; c++) ctx->result[c] = nullptr;
  ctx->chroma_lazy = false;
}
}  // namespace jxlh_host

extern "C" {

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
  if (!ctx->in_frame || ctx->modular || ctx->lf_from_slot) return JXLH_ERR_BAD_STATE;
  if (!rect_ok(ctx, x0, y0, w, h)) return JXLH_ERR_INVALID_ARGUMENT;
  if (w == 0 || h == 0) return JXLH_OK;
  ctx->lf_from_caller = true;
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
  ctx->lf_smoothed = false;
  return JXLH_OK;
}

jxlh_status jxlh_frame_set_lf(jxlh_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const float* x,
                              const float* y, const float* b, size_t stride) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !x || !y || !b || stride < w) return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->in_frame || ctx->modular || ctx->lf_from_slot) return JXLH_ERR_BAD_STATE;
  if (!rect_ok(ctx, x0, y0, w, h)) return JXLH_ERR_INVALID_ARGUMENT;
  if (w == 0 || h == 0) return JXLH_OK;  // nothing written: the frame may still take a slot
  ctx->lf_from_caller = true;
  const float* src[3] = {x, y, b};
  const size_t off = (size_t)y0 * ctx->fd.xblocks + x0;
  for (int c = 0; c < 3; c++) {
    jxlh_status st = copy2d(ctx, ctx->lf_raw[c].p + off, ctx->fd.xblocks * sizeof(float), src[c],
                            stride * sizeof(float), w * sizeof(float), h, ctx->stream);
    if (st != JXLH_OK) return st;
  }
  JXLH_SYNC(ctx);
  ctx->lf_smoothed = false;
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
    ctx->strip_all_closed = false;
  } else if (ctx->strip_all_closed) {
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
    ctx->strip_all_closed = closed;
  }
  if (is_device_ptr(transform_map)) {
    ctx->has_special = ctx->has_large = true;
  } else if (!(ctx->has_special && ctx->has_large)) {
    bool sp = false, lg = false;
    for (uint32_t y = 0; y < h; y++) {
      const uint8_t* row = transform_map + (size_t)y * map_stride;
      for (uint32_t x = 0; x < w; x++) {
        const uint8_t t = row[x] & 127;
        lg |= t >= 18;
        sp |= (t >= 1 && t <= 3) || (t >= 12 && t <= 17);
      }
    }
    ctx->has_special |= sp;
    ctx->has_large |= lg;
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

jxlh_status ensure_jump_table(jxlh_ctx* ctx) {
  if (ctx->xs_jump.p) return JXLH_OK;
  static uint64_t table[16][128][2];
  static std::once_flag once;
  std::call_once(once, [] { xorshift_jump_table(table); });
  if (jxlh_status st = ensure(ctx, ctx->xs_jump, sizeof(table) / sizeof(uint64_t))) return st;
  HIPCHK(ctx, hipMemcpyAsync(ctx->xs_jump.p, table, sizeof(table), hipMemcpyHostToDevice, ctx->stream));
  JXLH_SYNC(ctx);
  return JXLH_OK;
}

bool noise_lut_is_zero(const float lut[8]) {
  for (int i = 0; i < 8; i++)
    if (lut[i] != 0.0f) return false;
  return true;
}

// chroma upsampling of the sub-sampled channels, tmp[c] -> planes[c], over the rows of the sub-sampled channels that
// cover pixel rows [y0, y1) (y0 even).  Over the rows K1 produced for group rows: the outermost rows of a halo group row
// read beyond the region, and nobody reads them.
void run_chroma_upsample_rows(jxlh_ctx* ctx, int y0, int y1) {
  const FrameDev& f = ctx->fd;
  ScopedKernelTimer t(ctx, "k_chroma_upsample");
  const PixLayout lay = pix_layout(f);
  for (int c = 0; c < 3; c++) {
    const int hs = f.hshift[c], vs = f.vshift[c];
    if (!(hs | vs)) continue;
    const int cw = (f.xsize + (1 << hs) - 1) >> hs, ch = (f.ysize + (1 << vs) - 1) >> vs;
    const int sy0 = y0 >> vs, sy1 = min(ch, (y1 + (1 << vs) - 1) >> vs);
    launch_chroma_upsample(ctx->stream, f.tmp[c], f.planes[c], lay, lay, hs, vs, cw, ch, sy0, sy1, f.xblocks * 8,
                           f.yblocks * 8);
  }
}

void materialise_chroma(jxlh_ctx* ctx) {
  if (!ctx->chroma_lazy) return;
  run_chroma_upsample_rows(ctx, ctx->lazy_gr0 * kGroupDim, ctx->lazy_gr1 * kGroupDim);
  ctx->chroma_lazy = false;
}

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

// The coefficient transport of an epoch: plans it (coeff_epoch.h), issues the plan's copies and launches on the main
// stream, moves the state on.  *sparse_k1: the transforms read a bucketed form instead of the dense slabs.
static jxlh_status apply_coeff_epoch(jxlh_ctx* ctx, bool want_strip, bool* sparse_k1) {
  std::lock_guard<std::mutex> lock(ctx->sp_mutex);
  CoeffEpoch& e = ctx->epoch;
  if (e.dirty) {
    static_assert(sizeof(WideValue) == sizeof(uint2) && kEpochGroupCoeffs == 3u * kGroupArea, "coeff_epoch.h");
    e.upload.swap(e.pending);  // the descriptors and the plan stay alive until the next run: the H2D copies read them
    e.wide_upload.swap(e.wide);
    e.pending.clear();
    e.wide.clear();
    const size_t n = ctx->ngroups, ng = e.upload.size(), nw = e.wide_upload.size();
    if (jxlh_status st = ensure(ctx, ctx->sp_groups_dev, ng)) return st;
    if (jxlh_status st = ensure(ctx, ctx->sp_wide_dev, nw)) return st;
    if (jxlh_status st = ensure(ctx, ctx->group_dense, n)) return st;
    e.plan = plan_coeff_epoch(e.inputs((ctx->params.flags & JXLH_FRAME_EXPAND_SPARSE) != 0, want_strip));
    const EpochPlan& pl = e.plan;
    const int live = ctx->se_live, pend = live ^ 1;
    if (pl.descs == Descs::kAll && ng)
      HIPCHK(ctx, hipMemcpyAsync(ctx->sp_groups_dev.p, e.upload.data(), ng * sizeof(SparseGroup), hipMemcpyHostToDevice,
                                 ctx->stream));
    if (nw)
      HIPCHK(ctx, hipMemcpyAsync(ctx->sp_wide_dev.p, e.wide_upload.data(), nw * sizeof(uint2), hipMemcpyHostToDevice,
                                 ctx->stream));
    if (!pl.rebuild.empty()) {
      HIPCHK(ctx, hipMemcpyAsync(ctx->group_dense.p, pl.rebuild.data(), n, hipMemcpyHostToDevice, ctx->stream));
      ScopedKernelTimer t(ctx, "k_expand_sparse");
      if (e.live.form == Resident::kEntries)
        launch_expand_entries(ctx->stream, ctx->coeffs.p, ctx->se_entries[live].p, ctx->se_counts[live].p,
                              ctx->se_runs[live].p, ctx->group_dense.p, (int)n);
      else
        launch_expand_sorted(ctx->stream, ctx->coeffs.p, ctx->sp_sorted.p, ctx->sp_slot_start.p, ctx->group_dense.p, (int)n);
    }
    if (!pl.widen.empty()) {
      if (jxlh_status st = ensure(ctx, ctx->bucketed_dev, n)) return st;
      HIPCHK(ctx, hipMemcpyAsync(ctx->bucketed_dev.p, pl.widen.data(), n, hipMemcpyHostToDevice, ctx->stream));
      ScopedKernelTimer t(ctx, "k_entries_to_pairs");
      launch_entries_to_pairs(ctx->stream, ctx->se_entries[pend].p, ctx->se_counts[pend].p, ctx->se_runs[pend].p,
                              ctx->bucketed_dev.p, (int)n, ctx->sp_pairs.p);
    }
    size_t n_expand = ng;
    if (pl.descs == Descs::kRouted) {
      if (jxlh_status st = ensure(ctx, ctx->route_dev, n)) return st;
      HIPCHK(ctx, hipMemcpyAsync(ctx->route_dev.p, pl.after.route.data(), n, hipMemcpyHostToDevice, ctx->stream));
      // only the routed groups that arrived as pairs / entries have anything to expand: their descriptors go to the
      // front of the list (a frame whose only routed group is a dense slab launches nothing here)
      n_expand = 0;
      for (size_t i = 0; i < ng; i++)
        if (pl.after.route[e.upload[i].group]) std::swap(e.upload[n_expand++], e.upload[i]);
      if (n_expand)
        HIPCHK(ctx, hipMemcpyAsync(ctx->sp_groups_dev.p, e.upload.data(), n_expand * sizeof(SparseGroup),
                                   hipMemcpyHostToDevice, ctx->stream));
    }
    if (pl.sort) {
      if (jxlh_status st = ensure(ctx, ctx->sp_sorted, n * kEpochGroupCoeffs)) return st;
      if (jxlh_status st = ensure(ctx, ctx->sp_slot_start, n * 3 * (size_t)kSlotTable)) return st;
      ScopedKernelTimer t(ctx, "k_sort_sparse");
      launch_sort_sparse(ctx->stream, ctx->sp_pairs.p, ctx->sp_groups_dev.p, (int)ng, ctx->sp_sorted.p, ctx->sp_slot_start.p);
    } else if (pl.descs != Descs::kNone && (n_expand || nw)) {
      // zero-fill + scatter of the pair words (their own, or the ones the widening made of their entries) + the wide
      // values into the slabs -- or, for an added pass, on top of what the slab holds
      ScopedKernelTimer t(ctx, "k_expand_sparse");
      launch_expand_sparse(ctx->stream, ctx->coeffs.p, ctx->sp_pairs.p, ctx->sp_groups_dev.p, (int)n_expand,
                           ctx->sp_wide_dev.p, (uint32_t)nw, nullptr);
    }
    if (pl.pending_read) {
      HIPCHK(ctx, ctx->se_read[pend].record(ctx->stream));
    }
    if (pl.trade_sets()) ctx->se_live = pend;  // the next epoch's uploads go to the set read two frames ago
    e.reset(n);
    e.live = pl.after;
    if (ctx->sp_expanded.ev) HIPCHK(ctx, ctx->sp_expanded.record(ctx->stream));  // the pair buffer has been consumed
  }
  *sparse_k1 = e.live.form != Resident::kDense;
  return JXLH_OK;
}

// the frame's stage list, and what a run's routing reads from the context (run_plan.h; takes the snapshot of the
// LF-only marks)
StageList stage_list(const jxlh_ctx* ctx) {
  return StageList{ctx->fd.gab != 0, ctx->fd.epf_iters, (ctx->params.flags & JXLH_FRAME_UNFUSED_FILTERS) != 0};
}
RunInputs run_inputs(jxlh_ctx* ctx) {
  const FrameDev& f = ctx->fd;
  const jxlh_frame_params& p = ctx->params;
  static const bool strip_forced = [] {  // JXLH_STRIP=1: every eligible frame, whatever its flags say (A/B runs of whole suites)
    const char* e = getenv("JXLH_STRIP");
    return e && *e && *e != '0';
  }();
  return RunInputs{stage_list(ctx), f.xgroups, f.ygroups, f.ysize, (int)p.upsampling, comm_nranks(ctx), f.subsampled != 0,
                   ctx->modular, p.noise && !noise_lut_is_zero(p.noise_lut), draws_in_place(ctx),
                   strip_forced || (p.flags & JXLH_FRAME_STRIP), lf_only_snapshot(ctx), ctx->rendered, ctx->strip_ran};
}

// everything before K1: upload fences, the coefficient transport, K0b, K3 sigma
jxlh_status run_prologue(jxlh_ctx* ctx, bool strip_candidate, bool tiled, bool* sparse_k1) {
  FrameDev& f = ctx->fd;
  const jxlh_frame_params& p = ctx->params;
  // coefficient uploads issued on slot streams must land before K1
  for (auto& s : ctx->slots) {
    if (s.used) HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, s.done, 0));
  }
  if (jxlh_status st = apply_coeff_epoch(ctx, strip_candidate, sparse_k1)) return st;
  // ---- K0b: Frame::finalize_lf (frame/mod.rs:360-378)
  // (adaptive_lf_smoothing.rs:51-53; an LF image taken from an LF frame is used as it is, frame_header.rs:496-500)
  const bool smooth = p.do_lf_smoothing && !ctx->lf_from_slot && f.xblocks > 2 && f.yblocks > 2;
  if (smooth) {
    {  // out of place (raw -> smoothed), so re-running a frame repeats the full work
      const float inv_quant_lf = f.inv_global_scale / (float)p.quant_lf;  // quantizer.rs:82-84
      const float lf_factors[3] = {inv_quant_lf * p.lf_quant_factors[0], inv_quant_lf * p.lf_quant_factors[1],
                                   inv_quant_lf * p.lf_quant_factors[2]};
      const float* in[3] = {ctx->lf_raw[0].p, ctx->lf_raw[1].p, ctx->lf_raw[2].p};
      float* out[3] = {ctx->lf_sm[0].p, ctx->lf_sm[1].p, ctx->lf_sm[2].p};
      ScopedKernelTimer t(ctx, "k0b_lf_smooth");
      launch_lf_smooth(ctx->stream, in, out, f.xblocks, f.yblocks, lf_factors);
      ctx->lf_smoothed = true;
    }
    for (int c = 0; c < 3; c++) f.lf[c] = ctx->lf_sm[c].p;
  } else {
    for (int c = 0; c < 3; c++) f.lf[c] = ctx->lf_raw[c].p;
  }
  // ---- K3 sigma: SigmaSource::new (features/epf.rs:35-87)
  if (f.epf_iters > 0) {
    ScopedKernelTimer t(ctx, "k3_sigma_map");
    launch_sigma_map(ctx->stream, f, p.epf_quant_mul, p.epf_sharp_lut);
  }
  f.tiled = tiled ? 1 : 0;
  return JXLH_OK;
}

// what the transforms read when the frame is resident in a bucketed sparse form: the slot-bucketed entries in place
// (se_*) or the sorted pair words (sp_sorted); all null = the dense slabs
static void set_sparse_view(jxlh_ctx* ctx, FrameDev& f, bool sparse_k1) {
  const CoeffEpoch& e = ctx->epoch;
  const bool ent = sparse_k1 && e.live.form == Resident::kEntries;
  f.sp_sorted = sparse_k1 && !ent ? ctx->sp_sorted.p : nullptr;
  f.sp_slot_start = sparse_k1 && !ent ? ctx->sp_slot_start.p : nullptr;
  f.se_entries = ent ? ctx->se_entries[ctx->se_live].p : nullptr;
  f.se_counts = ent ? ctx->se_counts[ctx->se_live].p : nullptr;
  f.se_runs = ent ? ctx->se_runs[ctx->se_live].p : nullptr;
  f.group_dense = sparse_k1 ? ctx->group_dense.p : nullptr;
  f.group_route = ent && e.live.n_route > 0 ? ctx->route_dev.p : nullptr;
  f.se_dense_hint = ent ? e.live.se_dense_hint : 0;
  f.k1_stats = ctx->timing ? 1 : 0;
}
// behind the transforms: the coefficient slabs are free again (dense resubmissions of the next frame wait for this,
// jxlh_submit_group), and so is the live set of the slot-bucketed form once it has become the pending one
static jxlh_status mark_coefficients_read(jxlh_ctx* ctx, bool sparse_k1) {
  HIPCHK(ctx, ctx->k1_done.record(ctx->stream));
  if (sparse_k1 && ctx->epoch.live.form == Resident::kEntries) HIPCHK(ctx, ctx->se_read[ctx->se_live].record(ctx->stream));
  return JXLH_OK;
}

// The transforms of group rows [gr0, gr1) or, `listed`, of the first n_k1 groups of rerender_list; the LF fill of the
// n_fill groups listed behind them (jxlh_frame_set_groups_lf_only; never a sub-sampled frame): it writes them into the
// same planes, their coefficient store is not read.
static jxlh_status run_transforms(jxlh_ctx* ctx, bool sparse_k1, int gr0, int gr1, bool listed, int n_k1, int n_fill) {
  FrameDev& f = ctx->fd;
  {
    ScopedKernelTimer t(ctx, "k1_vardct");
    set_sparse_view(ctx, f, sparse_k1);
    // (a whole-frame run rewrites every group's flag in k1_scan: no clearing launch then)
    if (sparse_k1 && (listed || !(gr0 == 0 && gr1 == f.ygroups)))
      HIPCHK(ctx, hipMemsetAsync(ctx->group_dense.p, 0, ctx->ngroups, ctx->stream));
    // a sub-sampled channel is reconstructed at its own resolution into tmp[c] ...
    FrameDev fk = f;
    for (int c = 0; c < 3; c++)
      if (f.hshift[c] | f.vshift[c]) fk.planes[c] = f.tmp[c];
    launch_vardct_groups(ctx->stream, fk, listed ? 0 : gr0, listed ? 0 : gr1, ctx->worklist.p, &ctx->k1_launches,
                         ctx->error_flag.p, sparse_k1 ? ctx->coeffs.p : nullptr, listed ? ctx->rerender_list.p : nullptr,
                         listed ? n_k1 : 0, ctx->has_special, ctx->has_large, sparse_k1 ? ctx->epoch.live.n_route : 0);
  }
  if (jxlh_status st = run_lf_fill(ctx, f, ctx->rerender_list.p + n_k1, n_fill)) return st;
  return mark_coefficients_read(ctx, sparse_k1);
}

// K1 for the plan's group rows (+ the chroma upsampling of a sub-sampled frame)
jxlh_status run_k1(jxlh_ctx* ctx, const RunPlan& plan) {
  const FrameDev& f = ctx->fd;
  const int gr0 = plan.k1_row0, gr1 = plan.k1_row1;
  // a run with marked groups: K1 runs on the band's other groups through its group list
  const bool lf_only = !ctx->lf_only_run.empty();
  int n_k1 = 0, n_fill = 0;
  if (lf_only) {
    std::vector<int> band;
    for (int g = gr0 * f.xgroups; g < gr1 * f.xgroups; g++) band.push_back(g);
    if (jxlh_status st = lf_split_groups(ctx, band, &n_k1, &n_fill)) return st;
  }
  if (jxlh_status st = run_transforms(ctx, plan.sparse_k1, gr0, gr1, lf_only, n_k1, n_fill)) return st;
  ctx->chroma_lazy = plan.chroma_lazy;
  if (f.subsampled) {
    // ... and brought to full resolution into planes[c] before any filter, or lazily (run_plan.h: band_plan)
    ctx->lazy_gr0 = gr0;
    ctx->lazy_gr1 = gr1;
    if (!plan.chroma_lazy) run_chroma_upsample_rows(ctx, gr0 * kGroupDim, gr1 * kGroupDim);
  }
  return JXLH_OK;
}

// transforms + stage list of the whole frame in the strip kernel; tiles it cannot take (k1_scan decides) go through
// K1's class kernels first
jxlh_status run_strip(jxlh_ctx* ctx) {
  FrameDev& f = ctx->fd;
  if (!ctx->cu_count) {
    hipDeviceProp_t prop;
    HIPCHK(ctx, hipGetDeviceProperties(&prop, ctx->device));
    ctx->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  const int strips = strip_strips(f), tile_rows = strip_tile_rows(f);
  // The strips of a band spin on their neighbours' progress flags: every workgroup of the launch must be resident.
  // The occupancy query says how many are (two per CU on MI355X: the 77 KB window); a frame wider than that in strips
  // cannot take this path at all (the grid used to assume two per CU).
  // (per context: contexts may sit on devices of different sizes; a failed query is asked again -- ADVICE r05)
  if (ctx->strip_resident <= 0) ctx->strip_resident = strip_resident_workgroups(ctx->cu_count);
  const int resident = ctx->strip_resident;
  if (resident < strips) return JXLH_ERR_UNSUPPORTED;  // (the caller falls back to the two-kernel path)
  // a band is at least 4 tile rows (two extra transforms per band and strip)
  int bands = std::min((2 * ctx->cu_count + strips / 2) / strips, resident / strips);
  bands = std::max(1, std::min(bands, std::max(1, tile_rows / 4)));
  static const int forced_bands = [] {
    const char* e = getenv("JXLH_STRIP_BANDS");
    return e ? atoi(e) : 0;
  }();
  if (forced_bands > 0) bands = std::min(std::min(forced_bands, tile_rows), std::max(1, resident / strips));
  const size_t nblocks = (size_t)f.xblocks * f.yblocks;
  const bool fresh = ctx->strip_desc.n < nblocks;
  if (jxlh_status st = ensure(ctx, ctx->strip_desc, nblocks)) return st;
  if (jxlh_status st = ensure(ctx, ctx->strip_mode, (size_t)strips * tile_rows)) return st;
  if (jxlh_status st = ensure(ctx, ctx->strip_xchg, strip_xchg_floats(f))) return st;
  if (jxlh_status st = ensure(ctx, ctx->strip_flags, strip_flag_ints(f, bands))) return st;
  // blocks no varblock covers (rects never set, broken maps) keep an invalid descriptor
  if (fresh) HIPCHK(ctx, hipMemsetAsync(ctx->strip_desc.p, 0, nblocks * sizeof(uint2), ctx->stream));
  f.strip_desc = ctx->strip_desc.p;
  f.strip_mode = ctx->strip_mode.p;
  f.strip_flags = ctx->strip_flags.p;
  f.strip_nflags = (int)strip_flag_ints(f, bands);
  f.strips = strips;
  f.tile_rows = tile_rows;
  f.strip_all_closed = ctx->strip_all_closed ? 1 : 0;
  f.tiled = 1;
  set_sparse_view(ctx, f, false);
  {
    ScopedKernelTimer t(ctx, "k1_vardct");
    launch_vardct_groups(ctx->stream, f, 0, f.ygroups, ctx->worklist.p, &ctx->k1_launches, ctx->error_flag.p, nullptr,
                         nullptr, 0, ctx->has_special, ctx->has_large, 0);
  }
  {
    ScopedKernelTimer t(ctx, "k123_strip");
    static const float deadline_s = [] {
      const char* e = getenv("JXLH_STRIP_DEADLINE_S");
      return e ? (float)atof(e) : 4.0f;
    }();
    if (!launch_strip(ctx->stream, f, f.strip_desc, f.strip_mode, ctx->strip_xchg.p, ctx->strip_flags.p, bands,
                      ctx->error_flag.p, deadline_s)) {
      f.strip_desc = nullptr;
      f.strip_mode = nullptr;
      return JXLH_ERR_UNSUPPORTED;  // stage list not covered (run_plan.h: strip_eligible should have said so)
    }
  }
  f.strip_desc = nullptr;  // band runs / re-renders of this frame take the two-kernel path
  f.strip_mode = nullptr;
  if (jxlh_status st = mark_coefficients_read(ctx, false)) return st;
  ctx->chroma_lazy = false;
  ctx->rendered = true;
  ctx->strip_ran = true;
  // upsampling / noise behind the stage list: the strip kernel leaves the filtered planes in f.tmp
  return run_post_stages(ctx, f.tmp, 0, f.ysize, true);
}

// the stage list on pixel rows [y_lo, y_hi), then upsampling and noise
jxlh_status run_stages_rows(jxlh_ctx* ctx, const StageList& sl, int y_lo, int y_hi, bool whole_frame) {
  FrameDev& f = ctx->fd;
  // ---- stage list of frame/render.rs:569-622
  StageList::Stage stages[4];
  int ns = sl.sequence(stages);
  float* cur[3] = {f.planes[0], f.planes[1], f.planes[2]};
  float* oth[3] = {f.tmp[0], f.tmp[1], f.tmp[2]};
  if (sl.fused()) {
    // production path: the whole stage list in one pass over HBM (two for epf_iters == 3)
    ScopedKernelTimer t(ctx, "k23_fused_filters");
    (void)launch_fused_filters(ctx->stream, f, y_lo, y_hi);
    if (sl.result_in_tmp()) std::swap(cur, oth);
    ns = 0;
  }
  for (int s = 0; s < ns; s++) {
    const int later = sl.reach_after(s), kind = stages[s].kind;
    const int y0 = max(0, y_lo - later), y1 = min(f.ysize, y_hi + later);
    if (kind == StageList::kGaborish) {
      ScopedKernelTimer t(ctx, "k2_gaborish");
      for (int c = 0; c < 3; c++)
        launch_gaborish(ctx->stream, cur[c], oth[c], f.xsize, f.ysize, f.plane_stride, f.gab_k[c][0], f.gab_k[c][1],
                        f.gab_k[c][2], y0, y1);
    } else {
      EpfArgs a;
      for (int c = 0; c < 3; c++) {
        a.in[c] = cur[c];
        a.out[c] = oth[c];
        a.scale[c] = f.epf_channel_scale[c];
      }
      a.inv_sigma = f.inv_sigma;
      a.stride = f.plane_stride;
      a.sigma_stride = (size_t)f.xblocks;
      a.w = f.xsize;
      a.h = f.ysize;
      a.sm = f.epf_sm[kind];
      a.bsm = f.epf_bsm[kind];
      static const char* names[3] = {"k3a_epf0", "k3b_epf1", "k3c_epf2"};
      ScopedKernelTimer t(ctx, names[kind]);
      launch_epf(ctx->stream, kind, a, y0, y1);
    }
    std::swap(cur, oth);
  }
  return run_post_stages(ctx, cur, y_lo, y_hi, whole_frame);
}

// what follows the filters: patches, splines, upsampling and noise on the finished planes `cur` (rows [y_lo, y_hi))
jxlh_status run_post_stages(jxlh_ctx* ctx, float* const cur[3], int y_lo, int y_hi, bool whole_frame) {
  FrameDev& f = ctx->fd;
  const jxlh_frame_params& p = ctx->params;
  for (int c = 0; c < 3; c++) ctx->result[c] = cur[c];
  ctx->res_w = f.xsize;
  ctx->res_h = f.ysize;
  ctx->res_stride = f.plane_stride;
  bool extra_run = false;
  if (ctx->patch_n > 0) {
    // PatchesStage (frame/render.rs:644-650): after the extra channels' own upsampling, before the colour upsampling
    // and noise, at the coded size.  The extra channels must be converted before the patches read them.
    bool pending = whole_frame;
    for (uint32_t i = 0; i < ctx->patch_nec; i++) pending |= !ctx->extra[i].done;
    if (ctx->patch_nec > 0 && pending) {
      if (jxlh_status st = run_extra_channels(ctx)) return st;
      extra_run = true;
    }
    if (jxlh_status st = run_patches(ctx, cur, f.plane_stride, y_lo, y_hi)) return st;
  }
  // SplinesStage (frame/render.rs:652-653): behind patches, at the coded size
  if (ctx->spline_n > 0)
    if (jxlh_status st = run_splines(ctx, cur, f.plane_stride, f.xsize, f.ysize, y_lo, y_hi)) return st;
  if (p.upsampling > 1) {
    // Upsample2x/4x/8x on the three colour channels (frame/render.rs:655-671).  The 5x5 window crosses band
    // edges, so an upsampled frame is run whole.
    if (!whole_frame) return JXLH_ERR_UNSUPPORTED;
    const int n = (int)p.upsampling;
    const int ow = p.xsize_upsampled ? (int)p.xsize_upsampled : f.xsize * n;
    const int oh = p.ysize_upsampled ? (int)p.ysize_upsampled : f.ysize * n;
    const size_t ostride = round_up((size_t)f.xsize * n, 64);
    if (jxlh_status st = upload_upsampling_kernels(ctx, n)) return st;
    for (int c = 0; c < 3; c++)
      if (jxlh_status st = ensure(ctx, ctx->ups[c], ostride * (size_t)f.ysize * n)) return st;
    ScopedKernelTimer t(ctx, "k_upsample");
    for (int c = 0; c < 3; c++) {
      launch_upsample(ctx->stream, n, cur[c], f.plane_stride, f.xsize, f.ysize, ctx->ups_kernels.p, ctx->ups[c].p,
                      ostride, ow, oh);
      ctx->result[c] = ctx->ups[c].p;
    }
    ctx->res_w = ow;
    ctx->res_h = oh;
    ctx->res_stride = ostride;
  }
  if (p.noise && !noise_lut_is_zero(p.noise_lut)) {  // AddNoiseStage returns early on an all-zero LUT (noise.rs:153-155)
    // render_noise_for_group + ConvolveNoise x3 + AddNoise (frame/decode.rs:578-668, frame/render.rs:673-683),
    // at the resolution of the result (after upsampling).  Random planes: the 256-row tile rows that cover
    // the band plus the convolution's 2-row border.
    const int W = ctx->res_w, H = ctx->res_h;
    const int ya = p.upsampling > 1 ? 0 : y_lo, yb = p.upsampling > 1 ? H : y_hi;
    if (jxlh_status st = ensure_jump_table(ctx)) return st;
    for (int c = 0; c < 3; c++)
      if (jxlh_status st = ensure(ctx, ctx->noise[c], ctx->res_stride * (size_t)H)) return st;
    float* nz[3] = {ctx->noise[0].p, ctx->noise[1].p, ctx->noise[2].p};
    const int ty0 = max(0, ya - 2) / 256, ty1 = (min(H, yb + 2) + 255) / 256;
    {
      ScopedKernelTimer t(ctx, "k_noise_generate");
      launch_noise_generate(ctx->stream, nz, ctx->res_stride, W, H, ty0, ty1, p.visible_frame_index,
                            p.nonvisible_frame_index, ctx->xs_jump.p);
    }
    const float ytox = p.base_correlation_x + (float)p.ytox_lf / (float)p.color_factor;  // y_to_x_lf
    const float ytob = p.base_correlation_b + (float)p.ytob_lf / (float)p.color_factor;
    ScopedKernelTimer t(ctx, "k_noise_apply");
    launch_noise_apply(ctx->stream, nz, ctx->res_stride, ctx->result, ctx->res_stride, W, H, ya, yb, p.noise_lut, ytox,
                       ytob);
  }
  // (a partial re-render still picks up a channel that was handed over after the last whole-frame run)
  bool pending_extra = false;
  for (int i = 0; i < JXLH_MAX_EXTRA_CHANNELS; i++) pending_extra |= ctx->extra[i].set && !ctx->extra[i].done;
  if ((whole_frame || pending_extra) && !extra_run)
    if (jxlh_status st = run_extra_channels(ctx)) return st;
  HIPCHK(ctx, hipGetLastError());
  return JXLH_OK;
}

// channels 3.. of the reference's pipeline: ConvertModularToF32Stage, then Upsample<N> by the channel's own factor
// (frame/render.rs:564-567, :624-637 / :655-671)
jxlh_status run_extra_channels(jxlh_ctx* ctx) {
  for (int i = 0; i < JXLH_MAX_EXTRA_CHANNELS; i++) {
    jxlh_ctx::ExtraChannel& e = ctx->extra[i];
    if (!e.set) continue;
    const size_t n = (size_t)e.w * e.h;
    e.done = false;
    e.pat_ready = false;  // a new base: the patched copy is rebuilt by the next patches launch
    ctx->patch_ec_stale = true;
    if (jxlh_status st = ensure(ctx, e.f32, n)) return st;
    {
      ScopedKernelTimer t(ctx, "k_modular_to_f32");
      if (e.bits >> 8)  // floating-point samples (BitDepth::floating_point_sample, convert.rs:525-526)
        launch_float_samples_to_f32(ctx->stream, e.raw.p, n, e.bits & 0xffu, e.bits >> 8, e.f32.p);
      else
        launch_modular_to_f32(ctx->stream, e.raw.p, n, 1.0f / (float)((1ull << e.bits) - 1), e.f32.p);
    }
    // the frame's result size bounds the channel's (the padding of ceil(size / factor) * factor is cut off)
    const uint32_t full_w = (uint32_t)(ctx->res_w > 0 ? ctx->res_w : ctx->fd.xsize),
                   full_h = (uint32_t)(ctx->res_h > 0 ? ctx->res_h : ctx->fd.ysize);
    e.out_w = std::min(e.w * e.up, full_w);
    e.out_h = std::min(e.h * e.up, full_h);
    if (e.up > 1) {
      if (jxlh_status st = upload_upsampling_kernels(ctx, (int)e.up)) return st;
      e.out_stride = round_up((size_t)e.w * e.up, 64);
      if (jxlh_status st = ensure(ctx, e.out, e.out_stride * (size_t)e.h * e.up)) return st;
      ScopedKernelTimer t(ctx, "k_upsample");
      launch_upsample(ctx->stream, (int)e.up, e.f32.p, e.w, (int)e.w, (int)e.h, ctx->ups_kernels.p, e.out.p, e.out_stride,
                      (int)e.out_w, (int)e.out_h);
    } else {
      e.out_stride = e.w;
    }
    e.done = true;
  }
  return JXLH_OK;
}
}  // namespace jxlh_host

extern "C" {

jxlh_status jxlh_frame_run(jxlh_ctx* ctx, uint32_t group_row0, uint32_t group_row1) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx) return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->in_frame || (!ctx->modular && !ctx->tables_set)) return JXLH_ERR_BAD_STATE;
  group_row1 = std::min(group_row1, (uint32_t)ctx->fd.ygroups);
  if (group_row0 >= group_row1) return JXLH_ERR_INVALID_ARGUMENT;
  if (ctx->modular) return modular_frame_run(ctx, group_row0, group_row1);
  if (jxlh_status st = patches_check_run(ctx)) return st;
  RunPlan plan = plan_run(run_inputs(ctx), (int)group_row0, (int)group_row1);
  bool sparse_k1 = false;
  if (jxlh_status st = run_prologue(ctx, plan.strip_candidate, plan.tiled, &sparse_k1)) return st;
  plan = resolve_strip(plan, sparse_k1);
  ctx->strip_ran = false;
  if (plan.strip) {
    const jxlh_status st = run_strip(ctx);
    if (st != JXLH_ERR_UNSUPPORTED) return st;
    ctx->fd.strip_desc = nullptr;  // (nothing was launched) the two-kernel path takes the frame
    ctx->fd.strip_mode = nullptr;
  }
  if (jxlh_status st = run_k1(ctx, plan)) return st;
  if (plan.whole) ctx->rendered = true;
  return run_stages_rows(ctx, plan.stages, plan.y_lo, plan.y_hi, plan.whole);
}

jxlh_status jxlh_frame_rerender_groups(jxlh_ctx* ctx, const uint32_t* group_ids, uint32_t count) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || (count && !group_ids)) return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->in_frame) return JXLH_ERR_BAD_STATE;
  if (ctx->modular) return JXLH_ERR_UNSUPPORTED;  // a progressive Modular decode sets the changed rects and runs again
  if (!ctx->tables_set) return JXLH_ERR_BAD_STATE;
  for (uint32_t i = 0; i < count; i++)
    if (group_ids[i] >= ctx->ngroups) return JXLH_ERR_INVALID_ARGUMENT;
  if (count == 0) return JXLH_OK;
  if (jxlh_status st = patches_check_run(ctx)) return st;
  ctx->rerender_upload.assign(group_ids, group_ids + count);
  std::sort(ctx->rerender_upload.begin(), ctx->rerender_upload.end());
  ctx->rerender_upload.erase(std::unique(ctx->rerender_upload.begin(), ctx->rerender_upload.end()),
                             ctx->rerender_upload.end());
  const RunInputs in = run_inputs(ctx);
  const RerenderPlan plan = plan_rerender(in, ctx->rerender_upload);
  if (plan.route == RerenderPlan::kUnsupported) return JXLH_ERR_UNSUPPORTED;
  if (plan.route == RerenderPlan::kFullRun) return jxlh_frame_run(ctx, 0, UINT32_MAX);
  bool sparse_k1 = false;
  if (jxlh_status st = run_prologue(ctx, false, in.stages.fused(), &sparse_k1)) return st;
  // ---- transforms of exactly the listed groups
  // a listed group whose HF has not arrived (jxlh_frame_set_groups_lf_only) is filled from the LF image again, the
  // others are transformed: the list goes up with the transforms' groups first
  int n_k1 = 0, n_fill = 0;
  if (jxlh_status st = lf_split_groups(ctx, ctx->rerender_upload, &n_k1, &n_fill)) return st;
  if (jxlh_status st = run_transforms(ctx, sparse_k1, 0, 0, true, n_k1, n_fill)) return st;
  // ---- the filters on every pixel row the listed groups influence
  for (const RowBand& b : plan.bands)
    if (jxlh_status st = run_stages_rows(ctx, in.stages, b.y_lo, b.y_hi, b.whole_frame)) return st;
  return JXLH_OK;
}

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
  return JXLH_OK;
}

jxlh_status jxlh_frame_read_extra_channel(jxlh_ctx* ctx, uint32_t ec, const jxlh_plane* out) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !out || ec >= JXLH_MAX_EXTRA_CHANNELS) return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->in_frame) return JXLH_ERR_BAD_STATE;
  const jxlh_ctx::ExtraChannel& e = ctx->extra[ec];
  if (!e.set || !e.done) return JXLH_ERR_BAD_STATE;  // handed over but no jxlh_frame_run since
  if (blended(ctx)) {  // the composed channel, image-sized (jxlh_frame_blend)
    if (ec >= ctx->blend_nec) return JXLH_ERR_BAD_STATE;
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

// hand-over of caller-filled device buffers (jxl_hip.h "STREAM ORDERING OF DEVICE POINTERS"): every stream of the
// context -- the main one and the slot streams -- waits for the event
static jxlh_status all_streams_wait(jxlh_ctx* ctx, hipEvent_t e) {
  HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, e, 0));
  for (auto& s : ctx->slots) HIPCHK(ctx, hipStreamWaitEvent(s.stream, e, 0));
  return JXLH_OK;
}

jxlh_status jxlh_ctx_tune_placement(jxlh_ctx* ctx, int32_t trials, float* report, int32_t report_capacity, int32_t* n_report,
                                    int32_t* picked) {
  if (!ctx || trials < 0 || trials > 64 || (report_capacity > 0 && !report)) return JXLH_ERR_INVALID_ARGUMENT;
  if (trials > 0) ctx->placement_trials = trials;
  const int n = (int)ctx->placement_report.size();
  for (int i = 0; i < n && i < report_capacity; i++) report[i] = ctx->placement_report[(size_t)i];
  if (n_report) *n_report = n;
  if (picked) *picked = ctx->placement_pick;
  return JXLH_OK;
}

jxlh_status jxlh_ctx_wait_event(jxlh_ctx* ctx, void* hip_event) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !hip_event) return JXLH_ERR_INVALID_ARGUMENT;
  return all_streams_wait(ctx, static_cast<hipEvent_t>(hip_event));
}

jxlh_status jxlh_ctx_wait_stream(jxlh_ctx* ctx, void* hip_stream) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx) return JXLH_ERR_INVALID_ARGUMENT;
  HIPCHK(ctx, ctx->handover.create());
  // (an event may be re-recorded while earlier waits on it are still pending: a wait captures the record it follows)
  HIPCHK(ctx, hipEventRecord(ctx->handover, static_cast<hipStream_t>(hip_stream)));
  return all_streams_wait(ctx, ctx->handover);
}

jxlh_status jxlh_ctx_record_event(jxlh_ctx* ctx, void* hip_event) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !hip_event) return JXLH_ERR_INVALID_ARGUMENT;
  HIPCHK(ctx, hipEventRecord(static_cast<hipEvent_t>(hip_event), ctx->stream));
  return JXLH_OK;
}

// the dataflow squeeze launch's error word (pinned host memory the kernel writes): non-zero = a wait between two levels
// outlasted its deadline; reported once
static jxlh_status flow_error_status(jxlh_ctx* ctx) {
  if (!ctx->host_flow_flag.p) return JXLH_OK;
  const int v = *reinterpret_cast<volatile int*>(ctx->host_flow_flag.p);
  if (v == 0) return JXLH_OK;
  *ctx->host_flow_flag.p = 0;
  ctx->last_error = "jxlh_unsqueeze_chain: a wait between two levels of the dataflow launch outlasted its deadline";
  return (jxlh_status)v;
}

jxlh_status jxlh_ctx_mark(jxlh_ctx* ctx, uint32_t* mark) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !mark) return JXLH_ERR_INVALID_ARGUMENT;
  const uint32_t seq = ++ctx->mark_seq;
  Event& e = ctx->marks[seq % JXLH_MAX_MARKS];
  HIPCHK(ctx, e.create());
  HIPCHK(ctx, hipEventRecord(e, ctx->stream));
  *mark = seq;
  return JXLH_OK;
}

jxlh_status jxlh_ctx_wait_mark(jxlh_ctx* ctx, uint32_t mark) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || mark == 0 || (int32_t)(ctx->mark_seq - mark) < 0) return JXLH_ERR_INVALID_ARGUMENT;  // never handed out
  // (a mark older than the ring: its slot holds a later point of the stream -- waiting for that one is sufficient)
  hipEvent_t e = ctx->marks[mark % JXLH_MAX_MARKS];
  if (!e) return JXLH_ERR_BAD_STATE;
  HIPCHK(ctx, hipEventSynchronize(e));
  return flow_error_status(ctx);  // (a streaming caller that only ever waits for marks sees a dataflow fault too)
}

jxlh_status jxlh_ctx_sync(jxlh_ctx* ctx) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx) return JXLH_ERR_INVALID_ARGUMENT;
  if (ctx->flow_used && ctx->host_flow_flag.p) {
    // a dataflow squeeze launch ran since the last synchronisation: did one of its waits give up?
    ctx->flow_used = false;
    if (jxlh_status st = comm_wait_stream(ctx)) return st;
    if (jxlh_status st = flow_error_status(ctx)) return st;
  }
  if (ctx->in_frame && ctx->error_flag.p) {
    // read the flag on the context's own stream into pinned memory: a synchronous hipMemcpy would
    // go through the null stream and serialise against other contexts' work
    if (!ctx->host_flag.p) HIPCHK(ctx, ctx->host_flag.alloc(1));
    HIPCHK(ctx, hipMemcpyAsync(ctx->host_flag.p, ctx->error_flag.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (jxlh_status st = comm_wait_stream(ctx)) return st;
    if (*ctx->host_flag.p != 0) return (jxlh_status)*ctx->host_flag.p;
    return JXLH_OK;
  }
  return comm_wait_stream(ctx);
}

}  // extern "C"
