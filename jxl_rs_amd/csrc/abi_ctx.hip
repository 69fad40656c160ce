// C ABI, the context's lifetime: version and status strings, default parameters, create / destroy, pinned memory, the
// placement of the large buffers, and the calls that order the context's streams against the caller's (events, marks,
// jxlh_ctx_sync).  What belongs to a frame is in abi_frame.hip (begin and setters) and frame_run.hip (the run).
#include <algorithm>

#include "jxlh_ctx.h"

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

}  // extern "C"

namespace jxlh_host {
// Where the driver places a context's large buffers decides how fast the transforms and the filters run on them: the
// same kernels on the same data are up to 10 % apart between two contexts of one process, persistently, while copies
// between the buffers run alike (profiles/r06_q_context_placement.txt).  With jxlh_ctx_tune_placement(ctx, n) the first
// allocation of {three planes, three filter planes, coefficient buffer} becomes a pick among n candidate sets, rated by
// two byte movers with the streams of the 8x8 transform class and of the filters (k_probe.hip); the candidates are held
// until the pick (so that they ARE different placements), then all but the best are freed.  Setup cost: n x ~2.6 GB of
// transient device memory at 8192^2 and a few ms per candidate; a candidate that cannot be allocated ends the trials.
jxlh_status choose_placement(jxlh_ctx* ctx, const FramePlan& pl) {
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
    for (int i = 0; i < 3 && ok; i++) {  // (the order of jxlh_frame_begin's plain path)
      ok = c.planes[i].alloc(pl.planes_n) == hipSuccess && c.tmp[i].alloc(pl.tmp_n) == hipSuccess;
    }
    ok = ok && c.coeffs.alloc(pl.coeffs_n) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();  // out of memory: the candidates so far are the choice
      break;
    }
    float* const planes[3] = {c.planes[0].p, c.planes[1].p, c.planes[2].p};
    float* const tmp[3] = {c.tmp[0].p, c.tmp[1].p, c.tmp[2].p};
    if (jxlh_status st = probe_placement(ctx, c.coeffs.p, pl.ngroups, planes, tmp, pl.probe_elems, &c.k1, &c.filt))
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
}  // namespace jxlh_host

extern "C" {

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
