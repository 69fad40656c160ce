// Host-side state behind the C ABI: the context structure and the small helpers the abi_*.hip files and comm.hip share.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "blend_rects_plan.h"
#include "device_owned.h"
#include "ec_rects_plan.h"
#include "frame_plan.h"
#include "jxlh_internal.h"
#include "repaint_plan.h"
#include "run_plan.h"
#include "save_rects_plan.h"

using namespace jxlh;

// Every entry point that takes a context makes the context's device the calling thread's current device first: the
// ABI promises one submitting thread per slot plus whoever runs / reads the frame, and HIP's current device is
// per-thread state (a fresh thread sits on device 0).  hipSetDevice on the device already current costs ~70 ns.
#define JXLH_ON_DEVICE(ctx)                        \
  do {                                             \
    if ((ctx) != nullptr) (void)hipSetDevice((ctx)->device); \
  } while (0)

namespace jxlh_host {

struct Slot {
  Stream stream;
  Event done;
  // the last submission's host-to-device copies have landed -- recorded apart from `done` when device work follows the
  // copies on the slot's stream (the 12-bit entries' unpack kernel): jxlh_slot_wait / jxlh_slot_after are about the
  // copies (host buffers, the bus), the frame waits for `done`.  Valid per submission: every one clears or records it.
  Fence copied;
  bool used = false;
  DevBuf<uint8_t> stage8;  // device staging of the 3-byte sparse form (positions | values), grown on demand
};

struct KernelTime {
  std::string name;
  std::vector<std::pair<Event, Event>> pending;
  float total_ms = 0.f;
  int launches = 0;
};

}  // namespace jxlh_host
using namespace jxlh_host;

namespace jxlh_host {
struct Comm;  // comm.hip
}

// The per-frame state: every field that each jxlh_frame_begin must start from the same value, and only those --
// `ctx->frame = FrameState{}` starts them (start_frame, abi_frame.hip, which also takes the steps that are no plain
// value: the extra channels' flags, slots[].used, the host vectors, the coefficient epoch).  Resources and settings of
// the context, what a begin takes from its parameters (params, fd, ngroups, modular, params_direct_ok) and decoder state
// that outlives a frame (refs, lf_slots, the epoch's resident form, se_live, ...) are members of jxlh_ctx.
struct FrameState {
  uint32_t mod_format = 0;  // a Modular frame's sample format (0 = no rect set yet)
  bool lf_smoothed = false;
  // lf_from_slot: this frame's LF image is a copy of an LF slot (no K0b, no jxlh_frame_set_lf*); lf_from_caller: a
  // jxlh_frame_set_lf* call has written into it
  bool lf_from_slot = false, lf_from_caller = false;
  bool rendered = false;                        // a full jxlh_frame_run has happened in this frame
  bool has_special = false, has_large = false;  // transform families seen in the frame's maps (jxlh_frame_set_hf_meta)
  // strip_all_closed: every rect of the transform map came from host memory and every varblock in it is a small DCT
  // inside its 64x64 tile (jxlh_frame_set_hf_meta); strip_ran: the last jxlh_frame_run went through the strip kernel
  // (`planes` then hold no unfiltered pixels)
  bool strip_all_closed = true, strip_ran = false;
  float* result[3] = {nullptr, nullptr, nullptr};  // the planes the last run left the frame in (res_w, res_h, res_stride)
  // chroma-subsampled frame with nothing between the transforms and the output: the upsampling into planes[] is
  // deferred until somebody asks for the planes (the YCbCr output calls read the sub-sampled channels directly);
  // lazy_gr0 / 1: the group rows it is owed on (written whenever chroma_lazy is)
  bool chroma_lazy = false;
  int lazy_gr0 = 0, lazy_gr1 = 0;
  // the patch dictionary (jxlh_frame_set_patches; the reference slots are not per frame).  patch_slots_used bit s: the
  // dictionary reads slot s, up to patch_need_w / _h[s] of it; patch_ec_stale: the patched extra channels must be
  // rebuilt from their base planes on all rows
  uint32_t patch_n = 0, patch_nec = 0;  // 0 patches: no dictionary
  uint32_t patch_ec_alpha = 0, patch_ec_assoc = 0;
  uint32_t patch_need_w[JXLH_MAX_REFERENCE_FRAMES] = {}, patch_need_h[JXLH_MAX_REFERENCE_FRAMES] = {};
  uint32_t patch_slots_used = 0;
  bool patch_ec_stale = true;
  // the splines (jxlh_frame_set_splines): segment count, and which batch's bin list the device holds (-1: none)
  uint32_t spline_n = 0;
  int spline_resident = -1;
  // jxlh_frame_blend: while the frame's result points at the canvas (blended()), blend_frame / blend_f* keep the frame's
  // own planes and geometry, blend_nec the canvas's extra channels
  uint32_t blend_nec = 0;
  float* blend_frame[3] = {nullptr, nullptr, nullptr};
  int blend_fw = 0, blend_fh = 0;
  size_t blend_fstride = 0;
  // jxlh_frame_blend_rects: the canvas holds a composition of this frame (written by jxlh_frame_blend, patched by
  // jxlh_frame_blend_rects) made with blend_kept_desc behind the colour stage blend_kept_mode / _xyb / _tf.  A render
  // points `result` away from the canvas and leaves this record: the stale composition is still in memory
  bool blend_kept = false;
  jxlh_blend_desc blend_kept_desc = {};
  int blend_kept_mode = 0;
  XybParamsDev blend_kept_xyb = {};
  TfParamsDev blend_kept_tf = {};
};

struct jxlh_ctx {
  jxlh_host::Comm* comm = nullptr;  // multi-GPU: rank / transport of this context (null = single GPU)
  int device = 0;
  Stream stream;
  std::vector<Slot> slots;
  Event t0, t1;
  std::string last_error;
  // frame state
  bool in_frame = false;
  // a Modular frame (JXLH_FRAME_MODULAR, abi_modular_frame.hip): the i32 samples of the three colour channels as
  // jxlh_frame_set_modular_channels handed them over, at the planes' row stride (rows 256-byte aligned)
  bool modular = false;
  DevBuf<int32_t> mod_src[3];
  // group-local transforms (abi_modular_local.hip): device scratch of a host arena and of a batch's descriptors + work
  // list; the descriptors go up from a pinned block, reused once local_copied (recorded behind its copy) has passed
  DevBuf<int32_t> local_arena;
  // groups with general palettes: index channels their palette would overwrite, and the weighted predictor's state rows
  DevBuf<int32_t> local_scratch;
  DevBuf<uint8_t> local_desc;
  Pinned<uint8_t> local_desc_host;
  Fence local_copied;
  bool tables_set = false;
  jxlh_frame_params params;
  FrameDev fd;
  FrameState frame;  // what every jxlh_frame_begin starts from its defaults (start_frame, abi_frame.hip)
  size_t ngroups = 0;
  DevBuf<float> planes[3], tmp[3], lf_raw[3], lf_sm[3], sigma, tables;
  int table_offset[JXLH_NUM_QUANT_TABLES] = {0};
  DevBuf<int32_t> coeffs, raw_quant, lfq;
  DevBuf<uint8_t> transform_map, epf_map;
  DevBuf<int8_t> ytox, ytob;
  DevBuf<int> error_flag;
  DevBuf<int> tables_ok;     // FrameDev::tables_ok
  int tables_ok_host = 0;    // ... read back when the tables are set
  bool params_direct_ok = false;  // the frame parameters' share of FrameDev::se_direct_ok
  DevBuf<uint8_t> rgb8;  // write_out's staging for host destinations
  // jxlh_frame_save_rects: the work list on the device; it goes up from a pinned block, reused once save_rects_copied
  // (recorded behind its copy) has passed -- an _async call returns while the copy is still queued
  DevBuf<SaveRectWork> save_rects_dev;
  Pinned<SaveRectWork> save_rects_host;
  Fence save_rects_copied;
  Pinned<int> host_flag;
  DevBuf<uint8_t> worklist;
  DevBuf<int> rerender_list;          // group ids of jxlh_frame_rerender_groups on the device
  std::vector<int> rerender_upload;   // ... and their host copy (alive until the copy has run)
  // jxlh_frame_set_groups_lf_only (abi_lf_fill.hip): the marks (CoeffEpoch::lf_only) as the run in progress took them
  // (empty = no group is marked: the run enqueues what it always did), and the split of the run's groups -- the ones
  // K1 transforms, then the ones the fill writes -- as it is copied to rerender_list
  std::vector<uint8_t> lf_only_run;
  std::vector<int> lf_split_upload;
  // geometry of frame.result (written with it): the frame itself, or its upsampled image (frame_header.upsampling > 1)
  int res_w = 0, res_h = 0;
  size_t res_stride = 0;
  DevBuf<float> noise[3];      // random planes of the noise synthesis
  DevBuf<uint64_t> xs_jump;    // xorshift128+ jump matrices T^(2^j), uploaded on first use
  DevBuf<float> ups[3];        // upsampled planes
  // expanded 5x5 kernels per factor (2, 4, 8), uploaded on first use and whenever jxlh_set_upsampling_weights changes
  // the weights; ups_kernels = the set the last upload_upsampling_kernels call selected
  DevBuf<float> ups_kernels_n[3];
  bool ups_valid[3] = {false, false, false};
  struct { float* p = nullptr; } ups_kernels;
  std::vector<float> ups_weights[3];  // custom weights2 / weights4 / weights8 (empty = defaults)
  // stage hooks scratch
  DevBuf<float> hook_f[8];
  DevBuf<int32_t> hook_i[4];
  // jxlh_unsqueeze_chain's dataflow launches (k6_unsqueeze_flow): ticket + progress words, zeroed per launch; the error
  // word (zeroed when allocated and after an error was reported) is read back by the next jxlh_ctx_sync
  DevBuf<int> flow_words;
  // jxlh_unsqueeze_chain_preview_tiles: the call's work lists (16-byte records) on the device; they go up from a pinned
  // block, reused once its fence (recorded behind the copy) has passed.  The call returns while the copy is queued, and
  // a caller paints again at once: a ring of blocks, so that a call waits for the copy of the fourth call before it
  static constexpr int kSqTilesRing = 4;
  DevBuf<int4> sq_tiles_dev;
  Pinned<int4> sq_tiles_host[kSqTilesRing];
  Fence sq_tiles_copied[kSqTilesRing];
  int sq_tiles_next = 0;
  bool flow_used = false;
  Pinned<int> host_flow_flag;  // device-visible: the dataflow launches' error word (0 = none)
  // jxlh_flow_profile (jxl_hip_dev.h): per-level timeline of the last dataflow launch
  DevBuf<unsigned long long> flow_prof;
  bool flow_prof_on = false;
  int flow_prof_levels = 0;
  // coefficient transport: what this epoch's submissions were and in which form the frame is resident (coeff_epoch.h);
  // the device buffers those forms live in.  Pairs land in sp_pairs (bump allocated, sized for a frame's worst case).
  std::mutex sp_mutex;
  CoeffEpoch epoch;
  DevBuf<uint32_t> sp_pairs;
  DevBuf<SparseGroup> sp_groups_dev;
  DevBuf<uint2> sp_wide_dev;
  Fence sp_expanded;  // recorded behind what consumed the pair buffer (the next epoch's uploads wait)
  Fence k1_done;      // recorded behind the transforms of every jxlh_frame_run: dense resubmissions wait for it
  size_t worklist_nblocks = 0;  // the frame size the work list's fallback flags were last zeroed for
  uint32_t k1_launches = 0;  // parity selects the work-list counter set (vardct_worklist_reset / launch_vardct_groups)
  // Resident::kSortedPairs: the frame's pairs bucketed by varblock slot + slot tables
  DevBuf<uint32_t> sp_sorted, sp_slot_start;
  DevBuf<uint8_t> group_dense;
  DevBuf<uint8_t> bucketed_dev;  // EpochPlan::widen on the device
  // Resident::kEntries: the transforms read the live set se_*[se_live] as uploaded, the next epoch's entries go to the
  // pending set se_*[se_live ^ 1]; the two trade places when a frame arrives slot-bucketed, so the uploads of frame i + 1
  // never touch what the transforms of frame i read.  se_read[i]: recorded behind the last kernels that read set i.
  DevBuf<uint16_t> se_entries[2];
  DevBuf<uint8_t> se_counts[2];
  DevBuf<uint2> se_runs[2];
  Fence se_read[2];
  int se_live = 0;
  DevBuf<uint8_t> route_dev;  // Residence::route on the device (FrameDev::group_route)
  // extra channels inside the frame path (jxlh_frame_set_extra_channel): as handed over, converted, upsampled
  struct ExtraChannel {
    bool set = false, done = false;
    uint32_t w = 0, h = 0, bits = 0, up = 1;
    uint32_t out_w = 0, out_h = 0;
    size_t out_stride = 0;
    DevBuf<int32_t> raw;
    DevBuf<float> f32, out;
    // the channel with the frame's patches drawn in (abi_patches.hip); `pat_ready`: it holds the current dictionary's
    // result for the current conversion (read-outs then return it)
    DevBuf<float> pat;
    bool pat_ready = false;
    // rect state (jxl_hip_extra_rects.h): the channel was begun without samples or touched by a rects call -- a run
    // finishes only the dirty tiles of ec_plan.ch[i]
    bool rect = false;
  };
  ExtraChannel extra[JXLH_MAX_EXTRA_CHANNELS];
  // extra channels by rect: the channels' tile grids and dirty bitmaps (ec_rects_plan.h); the scatter descriptors of a
  // rects call and the host block's span on the device; a run's channel descriptors + item list.  Both lists go up from
  // a pinned block, reused once its fence (recorded behind the copy) has passed.
  EcRectsPlan ec_plan;
  DevBuf<int32_t> ec_block;
  DevBuf<EcScatterDesc> ec_scatter_dev;
  Pinned<EcScatterDesc> ec_scatter_host;
  Fence ec_scatter_copied;
  DevBuf<uint8_t> ec_finish_dev;
  Pinned<uint8_t> ec_finish_host;
  Fence ec_finish_copied;
  std::vector<EcItem> ec_items;
  // reference frames (DecoderState::reference_frames): n_channels planes of w x h at `stride`, channel c at c * stride * h
  struct RefSlot {
    bool set = false;
    uint32_t n_channels = 0, w = 0, h = 0;
    size_t stride = 0;
    DevBuf<float> buf;
  };
  RefSlot refs[JXLH_MAX_REFERENCE_FRAMES];
  // LF frames (DecoderState::lf_frames, abi_lf_frame.hip): the X, Y, B planes of w x h at `stride` (rows 256-byte
  // aligned), channel c at c * stride * h
  struct LfSlot {
    bool set = false;
    uint32_t w = 0, h = 0;
    size_t stride = 0;
    DevBuf<float> buf;
  };
  LfSlot lf_slots[JXLH_NUM_LF_FRAMES];
  // the frame's patch dictionary (jxlh_frame_set_patches), binned into 64 x 4 tiles: words = tile ids | starts | patch
  // indices; row_first[r] = first listed tile of tile row r
  struct PatchBins {
    int w = 0, h = 0, ntx = 0, nty = 0;
    uint32_t ntiles = 0;
    std::vector<uint32_t> words, row_first;
    DevBuf<uint32_t> dev;
  };
  std::vector<PatchDev> patch_desc_host;
  DevBuf<PatchDev> patch_desc;
  PatchBins patch_bins, patch_hook_bins;
  DevBuf<float> patch_hook;    // jxlh_stage_patches staging
  // the frame's spline segments (jxlh_frame_set_splines, abi_splines.hip): as the kernel reads them, host and device;
  // spline_first = the batches of consecutive segments planned for spline_plan_w x _h under spline_budget entries;
  // spline_bins = the bin list of batch frame.spline_resident for that size, also on the device
  std::vector<SplineDev> spline_desc_host;
  DevBuf<SplineDev> spline_desc;
  std::vector<uint32_t> spline_first;
  int spline_plan_w = 0, spline_plan_h = 0;
  SplineBins spline_bins;
  DevBuf<uint32_t> spline_bins_dev;
  uint64_t spline_budget = kSplineDefaultBudget;
  DevBuf<float> spline_hook;  // jxlh_stage_splines staging
  // frame blending (abi_blend.hip): the image-sized canvas of 3 + frame.blend_nec planes, channel c at
  // c * res_stride * res_h
  DevBuf<float> blend_canvas;
  DevBuf<float> blend_hook_in, blend_hook_out;  // jxlh_stage_blend staging
  // jxlh_frame_blend_rects: the work list on the device; it goes up from a ring of pinned blocks, each reused once its
  // fence (recorded behind the copy) has passed -- the call returns while the copy is queued, and a caller recomposes
  // again at once: a call waits for the copy of the fourth call before it
  static constexpr int kBlendRectsRing = 4;
  DevBuf<BlendRectWork> blend_rects_dev;
  Pinned<BlendRectWork> blend_rects_host[kBlendRectsRing];
  Fence blend_rects_copied[kBlendRectsRing];
  int blend_rects_next = 0;
  DevBuf<float> save_hook_in;                   // jxlh_stage_save staging of host planes (abi_save.hip)
  // strip path (k_strip.hip): block descriptors / tile modes written by k1_scan, the strips' edge-column exchange
  // buffer, progress flags + ticket
  DevBuf<uint2> strip_desc;
  DevBuf<uint8_t> strip_mode;
  DevBuf<float> strip_xchg;
  DevBuf<int> strip_flags;
  int cu_count = 0;
  // jxlh_ctx_tune_placement: candidate sets the first allocation of the large buffers is picked from (<= 1: plain
  // allocation); what the last pick saw (k1-like ms, filter-like ms per candidate) and took
  int placement_trials = 1;
  std::vector<float> placement_report;
  int placement_pick = -1;
  int strip_resident = 0;  // strip_resident_workgroups(cu_count), 0 = not asked yet
  // jxlh_ctx_mark / jxlh_ctx_wait_mark: a ring of events on the main stream
  Event handover;  // jxlh_ctx_wait_stream: recorded on the caller's stream
  Event marks[JXLH_MAX_MARKS];
  uint32_t mark_seq = 0;
  // profiling
  bool timing = false;
  std::vector<KernelTime> ktimes;
};

namespace jxlh_host {

inline jxlh_status fail(jxlh_ctx* ctx, hipError_t e, const char* what) {
  if (ctx) {
    ctx->last_error = std::string(what) + ": " + hipGetErrorString(e);
  }
  (void)hipGetLastError();  // clear the sticky per-thread error so later checks start clean
  return e == hipErrorOutOfMemory ? JXLH_ERR_OUT_OF_MEMORY : JXLH_ERR_DEVICE;
}

#define HIPCHK(ctx, expr)                               \
  do {                                                  \
    hipError_t e_ = (expr);                             \
    if (e_ != hipSuccess) return fail(ctx, e_, #expr);  \
  } while (0)

// k_probe.hip: average ms of two byte movers with K1's and the filters' streams on a candidate set of buffers
jxlh_status probe_placement(jxlh_ctx* ctx, const int32_t* coeffs, size_t ngroups, float* const planes[3], float* const tmp[3],
                            size_t plane_elems, float* k1_like_ms, float* filter_like_ms);

template <class T>
jxlh_status ensure(jxlh_ctx* ctx, DevBuf<T>& b, size_t n) {
  const char* what = "";
  const hipError_t e = b.ensure(n, &what);
  return e == hipSuccess ? JXLH_OK : fail(ctx, e, what);
}

struct ScopedKernelTimer {
  jxlh_ctx* ctx;
  Event a, b;
  KernelTime* kt = nullptr;
  ScopedKernelTimer(jxlh_ctx* c, const char* name) : ctx(c) {
    if (!ctx->timing) return;
    for (auto& k : ctx->ktimes)
      if (k.name == name) kt = &k;
    if (!kt) {
      ctx->ktimes.push_back(KernelTime{name, {}, 0.f, 0});
      kt = &ctx->ktimes.back();
    }
    (void)a.create(true);
    (void)b.create(true);
    (void)hipEventRecord(a, ctx->stream);
  }
  ~ScopedKernelTimer() {
    if (!kt) return;
    (void)hipEventRecord(b, ctx->stream);
    kt->pending.emplace_back(std::move(a), std::move(b));
  }
};

inline void drain_timers(jxlh_ctx* ctx) {
  for (auto& k : ctx->ktimes) {
    for (auto& pr : k.pending) {
      (void)hipEventSynchronize(pr.second);
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
        k.total_ms += ms;
        k.launches += 1;
      }
    }
    k.pending.clear();
  }
}

inline size_t round_up(size_t v, size_t m) { return (v + m - 1) / m * m; }

// plane -> device 2-D copy helper (pointers may be host or device)
inline bool is_device_ptr(const void* p) {
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return attr.type == hipMemoryTypeDevice;
}

inline jxlh_status copy2d(jxlh_ctx* ctx, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width_bytes,
                   size_t height, hipStream_t s) {
  if (width_bytes == 0 || height == 0) return JXLH_OK;
  if (dpitch == width_bytes && spitch == width_bytes) {  // contiguous on both sides: one linear copy
    HIPCHK(ctx, hipMemcpyAsync(dst, src, width_bytes * height, hipMemcpyDefault, s));
    return JXLH_OK;
  }
  HIPCHK(ctx, hipMemcpy2DAsync(dst, dpitch, src, spitch, width_bytes, height, hipMemcpyDefault, s));
  return JXLH_OK;
}

// A run is "fill the inputs, plan, issue" (run_plan.h): run_inputs reads what the decisions depend on out of the context
// (and takes the snapshot of the LF-only marks), plan_run / plan_rerender / plan_shard decide, and the pieces below issue
// what the plan says -- three of them, so that a sharded run (comm.hip) can put the halo exchange between the
// transforms and the filters.  run_prologue: everything before K1; *sparse_k1 is the coefficient epoch's answer, which
// resolve_strip puts into the plan.  run_k1: the transforms on the plan's k1 rows.  run_stages_rows: the stage list on
// pixel rows (the plan's, or a re-render's bands), then the post stages.
StageList stage_list(const jxlh_ctx* ctx);
RunInputs run_inputs(jxlh_ctx* ctx);
jxlh_status run_prologue(jxlh_ctx* ctx, bool strip_candidate, bool tiled, bool* sparse_k1);
jxlh_status run_k1(jxlh_ctx* ctx, const RunPlan& plan);
// repaint (jxlh_frame_repaint_groups, else null): the band belongs to a repaint, whose plan names the coded rows to
// upsample again and the result rows that then take their noise again (repaint_plan.h).  A repaint of several bands
// hands the rows over with its LAST band, when every coded row is final, and empty lists with the others.
struct PostRepaint {
  const std::vector<RowRange>* centre_rows;
  const std::vector<RowRange>* noise_rows;
};
jxlh_status run_stages_rows(jxlh_ctx* ctx, const StageList& stages, int y_lo, int y_hi, bool whole_frame,
                            const PostRepaint* repaint = nullptr);
jxlh_status run_post_stages(jxlh_ctx* ctx, float* const cur[3], int y_lo, int y_hi, bool whole_frame,
                            const PostRepaint* repaint = nullptr);
jxlh_status run_extra_channels(jxlh_ctx* ctx);  // ConvertModularToF32 + Upsample of the channels handed over
jxlh_status run_extra_channel_rects(jxlh_ctx* ctx);  // ... and of the dirty tiles of the channels with rect state
// an extra channel a run still has to convert: handed over or touched since it was last finished
inline bool extra_pending(const jxlh_ctx* ctx, uint32_t i) {
  return ctx->extra[i].set && (!ctx->extra[i].done || (ctx->extra[i].rect && ctx->ec_plan.dirty(i)));
}
// abi_patches.hip: the patches stage on the colour planes `cur` (rows [y_lo, y_hi)) and, when stale, on every row of
// the patched extra channels; the check a run makes before it launches anything
jxlh_status run_patches(jxlh_ctx* ctx, float* const cur[3], size_t stride, int y_lo, int y_hi);
jxlh_status patches_check_run(const jxlh_ctx* ctx);
// abi_splines.hip: the splines stage on the colour planes `cur` (rows [y_lo, y_hi))
jxlh_status run_splines(jxlh_ctx* ctx, float* const cur[3], size_t stride, int w, int h, int y_lo, int y_hi);
// patches and splines are drawn IN PLACE on the finished planes: whatever must not reach a pixel twice asks this
inline bool draws_in_place(const jxlh_ctx* ctx) { return ctx->frame.patch_n > 0 || ctx->frame.spline_n > 0; }
// abi_blend.hip.  blended(): the frame's result is the canvas jxlh_frame_blend composed (any render resets `result`).
inline bool blended(const jxlh_ctx* ctx) { return ctx->blend_canvas.p && ctx->frame.result[0] == ctx->blend_canvas.p; }
// abi_save.hip: the argument checks, shared with jxlh_lf_preview: the descriptor's own (n_planes: pipeline channels that
// exist), `out` and its pitch against the oriented image of a w x h source
jxlh_status save_check_desc(const jxlh_save_desc* d, uint32_t n_planes);
jxlh_status save_check_out(const jxlh_save_desc* d, uint32_t w, uint32_t h, const void* out, size_t bytes_per_row);
// ... the colour stage `colour` names (null = none) as the kernels take it: every entry point with a jxlh_output_desc
jxlh_status colour_stage(const jxlh_output_desc* colour, int* mode, XybParamsDev* xyb, TfParamsDev* tf);
// ... and what a (checked) descriptor says about the samples and their place: a.format, maxv, big_endian, fill_bits,
// transpose, flip_x, flip_y of a SaveLaunch / LfPreviewLaunch
inline int save_sample_bytes(uint32_t format) { return format == JXLH_SAVE_U8 ? 1 : format == JXLH_SAVE_F32 ? 4 : 2; }
template <class Launch>
void save_format(const jxlh_save_desc* d, Launch& a) {
  a.format = (int)d->format;  // JXLH_SAVE_* share the values of kSave*
  const uint32_t max_int = d->format <= JXLH_SAVE_U16 ? (1u << d->bit_depth) - 1 : 0;
  a.maxv = (float)max_int;
  a.big_endian = d->big_endian && d->format != JXLH_SAVE_U8;
  a.fill_bits = d->format <= JXLH_SAVE_U16 ? max_int : d->format == JXLH_SAVE_F16 ? 0x3c00u : 0x3f800000u;
  if (a.big_endian)
    a.fill_bits = d->format == JXLH_SAVE_F32 ? __builtin_bswap32(a.fill_bits)
                                             : (((a.fill_bits >> 8) | (a.fill_bits << 8)) & 0xffffu);
  const uint32_t o = d->orientation;  // headers/image_metadata.rs:85-96
  a.transpose = o >= 5;
  a.flip_x = o == 2 || o == 3 || o == 6 || o == 7;
  a.flip_y = o == 3 || o == 4 || o == 7 || o == 8;
}
struct OutRect {
  size_t x0, y0, w, h;  // pixels of an oriented output image
};
// the tail of jxlh_frame_save, which the integer read-outs (abi_output.hip) share: rows [y0, y1) of the frame's result
// through the save `d` (checked; ec_plane / ec_stride: the extra channels it names, may be null when it names none)
// behind the colour stage already in `a`, into the oriented image at `image`
jxlh_status save_result_rows(jxlh_ctx* ctx, SaveLaunch& a, const jxlh_save_desc* d, const float* const* ec_plane,
                             const uint32_t* ec_stride, uint32_t y0, uint32_t y1, void* image, size_t bytes_per_row,
                             const char* label, bool wait);
// abi_lf_fill.hip.  lf_only_snapshot: ctx->lf_only_run <- the frame's marks (true = at least one group is marked).
// lf_split_groups: the sorted `groups` of a run, the unmarked ones (all, without marks) first, on the device (rerender_list);
// *n_k1 of them are K1's, the *n_fill behind them the fill's.  run_lf_fill: Upsample8x of the LF image into the planes
// K1 writes, for the n groups listed at `groups_dev`.
bool lf_only_snapshot(jxlh_ctx* ctx);
jxlh_status lf_split_groups(jxlh_ctx* ctx, const std::vector<int>& groups, int* n_k1, int* n_fill);
jxlh_status run_lf_fill(jxlh_ctx* ctx, const FrameDev& f, const int* groups_dev, int n);
jxlh_status run_strip(jxlh_ctx* ctx);
void set_filter_params(FrameDev& f, const jxlh_frame_params& p);  // abi_frame.hip
// jxlh_frame_begin's commit takes its sizes from the plan (frame_plan.h).  abi_ctx.hip: the first allocation of the
// large buffers as a pick among candidate sets (jxlh_ctx_tune_placement)
jxlh_status choose_placement(jxlh_ctx* ctx, const FramePlan& pl);
// abi_modular_frame.hip: the commit / jxlh_frame_run of a Modular frame
jxlh_status modular_frame_begin(jxlh_ctx* ctx, const FramePlan& pl);
jxlh_status modular_frame_run(jxlh_ctx* ctx, uint32_t group_row0, uint32_t group_row1);
// ... and what it issues for a plan: the intake of the plan's rows, the stage list on rows [y_lo, y_hi)
jxlh_status modular_frame_issue(jxlh_ctx* ctx, const RunPlan& plan, int y_lo, int y_hi, const PostRepaint* repaint);
void run_chroma_upsample_rows(jxlh_ctx* ctx, int y0, int y1);  // frame_run.hip: ... of the rows that cover [y0, y1)
// frame_run.hip: pieces of the frame pipeline the read-out and stage-hook entry points share
bool noise_lut_is_zero(const float lut[8]);
void materialise_chroma(jxlh_ctx* ctx);          // deferred chroma upsampling of a sub-sampled frame, if still pending
jxlh_status ensure_jump_table(jxlh_ctx* ctx);    // xorshift128+ jump matrices of the noise generator
jxlh_status upload_upsampling_kernels(jxlh_ctx* ctx, int n);  // abi_frame.hip

// host or device source -> context-owned device scratch / back, on the main stream (stage hooks, Modular entry points)
template <class T>
jxlh_status stage_in(jxlh_ctx* ctx, DevBuf<T>& b, const T* src, size_t n) {
  jxlh_status st = ensure(ctx, b, n);
  if (st != JXLH_OK) return st;
  HIPCHK(ctx, hipMemcpyAsync(b.p, src, n * sizeof(T), hipMemcpyDefault, ctx->stream));
  return JXLH_OK;
}
// abi_output.hip
jxlh_status convert_band_to_output(jxlh_ctx* ctx, const jxlh_output_desc* d, uint32_t y0, uint32_t y1, void* out,
                                   size_t bytes_per_row);
// comm.hip
void comm_release(jxlh_ctx* ctx);
int comm_nranks(const jxlh_ctx* ctx);
// hipStreamSynchronize with a deadline while collectives may be queued.  EVERY blocking wait on the context's stream goes
// through it (JXLH_SYNC): on a sharded context a stuck collective then surfaces as JXLH_ERR_DEVICE from whichever call
// waits first -- a read-out as well as jxlh_ctx_sync -- instead of parking the process in the driver.
jxlh_status comm_wait_stream(jxlh_ctx* ctx);
#define JXLH_SYNC(ctx)                                        \
  do {                                                        \
    if (jxlh_status st_ = comm_wait_stream(ctx)) return st_;  \
  } while (0)
template <class T>
jxlh_status stage_out(jxlh_ctx* ctx, T* dst, const T* src, size_t n) {
  HIPCHK(ctx, hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDefault, ctx->stream));
  JXLH_SYNC(ctx);
  return JXLH_OK;
}

// The one way interleaved samples leave the device.  `launch(origin, pitch)` writes the pixels of rectangle `r` of an
// oriented output image whose pixel (0, 0) is at `origin`, rows `pitch` bytes apart; `dst` is where the rectangle's first
// pixel goes, rows bytes_per_row apart.  Device memory is written in place and never waited for.  Host memory goes
// through ctx->rgb8, which holds exactly the rectangle at a dword-rounded pitch (the origin is shifted so that the
// rectangle starts the buffer; it is never dereferenced outside it), and a 2-D copy of exactly the pixel bytes -- row
// padding and bytes outside the rectangle are never touched --, then a wait if `wait`.  `label` names the launch in
// jxlh_kernel_timing_get.
template <class Launch>
jxlh_status write_out(jxlh_ctx* ctx, void* dst, size_t bytes_per_row, size_t pixel_bytes, const OutRect& r,
                      const char* label, bool wait, Launch launch) {
  const bool staged = !is_device_ptr(dst);
  const size_t row_bytes = r.w * pixel_bytes, pitch = staged ? round_up(row_bytes, 4) : bytes_per_row;
  if (staged)
    if (jxlh_status st = ensure(ctx, ctx->rgb8, pitch * r.h)) return st;
  const uintptr_t first = reinterpret_cast<uintptr_t>(staged ? ctx->rgb8.p : dst);
  {
    ScopedKernelTimer t(ctx, label);
    launch(reinterpret_cast<uint8_t*>(first - r.y0 * pitch - r.x0 * pixel_bytes), pitch);
  }
  HIPCHK(ctx, hipGetLastError());
  if (!staged) return JXLH_OK;
  if (jxlh_status st = copy2d(ctx, dst, bytes_per_row, ctx->rgb8.p, pitch, row_bytes, r.h, ctx->stream)) return st;
  if (wait) JXLH_SYNC(ctx);
  return JXLH_OK;
}

}  // namespace jxlh_host
using namespace jxlh_host;
