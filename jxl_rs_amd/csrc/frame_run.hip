// The run of a frame: jxlh_frame_run and jxlh_frame_rerender_groups, and the pieces they issue -- the coefficient
// transport of an epoch, K0b / K3 sigma, the transforms, the strip kernel, the stage list and what follows it (patches,
// splines, upsampling, noise, the extra channels).  "Fill the inputs, plan, issue": run_plan.h decides the routing.
// No compute happens on the host here and there is no CPU fallback: every entry point launches HIP kernels or fails.
#include <algorithm>

#include "jxlh_ctx.h"

namespace jxlh_host {

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
  if (!ctx->frame.chroma_lazy) return;
  run_chroma_upsample_rows(ctx, ctx->frame.lazy_gr0 * kGroupDim, ctx->frame.lazy_gr1 * kGroupDim);
  ctx->frame.chroma_lazy = false;
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
                   strip_forced || (p.flags & JXLH_FRAME_STRIP), lf_only_snapshot(ctx), ctx->frame.rendered, ctx->frame.strip_ran};
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
  const bool smooth = p.do_lf_smoothing && !ctx->frame.lf_from_slot && f.xblocks > 2 && f.yblocks > 2;
  if (smooth) {
    {  // out of place (raw -> smoothed), so re-running a frame repeats the full work
      const float inv_quant_lf = f.inv_global_scale / (float)p.quant_lf;  // quantizer.rs:82-84
      const float lf_factors[3] = {inv_quant_lf * p.lf_quant_factors[0], inv_quant_lf * p.lf_quant_factors[1],
                                   inv_quant_lf * p.lf_quant_factors[2]};
      const float* in[3] = {ctx->lf_raw[0].p, ctx->lf_raw[1].p, ctx->lf_raw[2].p};
      float* out[3] = {ctx->lf_sm[0].p, ctx->lf_sm[1].p, ctx->lf_sm[2].p};
      ScopedKernelTimer t(ctx, "k0b_lf_smooth");
      launch_lf_smooth(ctx->stream, in, out, f.xblocks, f.yblocks, lf_factors);
      ctx->frame.lf_smoothed = true;
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
                         listed ? n_k1 : 0, ctx->frame.has_special, ctx->frame.has_large, sparse_k1 ? ctx->epoch.live.n_route : 0);
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
  ctx->frame.chroma_lazy = plan.chroma_lazy;
  if (f.subsampled) {
    // ... and brought to full resolution into planes[c] before any filter, or lazily (run_plan.h: band_plan)
    ctx->frame.lazy_gr0 = gr0;
    ctx->frame.lazy_gr1 = gr1;
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
  f.strip_all_closed = ctx->frame.strip_all_closed ? 1 : 0;
  f.tiled = 1;
  set_sparse_view(ctx, f, false);
  {
    ScopedKernelTimer t(ctx, "k1_vardct");
    launch_vardct_groups(ctx->stream, f, 0, f.ygroups, ctx->worklist.p, &ctx->k1_launches, ctx->error_flag.p, nullptr,
                         nullptr, 0, ctx->frame.has_special, ctx->frame.has_large, 0);
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
  ctx->frame.chroma_lazy = false;
  ctx->frame.rendered = true;
  ctx->frame.strip_ran = true;
  // upsampling / noise behind the stage list: the strip kernel leaves the filtered planes in f.tmp
  return run_post_stages(ctx, f.tmp, 0, f.ysize, true);
}

// the stage list on pixel rows [y_lo, y_hi), then upsampling and noise
jxlh_status run_stages_rows(jxlh_ctx* ctx, const StageList& sl, int y_lo, int y_hi, bool whole_frame,
                            const PostRepaint* repaint) {
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
  return run_post_stages(ctx, cur, y_lo, y_hi, whole_frame, repaint);
}

// what follows the filters: patches, splines, upsampling and noise on the finished planes `cur` (rows [y_lo, y_hi))
jxlh_status run_post_stages(jxlh_ctx* ctx, float* const cur[3], int y_lo, int y_hi, bool whole_frame,
                            const PostRepaint* repaint) {
  FrameDev& f = ctx->fd;
  const jxlh_frame_params& p = ctx->params;
  for (int c = 0; c < 3; c++) ctx->frame.result[c] = cur[c];
  ctx->res_w = f.xsize;
  ctx->res_h = f.ysize;
  ctx->res_stride = f.plane_stride;
  bool extra_run = false;
  if (ctx->frame.patch_n > 0) {
    // PatchesStage (frame/render.rs:644-650): after the extra channels' own upsampling, before the colour upsampling
    // and noise, at the coded size.  The extra channels must be converted before the patches read them.
    bool pending = whole_frame;
    for (uint32_t i = 0; i < ctx->frame.patch_nec; i++) pending |= !ctx->extra[i].done || extra_pending(ctx, i);
    if (ctx->frame.patch_nec > 0 && pending) {
      if (jxlh_status st = run_extra_channels(ctx)) return st;
      extra_run = true;
    }
    if (jxlh_status st = run_patches(ctx, cur, f.plane_stride, y_lo, y_hi)) return st;
  }
  // SplinesStage (frame/render.rs:652-653): behind patches, at the coded size
  if (ctx->frame.spline_n > 0)
    if (jxlh_status st = run_splines(ctx, cur, f.plane_stride, f.xsize, f.ysize, y_lo, y_hi)) return st;
  if (p.upsampling > 1) {
    // Upsample2x/4x/8x on the three colour channels (frame/render.rs:655-671).  The 5x5 window crosses band
    // edges, so an upsampled frame is run whole -- or, by a repaint behind a whole run, on the rows its plan names.
    if (!whole_frame && !repaint) return JXLH_ERR_UNSUPPORTED;
    const int n = (int)p.upsampling;
    const int ow = p.xsize_upsampled ? (int)p.xsize_upsampled : f.xsize * n;
    const int oh = p.ysize_upsampled ? (int)p.ysize_upsampled : f.ysize * n;
    const size_t ostride = round_up((size_t)f.xsize * n, 64);
    if (jxlh_status st = upload_upsampling_kernels(ctx, n)) return st;
    for (int c = 0; c < 3; c++)
      if (jxlh_status st = ensure(ctx, ctx->ups[c], ostride * (size_t)f.ysize * n)) return st;
    if (whole_frame) {
      ScopedKernelTimer t(ctx, "k_upsample");
      for (int c = 0; c < 3; c++)
        launch_upsample(ctx->stream, n, cur[c], f.plane_stride, f.xsize, f.ysize, ctx->ups_kernels.p, ctx->ups[c].p,
                        ostride, ow, oh);
    } else if (!repaint->centre_rows->empty()) {
      // (the buffers are the whole run's: ensure() at an unchanged size keeps them and what they hold)
      float* const out[3] = {ctx->ups[0].p, ctx->ups[1].p, ctx->ups[2].p};
      ScopedKernelTimer t(ctx, "k_upsample_rows");
      for (const RowRange& r : *repaint->centre_rows)
        launch_upsample_rows(ctx->stream, n, cur, f.plane_stride, f.xsize, f.ysize, r.lo, r.hi, ctx->ups_kernels.p, out,
                             ostride, ow, oh);
    }
    for (int c = 0; c < 3; c++) ctx->frame.result[c] = ctx->ups[c].p;
    ctx->res_w = ow;
    ctx->res_h = oh;
    ctx->res_stride = ostride;
  }
  if (p.noise && !noise_lut_is_zero(p.noise_lut)) {  // AddNoiseStage returns early on an all-zero LUT (noise.rs:153-155)
    // render_noise_for_group + ConvolveNoise x3 + AddNoise (frame/decode.rs:578-668, frame/render.rs:673-683),
    // at the resolution of the result (after upsampling).  Random planes: the 256-row tile rows that cover
    // the band plus the convolution's 2-row border.
    // An upsampled frame: all of it -- or, in a repaint, exactly the result rows that were just written again (every
    // other row still carries the noise of the whole run: adding it there would add it twice).
    const int W = ctx->res_w, H = ctx->res_h;
    const RowRange own{p.upsampling > 1 ? 0 : y_lo, p.upsampling > 1 ? H : y_hi};
    const bool listed = p.upsampling > 1 && !whole_frame;
    const RowRange* rows = listed ? repaint->noise_rows->data() : &own;
    const size_t n_rows = listed ? repaint->noise_rows->size() : 1;
    if (jxlh_status st = ensure_jump_table(ctx)) return st;
    for (int c = 0; c < 3; c++)
      if (jxlh_status st = ensure(ctx, ctx->noise[c], ctx->res_stride * (size_t)H)) return st;
    float* nz[3] = {ctx->noise[0].p, ctx->noise[1].p, ctx->noise[2].p};
    const float ytox = p.base_correlation_x + (float)p.ytox_lf / (float)p.color_factor;  // y_to_x_lf
    const float ytob = p.base_correlation_b + (float)p.ytob_lf / (float)p.color_factor;
    for (size_t i = 0; i < n_rows; i++) {
      const int ya = rows[i].lo, yb = rows[i].hi;
      const int ty0 = max(0, ya - 2) / 256, ty1 = (min(H, yb + 2) + 255) / 256;
      {
        ScopedKernelTimer t(ctx, "k_noise_generate");
        launch_noise_generate(ctx->stream, nz, ctx->res_stride, W, H, ty0, ty1, p.visible_frame_index,
                              p.nonvisible_frame_index, ctx->xs_jump.p);
      }
      ScopedKernelTimer t(ctx, "k_noise_apply");
      launch_noise_apply(ctx->stream, nz, ctx->res_stride, ctx->frame.result, ctx->res_stride, W, H, ya, yb, p.noise_lut,
                         ytox, ytob);
    }
  }
  // (a partial re-render still picks up a channel that was handed over after the last whole-frame run)
  bool pending_extra = false;
  for (int i = 0; i < JXLH_MAX_EXTRA_CHANNELS; i++) pending_extra |= extra_pending(ctx, (uint32_t)i);
  if ((whole_frame || pending_extra) && !extra_run)
    if (jxlh_status st = run_extra_channels(ctx)) return st;
  HIPCHK(ctx, hipGetLastError());
  return JXLH_OK;
}

// channels 3.. of the reference's pipeline: ConvertModularToF32Stage, then Upsample<N> by the channel's own factor
// (frame/render.rs:564-567, :624-637 / :655-671)
jxlh_status run_extra_channels(jxlh_ctx* ctx) {
  bool rect_channels = false;
  for (int i = 0; i < JXLH_MAX_EXTRA_CHANNELS; i++) {
    jxlh_ctx::ExtraChannel& e = ctx->extra[i];
    if (!e.set) continue;
    if (e.rect) {  // only its dirty tiles, below
      rect_channels = true;
      continue;
    }
    const size_t n = (size_t)e.w * e.h;
    e.done = false;
    e.pat_ready = false;  // a new base: the patched copy is rebuilt by the next patches launch
    ctx->frame.patch_ec_stale = true;
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
  return rect_channels ? run_extra_channel_rects(ctx) : JXLH_OK;
}

// The channels with rect state (jxl_hip_extra_rects.h): the dirty tiles of all of them (ec_rects_plan.h) in at most one
// k_ec_finish launch per factor -- ConvertModularToF32Stage, and Upsample<N> read from the i32 samples.  The buffers and
// strides are the whole-plane path's, so every reader of a finished channel takes them as they are.
jxlh_status run_extra_channel_rects(jxlh_ctx* ctx) {
  const uint32_t full_w = (uint32_t)(ctx->res_w > 0 ? ctx->res_w : ctx->fd.xsize),
                 full_h = (uint32_t)(ctx->res_h > 0 ? ctx->res_h : ctx->fd.ysize);
  EcChannelDesc chans[JXLH_MAX_EXTRA_CHANNELS] = {};
  size_t n_items = 0;
  for (int i = 0; i < JXLH_MAX_EXTRA_CHANNELS; i++) {
    jxlh_ctx::ExtraChannel& e = ctx->extra[i];
    if (!e.set || !e.rect) continue;
    const EcGrid& g = ctx->ec_plan.ch[i];
    e.out_w = std::min(e.w * e.up, full_w);
    e.out_h = std::min(e.h * e.up, full_h);
    e.out_stride = e.up > 1 ? round_up((size_t)e.w * e.up, 64) : e.w;
    DevBuf<float>& dst = e.up > 1 ? e.out : e.f32;
    // (allocated by the first run after the begin, when every tile is dirty, or by the whole-plane run before the rects)
    if (jxlh_status st = ensure(ctx, dst, e.up > 1 ? e.out_stride * (size_t)e.h * e.up : (size_t)e.w * e.h)) return st;
    if (e.up > 1)  // on first use this uploads and waits: in front of the timed launches
      if (jxlh_status st = upload_upsampling_kernels(ctx, (int)e.up)) return st;
    n_items += g.n_dirty;
    EcChannelDesc& c = chans[i];
    c.raw = e.raw.p;
    c.dst = dst.p;
    c.dst_stride = e.out_stride;
    c.w = e.w;
    c.h = e.h;
    c.ntx = g.ntx;
    c.out_w = e.out_w;
    c.out_h = e.out_h;
    c.bits = e.bits & 0xffu;
    c.exp_bits = e.bits >> 8;
    c.scale = c.exp_bits ? 0.0f : 1.0f / (float)((1ull << c.bits) - 1);
  }
  if (n_items) {
    // room first: once the plan has handed its tiles over (collect) they are issued
    const size_t bytes = sizeof(chans) + n_items * sizeof(EcItem);
    if (jxlh_status st = ensure(ctx, ctx->ec_finish_dev, bytes)) return st;
    HIPCHK(ctx, ctx->ec_finish_copied.sync());  // the pinned block's previous list is on its way
    ctx->ec_finish_copied.clear();
    if (ctx->ec_finish_host.n < bytes) {
      HIPCHK(ctx, ctx->ec_finish_host.reset());
      HIPCHK(ctx, ctx->ec_finish_host.alloc(bytes + bytes / 2));
    }
    uint32_t first[5];
    ctx->ec_plan.collect(ctx->ec_items, first);
    std::memcpy(ctx->ec_finish_host.p, chans, sizeof(chans));
    std::memcpy(ctx->ec_finish_host.p + sizeof(chans), ctx->ec_items.data(), n_items * sizeof(EcItem));
    HIPCHK(ctx, hipMemcpyAsync(ctx->ec_finish_dev.p, ctx->ec_finish_host.p, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, ctx->ec_finish_copied.record(ctx->stream));
    const EcChannelDesc* dchans = reinterpret_cast<const EcChannelDesc*>(ctx->ec_finish_dev.p);
    const EcItem* ditems = reinterpret_cast<const EcItem*>(ctx->ec_finish_dev.p + sizeof(chans));
    ScopedKernelTimer t(ctx, "k_ec_finish");
    for (int k = 0; k < 4; k++) {
      if (first[k + 1] == first[k]) continue;
      const float* kernels = nullptr;
      if (k > 0) {
        if (jxlh_status st = upload_upsampling_kernels(ctx, 1 << k)) return st;  // (valid already: selects the set)
        kernels = ctx->ups_kernels.p;
      }
      launch_ec_finish(ctx->stream, 1 << k, dchans, ditems + first[k], first[k + 1] - first[k], kernels);
    }
    // a new base: the patched copy is rebuilt (whole) by the next patches launch
    ctx->frame.patch_ec_stale = true;
    for (const EcItem& it : ctx->ec_items) ctx->extra[it.ec].pat_ready = false;
  }
  for (auto& e : ctx->extra)
    if (e.set && e.rect) e.done = true;
  return JXLH_OK;
}

// What jxlh_frame_rerender_groups and jxlh_frame_repaint_groups share once the plan says "bands": the transforms (or LF
// fill) of exactly the groups of ctx->rerender_upload, then the stage list on every band.  rows: a repaint's upsampling
// and noise rows, handed over with the last band (run_post_stages); null for a re-render.
static jxlh_status rerender_listed(jxlh_ctx* ctx, const RunInputs& in, const std::vector<RowBand>& bands,
                                   const PostRepaint* rows) {
  bool sparse_k1 = false;
  if (jxlh_status st = run_prologue(ctx, false, in.stages.fused(), &sparse_k1)) return st;
  // ---- transforms of exactly the listed groups
  // a listed group whose HF has not arrived (jxlh_frame_set_groups_lf_only) is filled from the LF image again, the
  // others are transformed: the list goes up with the transforms' groups first
  int n_k1 = 0, n_fill = 0;
  if (jxlh_status st = lf_split_groups(ctx, ctx->rerender_upload, &n_k1, &n_fill)) return st;
  if (jxlh_status st = run_transforms(ctx, sparse_k1, 0, 0, true, n_k1, n_fill)) return st;
  // ---- the filters on every pixel row the listed groups influence
  static const std::vector<RowRange> none;
  const PostRepaint wait{&none, &none};
  for (size_t i = 0; i < bands.size(); i++) {
    const RowBand& b = bands[i];
    if (jxlh_status st = run_stages_rows(ctx, in.stages, b.y_lo, b.y_hi, b.whole_frame,
                                         !rows ? nullptr : i + 1 == bands.size() ? rows : &wait))
      return st;
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
  ctx->frame.strip_ran = false;
  if (plan.strip) {
    const jxlh_status st = run_strip(ctx);
    if (st != JXLH_ERR_UNSUPPORTED) return st;
    ctx->fd.strip_desc = nullptr;  // (nothing was launched) the two-kernel path takes the frame
    ctx->fd.strip_mode = nullptr;
  }
  if (jxlh_status st = run_k1(ctx, plan)) return st;
  if (plan.whole) ctx->frame.rendered = true;
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
  return rerender_listed(ctx, in, plan.bands, nullptr);
}

jxlh_status jxlh_frame_repaint_groups(jxlh_ctx* ctx, const uint32_t* group_ids, uint32_t count) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || (count && !group_ids)) return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->in_frame) return JXLH_ERR_BAD_STATE;
  if (comm_nranks(ctx) > 1) return JXLH_ERR_UNSUPPORTED;  // a rank holds only its band
  if (!ctx->modular && !ctx->tables_set) return JXLH_ERR_BAD_STATE;
  const uint32_t ncells = (uint32_t)ctx->fd.xgroups * (uint32_t)ctx->fd.ygroups;
  for (uint32_t i = 0; i < count; i++)
    if (group_ids[i] >= ncells) return JXLH_ERR_INVALID_ARGUMENT;
  if (count == 0) return JXLH_OK;
  if (jxlh_status st = patches_check_run(ctx)) return st;
  ctx->rerender_upload.assign(group_ids, group_ids + count);
  std::sort(ctx->rerender_upload.begin(), ctx->rerender_upload.end());
  ctx->rerender_upload.erase(std::unique(ctx->rerender_upload.begin(), ctx->rerender_upload.end()),
                             ctx->rerender_upload.end());
  const RunInputs in = run_inputs(ctx);
  const jxlh_frame_params& p = ctx->params;
  const int out_h = p.upsampling > 1 && p.ysize_upsampled ? (int)p.ysize_upsampled : in.ysize * std::max(1, in.upsampling);
  const RepaintPlan plan = plan_repaint(in, ctx->rerender_upload, out_h);
  if (plan.route == RepaintPlan::kWholeRun) return jxlh_frame_run(ctx, 0, UINT32_MAX);
  const PostRepaint rows{&plan.centre_rows, &plan.noise_rows};
  if (plan.route == RepaintPlan::kRerenderBands) return rerender_listed(ctx, in, plan.bands, &rows);
  // a Modular frame: the intake of every run of listed group rows, the stage list on its rows and the stage list's reach
  static const std::vector<RowRange> none;
  const PostRepaint wait{&none, &none};
  for (size_t i = 0; i < plan.runs.size(); i++)
    if (jxlh_status st = modular_frame_issue(ctx, plan.runs[i], plan.bands[i].y_lo, plan.bands[i].y_hi,
                                             i + 1 == plan.runs.size() ? &rows : &wait))
      return st;
  return JXLH_OK;
}

}  // extern "C"
