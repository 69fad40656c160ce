// C ABI, group-local Modular transforms (jxl_hip.h, jxl_hip_local_palette.h, jxl_hip_local_squeeze.h,
// jxl_hip_local_extra.h): the lowering
// entry points, and the issuer of a batch.  What a batch launches is decided by plan_local_batch (modular_local_plan.h);
// here the plan's block goes up in one copy from a pinned block, a host arena in one more, and the plan's steps are
// launched in their order.  Nothing is enqueued unless every group passed.
#include <algorithm>

#include "jxlh_ctx.h"
#include "modular_local_plan.h"

namespace jxlh_host {
namespace {

// the destination's planes; the plan knows their count and size (LocalBatchIn)
struct LocalOut {
  int32_t* out[4] = {nullptr, nullptr, nullptr, nullptr};
  size_t stride = 0;  // all planes', or (a table destination) slot 0's
  // a table destination (LocalBatchIn::dest): the planes' own strides, and where a grey slot 0 goes besides out[0]
  size_t slot_stride[4] = {0, 0, 0, 0};
  int32_t* fan[2] = {nullptr, nullptr};
  // the call's jxlh_local_dest when it names extra channels: their state is updated (mark_extra_channels) once the
  // call can no longer be refused and holds every buffer it needs, in front of the first enqueue
  const jxlh_local_dest* ec_dest = nullptr;
};

// The state of the extra channels a jxl_hip_local_extra.h call writes, per non-empty group rect: what
// jxlh_frame_set_extra_channel_rects does for a rect (abi_extra_rects.hip).  The channels' state first, so that a
// device error leaves them "not rendered".
void mark_extra_channels(jxlh_ctx* ctx, const LocalBatchIn& in, const jxlh_local_dest& dest) {
  for (size_t gi = 0; gi < in.n; gi++) {
    const jxlh_local_squeeze_group& g = in.sgroups[gi];
    if (g.w == 0 || g.h == 0) continue;
    for (uint32_t k = 0; k < dest.n_ec; k++) {
      jxlh_ctx::ExtraChannel& e = ctx->extra[dest.ec[k]];
      EcGrid& grid = ctx->ec_plan.ch[dest.ec[k]];
      if (!e.rect) {  // a whole-plane channel takes rect state: what a run finished of it stays finished
        e.rect = true;
        grid.reset(e.w, e.h, e.up);
        if (!e.done) grid.mark_all();
      }
      grid.mark(g.x0, g.y0, g.w, g.h);
      e.done = false;
    }
  }
}

jxlh_status local_enqueue(jxlh_ctx* ctx, const int32_t* arena, LocalBatchIn in, const LocalOut& d, size_t* first_bad) {
  auto at16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  bool aligned = at16(arena);
  if (in.dest) {  // alignment is a per-plane fact: the plan combines them with the strides it knows
    for (uint32_t c = 0; c < in.dest->n_slots; c++) in.plane_aligned[c] = at16(d.out[c]);
    in.fan_aligned = at16(d.fan[0]) && at16(d.fan[1]);
  } else {
    aligned = aligned && (d.stride & 3) == 0;
    for (uint32_t c = 0; c < in.n_out; c++) aligned = aligned && at16(d.out[c]);
  }
  const bool mixed = in.dest && in.dest->mixed();
  const LocalPlan plan = plan_local_batch(in, aligned);
  if (plan.status != JXLH_OK) {
    if (plan.why) {
      if (first_bad) *first_bad = plan.first_bad;
      ctx->last_error = "group " + std::to_string(plan.first_bad) + ": " + plan.why;
    }
    return plan.status;
  }
  if (plan.steps.empty()) return JXLH_OK;
  // ---- from here on the call cannot be refused for its arguments
  const size_t bytes = plan.layout.total;
  HIPCHK(ctx, ctx->local_copied.sync());  // the pinned block's previous content is on its way
  ctx->local_copied.clear();
  if (ctx->local_desc_host.n < bytes) {
    HIPCHK(ctx, ctx->local_desc_host.reset());
    HIPCHK(ctx, ctx->local_desc_host.alloc(bytes + bytes / 2));
  }
  if (jxlh_status st = ensure(ctx, ctx->local_desc, bytes)) return st;
  if (plan.scratch > 0)
    if (jxlh_status st = ensure(ctx, ctx->local_scratch, (size_t)plan.scratch)) return st;
  plan.serialize(ctx->local_desc_host.p);
  const int32_t* arena_dev = arena;
  const bool staged = !is_device_ptr(arena);
  if (staged)
    if (jxlh_status st = ensure(ctx, ctx->local_arena, (size_t)in.arena_samples)) return st;
  // ---- every buffer is held: the first enqueue follows
  if (d.ec_dest) mark_extra_channels(ctx, in, *d.ec_dest);
  if (staged) {
    // one copy; 16-byte alignment of the samples is kept (hipMalloc's and the caller's bases are both taken as they
    // are: the vector path was decided on the caller's base, so an unaligned host arena already runs the scalar path)
    HIPCHK(ctx, hipMemcpyAsync(ctx->local_arena.p, arena, (size_t)in.arena_samples * sizeof(int32_t), hipMemcpyDefault, ctx->stream));
    arena_dev = ctx->local_arena.p;
  }
  HIPCHK(ctx, hipMemcpyAsync(ctx->local_desc.p, ctx->local_desc_host.p, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, ctx->local_copied.record(ctx->stream));
  const int depth = (int)std::min(in.bit_depth, 24u);  // do_palette_step_general: bits_per_sample().min(24), palette.rs:177
  const uint8_t* block = ctx->local_desc.p;
  for (const LocalStep& s : plan.steps) {
    auto fill = [&](auto& a) {  // what every launch of the family takes
      a.arena = arena_dev;
      for (int c = 0; c < 4; c++) a.out[c] = d.out[c];
      for (int c = 0; c < 4; c++) a.slot_stride[c] = in.dest ? d.slot_stride[c] : d.stride;
      a.items = reinterpret_cast<const LocalItem*>(block + s.items.off), a.n_items = s.n_items;
    };
    if (s.kernel == LocalKernel::kLocal) {
      LocalLaunch a{};
      fill(a);
      a.groups = reinterpret_cast<const LocalGroupDev*>(block + s.desc.off);
      a.out_stride = d.stride;
      a.n_out = in.dest ? in.dest->n_slots : in.n_out, a.fan_grey = s.fan_grey, a.bit_depth = depth;
      a.mixed = mixed;
      for (int q = 0; q < 2; q++) a.fan[q] = d.fan[q];
      ScopedKernelTimer t(ctx, "k_modular_local");
      launch_modular_local(ctx->stream, a);
    } else if (s.kernel == LocalKernel::kSqueezeLds || s.kernel == LocalKernel::kSqueezeLevel) {
      const bool lds = s.kernel == LocalKernel::kSqueezeLds;
      LsLaunch a{};
      fill(a);
      a.scratch = ctx->local_scratch.p;
      a.chains = reinterpret_cast<const LsChainDev*>(block + s.desc.off);
      a.step = s.step;
      ScopedKernelTimer t(ctx, lds ? "k_modular_local_squeeze_lds" : "k_modular_local_squeeze_level");
      (lds ? launch_modular_local_squeeze_lds : launch_modular_local_squeeze_level)(ctx->stream, a);
    } else {
      const bool palette = s.kernel == LocalKernel::kPalette;
      LpLaunch a{};
      fill(a);
      a.scratch = ctx->local_scratch.p;
      a.out_stride = d.stride;
      a.bit_depth = depth;
      a.mixed = mixed;
      // where a descriptor's `fan` sends slot 0: the frame's planes 1 and 2 (unused by the stage-level calls)
      for (int q = 0; q < 2; q++) a.fan[q] = in.dest ? d.fan[q] : d.out[1 + q];
      if (palette) a.jobs = reinterpret_cast<const LpJobDev*>(block + s.desc.off), a.weighted = s.weighted, a.lds_palette = s.lds_palette;
      else a.phases = reinterpret_cast<const LpPhaseDev*>(block + s.desc.off);
      ScopedKernelTimer t(ctx, palette ? "k_modular_local_palette" : "k_modular_local_phase");
      (palette ? launch_modular_local_palette : launch_modular_local_phase)(ctx->stream, a);
    }
    // one check behind the plain launch, one behind the run of squeeze launches, one behind every phase
    const bool squeeze = s.kernel == LocalKernel::kSqueezeLds || s.kernel == LocalKernel::kSqueezeLevel;
    const LocalStep* next = &s + 1;
    if (!(squeeze && next != plan.steps.end() && next->kernel == LocalKernel::kSqueezeLevel)) HIPCHK(ctx, hipGetLastError());
  }
  return JXLH_OK;
}

// in: the call's groups; the bit depth and the destination are the frame's
jxlh_status frame_set_groups(jxlh_ctx* ctx, const int32_t* arena, LocalBatchIn in, uint32_t sample_format, size_t* first_bad,
                             bool wait) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !arena || (!in.has_groups() && in.n > 0)) return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->in_frame || !ctx->modular) return JXLH_ERR_BAD_STATE;
  const FrameDev& f = ctx->fd;
  if (f.subsampled) {
    ctx->last_error = "group-local transforms on a chroma-subsampled frame";
    return JXLH_ERR_UNSUPPORTED;
  }
  if (ctx->comm) {
    ctx->last_error = "group-local transforms on a sharded context";
    return JXLH_ERR_UNSUPPORTED;
  }
  const bool xyb = (sample_format & JXLH_MODULAR_XYB) != 0;
  const uint32_t depth = sample_format & ~(uint32_t)JXLH_MODULAR_XYB;
  if (!(xyb && depth == 0) && !bit_depth_ok(depth, 31)) return JXLH_ERR_INVALID_ARGUMENT;
  if (ctx->frame.mod_format && ctx->frame.mod_format != sample_format) return JXLH_ERR_INVALID_ARGUMENT;
  LocalOut d;
  for (int c = 0; c < 3; c++) d.out[c] = ctx->mod_src[c].p;
  d.stride = f.plane_stride;
  in.n_out = 3;
  in.w = (uint32_t)f.xsize, in.h = (uint32_t)f.ysize;
  in.frame = true;
  // the palettes' bit depth is the samples' (a palette on 32-bit float samples is refused: no bit depth of 1..31)
  in.bit_depth = depth & 0xffu;
  if (jxlh_status st = local_enqueue(ctx, arena, in, d, first_bad)) return st;
  ctx->frame.mod_format = sample_format;
  if (wait) JXLH_SYNC(ctx);
  return JXLH_OK;
}

// in: the call's groups and bit depth; the destination is `out`
jxlh_status stage_transforms(jxlh_ctx* ctx, const int32_t* arena, LocalBatchIn in, int32_t* const out[], uint32_t n_out,
                             uint32_t out_w, uint32_t out_h, size_t out_stride, size_t* first_bad) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !arena || (!in.has_groups() && in.n > 0) || !out || n_out < 1 || n_out > JXLH_LOCAL_MAX_CHANNELS || out_stride < out_w)
    return JXLH_ERR_INVALID_ARGUMENT;
  LocalOut d;
  for (uint32_t c = 0; c < n_out; c++) {
    if (!out[c] || !is_device_ptr(out[c])) return JXLH_ERR_INVALID_ARGUMENT;
    d.out[c] = out[c];
  }
  if (ctx->comm) {
    ctx->last_error = "group-local transforms on a sharded context";
    return JXLH_ERR_UNSUPPORTED;
  }
  d.stride = out_stride;
  in.n_out = n_out;
  in.w = out_w, in.h = out_h;
  if (jxlh_status st = local_enqueue(ctx, arena, in, d, first_bad)) return st;
  JXLH_SYNC(ctx);
  return JXLH_OK;
}

// jxl_hip_local_extra.h: the destination is a table over the frame's planes and its extra channels' sample stores
jxlh_status frame_set_groups_extra(jxlh_ctx* ctx, const int32_t* arena, LocalBatchIn in, uint32_t sample_format,
                                   const jxlh_local_dest* dest, size_t* first_bad, bool wait) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !arena || !dest || (!in.has_groups() && in.n > 0)) return JXLH_ERR_INVALID_ARGUMENT;
  LocalDestState state;
  state.in_frame = ctx->in_frame, state.modular = ctx->in_frame && ctx->modular;
  state.subsampled = state.modular && ctx->fd.subsampled;
  state.sharded = ctx->comm != nullptr;
  if (state.modular) {
    state.w = (uint32_t)ctx->fd.xsize, state.h = (uint32_t)ctx->fd.ysize;
    state.plane_stride = (uint32_t)ctx->fd.plane_stride;
    state.mod_format = ctx->frame.mod_format;
  }
  for (int i = 0; i < JXLH_MAX_EXTRA_CHANNELS; i++) {
    state.ec[i].set = ctx->extra[i].set;
    state.ec[i].w = ctx->extra[i].w, state.ec[i].h = ctx->extra[i].h;
  }
  const LocalDestTable table = plan_local_dest(*dest, sample_format, state);
  if (table.status != JXLH_OK) {
    ctx->last_error = std::string("jxlh_frame_set_modular_groups_extra: ") + table.why;
    return table.status;
  }
  LocalOut d;
  for (uint32_t c = 0; c < table.n_slots; c++) {
    const uint32_t plane = table.slot[c].plane;
    d.out[c] = plane >= kLocalPlaneExtra ? ctx->extra[plane - kLocalPlaneExtra].raw.p : ctx->mod_src[plane - kLocalPlaneColour].p;
    d.slot_stride[c] = table.slot[c].stride;
  }
  d.stride = d.slot_stride[0];
  if (table.fan) {
    d.fan[0] = ctx->mod_src[1].p, d.fan[1] = ctx->mod_src[2].p;
    // grey alone (1 + 0) runs the kernels of the frame form, whose fan-out stores through planes 1 and 2 of `out`
    if (!table.mixed()) d.out[1] = d.fan[0], d.out[2] = d.fan[1];
  }
  in.dest = &table;
  in.bit_depth = table.bit_depth;
  if (dest->n_ec > 0) d.ec_dest = dest;
  if (jxlh_status st = local_enqueue(ctx, arena, in, d, first_bad)) return st;
  if (table.n_colour > 0) ctx->frame.mod_format = sample_format;
  if (wait) JXLH_SYNC(ctx);
  return JXLH_OK;
}

// the three forms of a call, without the destination
LocalBatchIn plain_in(LocalBatchIn::Form form, const jxlh_local_group* groups, const jxlh_wp_header* wp, size_t n,
                      uint32_t bit_depth, uint64_t arena_samples) {
  LocalBatchIn in;
  in.form = form, in.groups = groups, in.wp = wp, in.n = n;
  in.bit_depth = bit_depth, in.arena_samples = arena_samples;
  return in;
}
LocalBatchIn squeeze_in(const jxlh_local_squeeze_group* groups, size_t n, const jxlh_local_coded_channel* coded, size_t n_coded,
                        const jxlh_squeeze_params* params, size_t n_params, const jxlh_wp_header* wp, uint32_t bit_depth,
                        uint64_t arena_samples) {
  LocalBatchIn in;
  in.form = LocalBatchIn::kSqueeze, in.sgroups = groups, in.n = n;
  in.coded = coded, in.n_coded = n_coded, in.params = params, in.n_params = n_params;
  in.wp = wp, in.bit_depth = bit_depth, in.arena_samples = arena_samples;
  return in;
}

// two passes, so that a refused call leaves `programs` as it was; one(g, program or null) lowers group g
template <class Program, class LowerOne>
jxlh_status lower_each(size_t n, Program* programs, size_t* first_bad, LowerOne one) {
  for (int pass = 0; pass < (programs ? 2 : 1); pass++) {
    for (size_t g = 0; g < n; g++) {
      if (jxlh_status st = one(g, pass ? &programs[g] : nullptr)) {
        if (first_bad) *first_bad = g;
        return st;
      }
    }
  }
  return JXLH_OK;
}

}  // namespace

}  // namespace jxlh_host

extern "C" {

jxlh_status jxlh_modular_local_lower(const jxlh_local_group* groups, size_t n, uint32_t bit_depth, uint64_t arena_samples,
                                     jxlh_local_program* programs, size_t* first_bad) {
  if (!groups && n > 0) return JXLH_ERR_INVALID_ARGUMENT;
  return jxlh_host::lower_each(n, programs, first_bad, [&](size_t g, jxlh_local_program* p) {
    return jxlh::local_lower_group(groups[g], bit_depth, arena_samples, p, nullptr);
  });
}

jxlh_status jxlh_modular_local_lower_general(const jxlh_local_group* groups, const jxlh_wp_header* wp, size_t n,
                                             uint32_t bit_depth, uint64_t arena_samples,
                                             jxlh_local_general_program* programs, size_t* first_bad) {
  if (!groups && n > 0) return JXLH_ERR_INVALID_ARGUMENT;
  return jxlh_host::lower_each(n, programs, first_bad, [&](size_t g, jxlh_local_general_program* p) {
    return jxlh::local_lower_core(groups[g], bit_depth, arena_samples, true, wp ? &wp[g] : nullptr, nullptr, p, nullptr);
  });
}

jxlh_status jxlh_modular_local_transforms(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                          const jxlh_local_group* groups, size_t n, uint32_t bit_depth, int32_t* const out[],
                                          uint32_t n_out, uint32_t out_w, uint32_t out_h, size_t out_stride,
                                          size_t* first_bad) {
  return jxlh_host::stage_transforms(ctx, arena, jxlh_host::plain_in(jxlh::LocalBatchIn::kPlain, groups, nullptr, n, bit_depth, arena_samples),
                                     out, n_out, out_w, out_h, out_stride, first_bad);
}

jxlh_status jxlh_modular_local_transforms_general(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                                  const jxlh_local_group* groups, const jxlh_wp_header* wp, size_t n,
                                                  uint32_t bit_depth, int32_t* const out[], uint32_t n_out, uint32_t out_w,
                                                  uint32_t out_h, size_t out_stride, size_t* first_bad) {
  return jxlh_host::stage_transforms(ctx, arena, jxlh_host::plain_in(jxlh::LocalBatchIn::kGeneral, groups, wp, n, bit_depth, arena_samples),
                                     out, n_out, out_w, out_h, out_stride, first_bad);
}

jxlh_status jxlh_frame_set_modular_groups(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                          const jxlh_local_group* groups, size_t n, uint32_t sample_format,
                                          size_t* first_bad) {
  return jxlh_host::frame_set_groups(ctx, arena, jxlh_host::plain_in(jxlh::LocalBatchIn::kPlain, groups, nullptr, n, 0, arena_samples),
                                     sample_format, first_bad, true);
}

jxlh_status jxlh_frame_set_modular_groups_async(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                                const jxlh_local_group* groups, size_t n, uint32_t sample_format,
                                                size_t* first_bad) {
  return jxlh_host::frame_set_groups(ctx, arena, jxlh_host::plain_in(jxlh::LocalBatchIn::kPlain, groups, nullptr, n, 0, arena_samples),
                                     sample_format, first_bad, false);
}

jxlh_status jxlh_frame_set_modular_groups_general(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                                  const jxlh_local_group* groups, const jxlh_wp_header* wp, size_t n,
                                                  uint32_t sample_format, size_t* first_bad) {
  return jxlh_host::frame_set_groups(ctx, arena, jxlh_host::plain_in(jxlh::LocalBatchIn::kGeneral, groups, wp, n, 0, arena_samples),
                                     sample_format, first_bad, true);
}

jxlh_status jxlh_frame_set_modular_groups_general_async(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                                        const jxlh_local_group* groups, const jxlh_wp_header* wp, size_t n,
                                                        uint32_t sample_format, size_t* first_bad) {
  return jxlh_host::frame_set_groups(ctx, arena, jxlh_host::plain_in(jxlh::LocalBatchIn::kGeneral, groups, wp, n, 0, arena_samples),
                                     sample_format, first_bad, false);
}

jxlh_status jxlh_modular_local_default_squeeze(const uint32_t* w, const uint32_t* h, uint32_t n, uint32_t n_meta,
                                               jxlh_squeeze_params* params, uint32_t cap, uint32_t* n_params) {
  if (!w || !h || !n_params || n < 1 || n > JXLH_LOCAL_MAX_CHANNELS || (!params && cap > 0)) return JXLH_ERR_INVALID_ARGUMENT;
  *n_params = jxlh::default_squeeze_list(w, h, n, n_meta, params, cap);
  return *n_params > cap ? JXLH_ERR_INVALID_ARGUMENT : JXLH_OK;
}

jxlh_status jxlh_modular_local_lower_squeeze(const jxlh_local_squeeze_group* groups, size_t n,
                                             const jxlh_local_coded_channel* coded, size_t n_coded,
                                             const jxlh_squeeze_params* params, size_t n_params, const jxlh_wp_header* wp,
                                             uint32_t bit_depth, uint64_t arena_samples,
                                             jxlh_local_squeeze_program* programs, size_t* first_bad) {
  if (!groups && n > 0) return JXLH_ERR_INVALID_ARGUMENT;
  return jxlh_host::lower_each(n, programs, first_bad, [&](size_t g, jxlh_local_squeeze_program* p) {
    return jxlh::local_lower_squeeze_group(groups[g], coded, n_coded, params, n_params, wp ? &wp[g] : nullptr, bit_depth,
                                           arena_samples, p, nullptr);
  });
}

jxlh_status jxlh_modular_local_transforms_squeeze(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                                  const jxlh_local_squeeze_group* groups, size_t n,
                                                  const jxlh_local_coded_channel* coded, size_t n_coded,
                                                  const jxlh_squeeze_params* params, size_t n_params,
                                                  const jxlh_wp_header* wp, uint32_t bit_depth, int32_t* const out[],
                                                  uint32_t n_out, uint32_t out_w, uint32_t out_h, size_t out_stride,
                                                  size_t* first_bad) {
  return jxlh_host::stage_transforms(ctx, arena, jxlh_host::squeeze_in(groups, n, coded, n_coded, params, n_params, wp, bit_depth, arena_samples),
                                     out, n_out, out_w, out_h, out_stride, first_bad);
}

jxlh_status jxlh_frame_set_modular_groups_squeeze(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                                  const jxlh_local_squeeze_group* groups, size_t n,
                                                  const jxlh_local_coded_channel* coded, size_t n_coded,
                                                  const jxlh_squeeze_params* params, size_t n_params,
                                                  const jxlh_wp_header* wp, uint32_t sample_format, size_t* first_bad) {
  return jxlh_host::frame_set_groups(ctx, arena, jxlh_host::squeeze_in(groups, n, coded, n_coded, params, n_params, wp, 0, arena_samples),
                                     sample_format, first_bad, true);
}

jxlh_status jxlh_frame_set_modular_groups_squeeze_async(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                                        const jxlh_local_squeeze_group* groups, size_t n,
                                                        const jxlh_local_coded_channel* coded, size_t n_coded,
                                                        const jxlh_squeeze_params* params, size_t n_params,
                                                        const jxlh_wp_header* wp, uint32_t sample_format,
                                                        size_t* first_bad) {
  return jxlh_host::frame_set_groups(ctx, arena, jxlh_host::squeeze_in(groups, n, coded, n_coded, params, n_params, wp, 0, arena_samples),
                                     sample_format, first_bad, false);
}

jxlh_status jxlh_frame_set_modular_groups_extra(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                                const jxlh_local_squeeze_group* groups, size_t n,
                                                const jxlh_local_coded_channel* coded, size_t n_coded,
                                                const jxlh_squeeze_params* params, size_t n_params,
                                                const jxlh_wp_header* wp, uint32_t sample_format,
                                                const jxlh_local_dest* dest, size_t* first_bad) {
  return jxlh_host::frame_set_groups_extra(ctx, arena, jxlh_host::squeeze_in(groups, n, coded, n_coded, params, n_params, wp, 0, arena_samples),
                                           sample_format, dest, first_bad, true);
}

jxlh_status jxlh_frame_set_modular_groups_extra_async(jxlh_ctx* ctx, const int32_t* arena, uint64_t arena_samples,
                                                      const jxlh_local_squeeze_group* groups, size_t n,
                                                      const jxlh_local_coded_channel* coded, size_t n_coded,
                                                      const jxlh_squeeze_params* params, size_t n_params,
                                                      const jxlh_wp_header* wp, uint32_t sample_format,
                                                      const jxlh_local_dest* dest, size_t* first_bad) {
  return jxlh_host::frame_set_groups_extra(ctx, arena, jxlh_host::squeeze_in(groups, n, coded, n_coded, params, n_params, wp, 0, arena_samples),
                                           sample_format, dest, first_bad, false);
}

}  // extern "C"
