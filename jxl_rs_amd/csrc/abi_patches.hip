// C ABI of the patches stage: the reference-frame slots of a context, the frame's patch dictionary (validated like
// PatchesDictionary::read, jxl/src/features/patches.rs:362-620, and binned into tiles once), the stage hook, and the
// piece of the frame pipeline that launches k_patches (run_post_stages, frame_run.hip).
#include <algorithm>

#include "blend_device.h"
#include "jxlh_ctx.h"

namespace jxlh_host {

namespace {

constexpr int kTileW = 64, kTileH = 4;

bool uses_alpha(uint32_t mode) {  // PatchBlendMode::uses_alpha (patches.rs:111-119)
  return mode == kBlendAbove || mode == kBlendBelow || mode == kBlendAddAbove || mode == kBlendAddBelow;
}

// The dictionary's patches binned into the 64 x 4 tiles of a w x h image: the tiles some patch touches (ascending id),
// each with its patches in definition order -- the order of application (set_patches_for_row's final sort,
// patches.rs:676-679).  Patches are clipped to the image.
jxlh_status build_bins(jxlh_ctx* ctx, jxlh_ctx::PatchBins& b, int w, int h) {
  b.w = w;
  b.h = h;
  b.ntx = (w + kTileW - 1) / kTileW;
  b.nty = (h + kTileH - 1) / kTileH;
  const size_t nt = (size_t)b.ntx * b.nty;
  std::vector<uint32_t> pos(nt + 1, 0);  // per tile: entries, then (prefix) where its entries go
  auto tile_span = [&](const PatchDev& d, int* tx0, int* tx1, int* ty0, int* ty1) {
    const int x1 = std::min(w, d.x + d.w), y1 = std::min(h, d.y + d.h);
    if (d.x >= x1 || d.y >= y1) return false;
    *tx0 = d.x / kTileW;
    *tx1 = (x1 - 1) / kTileW + 1;
    *ty0 = d.y / kTileH;
    *ty1 = (y1 - 1) / kTileH + 1;
    return true;
  };
  size_t entries = 0;
  for (const PatchDev& d : ctx->patch_desc_host) {
    int tx0, tx1, ty0, ty1;
    if (!tile_span(d, &tx0, &tx1, &ty0, &ty1)) continue;
    for (int ty = ty0; ty < ty1; ty++)
      for (int tx = tx0; tx < tx1; tx++) pos[(size_t)ty * b.ntx + tx]++;
    entries += (size_t)(tx1 - tx0) * (ty1 - ty0);
  }
  if (entries >= (1ull << 31)) return JXLH_ERR_UNSUPPORTED;
  uint32_t ntiles = 0;
  for (size_t t = 0; t < nt; t++) ntiles += pos[t] != 0;
  b.ntiles = ntiles;
  b.words.assign((size_t)2 * ntiles + 1 + entries, 0);
  uint32_t* tiles = b.words.data();
  uint32_t* start = tiles + ntiles;
  uint32_t* list = start + ntiles + 1;
  b.row_first.assign((size_t)b.nty + 1, ntiles);
  uint32_t k = 0, at = 0;
  for (size_t t = 0; t < nt; t++) {
    const uint32_t c = pos[t];
    if (!c) continue;
    const int ty = (int)(t / b.ntx);
    if (b.row_first[ty] == ntiles) b.row_first[ty] = k;
    tiles[k] = (uint32_t)t;
    start[k] = at;
    pos[t] = at;  // next free entry of tile t
    at += c;
    k++;
  }
  start[ntiles] = at;
  for (int r = b.nty - 1; r >= 0; r--)  // rows without a listed tile start where the next row does
    if (b.row_first[r] == ntiles || b.row_first[r] > b.row_first[r + 1]) b.row_first[r] = b.row_first[r + 1];
  for (uint32_t i = 0; i < (uint32_t)ctx->patch_desc_host.size(); i++) {
    int tx0, tx1, ty0, ty1;
    if (!tile_span(ctx->patch_desc_host[i], &tx0, &tx1, &ty0, &ty1)) continue;
    for (int ty = ty0; ty < ty1; ty++)
      for (int tx = tx0; tx < tx1; tx++) list[pos[(size_t)ty * b.ntx + tx]++] = i;
  }
  if (jxlh_status st = ensure(ctx, b.dev, b.words.size())) return st;
  HIPCHK(ctx, hipMemcpyAsync(b.dev.p, b.words.data(), b.words.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                             ctx->stream));
  return JXLH_OK;
}

// the slots the dictionary reads still hold what it was checked against
bool slots_ok(const jxlh_ctx* ctx) {
  for (int s = 0; s < JXLH_MAX_REFERENCE_FRAMES; s++) {
    if (!(ctx->frame.patch_slots_used >> s & 1u)) continue;
    const jxlh_ctx::RefSlot& r = ctx->refs[s];
    if (!r.set || r.n_channels != 3 + ctx->frame.patch_nec || r.w < ctx->frame.patch_need_w[s] || r.h < ctx->frame.patch_need_h[s])
      return false;
  }
  return true;
}

void fill_refs(const jxlh_ctx* ctx, PatchLaunch& a) {
  for (int s = 0; s < JXLH_MAX_REFERENCE_FRAMES; s++) {
    const jxlh_ctx::RefSlot& r = ctx->refs[s];
    a.ref[s] = r.set ? r.buf.p : nullptr;
    a.ref_plane[s] = r.set ? r.stride * r.h : 0;
    a.ref_stride[s] = r.set ? (uint32_t)r.stride : 0;
  }
}

// tiles of the listed set that cover rows [y0, y1): [first, last)
void tile_range(const jxlh_ctx::PatchBins& b, int y0, int y1, uint32_t* first, uint32_t* last) {
  y0 = std::max(0, y0);
  y1 = std::min(b.h, y1);
  if (y0 >= y1) {
    *first = *last = 0;
    return;
  }
  *first = b.row_first[y0 / kTileH];
  *last = b.row_first[(y1 - 1) / kTileH + 1];
}

void launch_bins(jxlh_ctx* ctx, const jxlh_ctx::PatchBins& b, PatchLaunch& a, int y0, int y1) {
  uint32_t first, last;
  tile_range(b, y0, y1, &first, &last);
  if (first >= last) return;
  a.ntx = b.ntx;
  a.tile0 = first;
  const uint32_t* tiles = b.dev.p;
  ScopedKernelTimer t(ctx, "k_patches");
  launch_patches(ctx->stream, (int)ctx->frame.patch_nec, a, last - first, tiles, tiles + b.ntiles, tiles + 2 * b.ntiles + 1,
                 ctx->patch_desc.p);
}

const float* ec_base(const jxlh_ctx::ExtraChannel& e) { return e.up > 1 ? e.out.p : e.f32.p; }

}  // namespace

jxlh_status patches_check_run(const jxlh_ctx* ctx) {
  if (ctx->frame.patch_n == 0) return JXLH_OK;
  if (!slots_ok(ctx)) return JXLH_ERR_BAD_STATE;
  // the dictionary's extra channels are exactly the ones handed over, each covering the whole frame
  for (uint32_t i = 0; i < JXLH_MAX_EXTRA_CHANNELS; i++) {
    const jxlh_ctx::ExtraChannel& e = ctx->extra[i];
    if (e.set != (i < ctx->frame.patch_nec)) return JXLH_ERR_BAD_STATE;
    if (e.set && (std::min(e.w * e.up, (uint32_t)ctx->fd.xsize) != (uint32_t)ctx->fd.xsize ||
                  std::min(e.h * e.up, (uint32_t)ctx->fd.ysize) != (uint32_t)ctx->fd.ysize))
      return JXLH_ERR_BAD_STATE;
  }
  return JXLH_OK;
}

jxlh_status run_patches(jxlh_ctx* ctx, float* const cur[3], size_t stride, int y_lo, int y_hi) {
  PatchLaunch a{};
  for (int c = 0; c < 3; c++) a.col[c] = cur[c];
  a.col_stride = stride;
  a.w = ctx->fd.xsize;
  a.h = ctx->fd.ysize;
  a.cy0 = y_lo;
  a.cy1 = y_hi;
  a.ec_alpha = ctx->frame.patch_ec_alpha;
  a.ec_assoc = ctx->frame.patch_ec_assoc;
  fill_refs(ctx, a);
  const bool ec_rebuild = ctx->frame.patch_nec > 0 && ctx->frame.patch_ec_stale;
  for (uint32_t i = 0; i < ctx->frame.patch_nec; i++) {
    jxlh_ctx::ExtraChannel& e = ctx->extra[i];
    const size_t n = e.out_stride * e.out_h;
    if (ec_rebuild) {  // the patched plane starts as a copy of the channel; the kernel writes the covered pixels
      if (jxlh_status st = ensure(ctx, e.pat, n)) return st;
      HIPCHK(ctx, hipMemcpyAsync(e.pat.p, ec_base(e), n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    }
    a.ec_in[i] = ec_base(e);
    a.ec_out[i] = e.pat.p;
    a.ec_stride[i] = (uint32_t)e.out_stride;
  }
  a.ey0 = 0;
  a.ey1 = ec_rebuild ? a.h : 0;
  const int r0 = ec_rebuild ? 0 : y_lo, r1 = ec_rebuild ? a.h : y_hi;
  launch_bins(ctx, ctx->patch_bins, a, r0, r1);
  HIPCHK(ctx, hipGetLastError());
  if (ec_rebuild) {
    ctx->frame.patch_ec_stale = false;
    for (uint32_t i = 0; i < ctx->frame.patch_nec; i++) ctx->extra[i].pat_ready = true;
  }
  return JXLH_OK;
}

}  // namespace jxlh_host

extern "C" {

jxlh_status jxlh_ctx_set_reference(jxlh_ctx* ctx, uint32_t slot, uint32_t n_channels, uint32_t w, uint32_t h,
                                   const float* const* planes, size_t stride) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || slot >= JXLH_MAX_REFERENCE_FRAMES || n_channels < 3 || n_channels > 3 + JXLH_MAX_EXTRA_CHANNELS ||
      w == 0 || h == 0 || !planes || stride < w)
    return JXLH_ERR_INVALID_ARGUMENT;
  for (uint32_t c = 0; c < n_channels; c++)
    if (!planes[c]) return JXLH_ERR_INVALID_ARGUMENT;
  if ((uint64_t)w * h >= (1ull << 31)) return JXLH_ERR_UNSUPPORTED;
  jxlh_ctx::RefSlot& r = ctx->refs[slot];
  const size_t dstride = round_up(w, 64);
  if (jxlh_status st = ensure(ctx, r.buf, dstride * h * n_channels)) return st;
  for (uint32_t c = 0; c < n_channels; c++)
    if (jxlh_status st = copy2d(ctx, r.buf.p + c * dstride * h, dstride * sizeof(float), planes[c],
                                stride * sizeof(float), (size_t)w * sizeof(float), h, ctx->stream))
      return st;
  JXLH_SYNC(ctx);  // the caller's planes may be reused as soon as the call returns
  r.set = true;
  r.n_channels = n_channels;
  r.w = w;
  r.h = h;
  r.stride = dstride;
  return JXLH_OK;
}

jxlh_status jxlh_frame_save_reference(jxlh_ctx* ctx, uint32_t slot) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || slot >= JXLH_MAX_REFERENCE_FRAMES) return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->in_frame || !ctx->frame.rendered || !ctx->frame.result[0]) return JXLH_ERR_BAD_STATE;
  materialise_chroma(ctx);
  const uint32_t w = (uint32_t)ctx->res_w, h = (uint32_t)ctx->res_h;
  if (blended(ctx)) {  // the composed image (jxlh_frame_blend): the canvas has the slot's layout, one linear copy
    jxlh_ctx::RefSlot& r = ctx->refs[slot];
    const uint32_t nch = 3 + ctx->frame.blend_nec;
    const size_t n = ctx->res_stride * h * nch;
    if (jxlh_status st = ensure(ctx, r.buf, n)) return st;
    HIPCHK(ctx, hipMemcpyAsync(r.buf.p, ctx->blend_canvas.p, n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    r.set = true;
    r.n_channels = nch;
    r.w = w;
    r.h = h;
    r.stride = ctx->res_stride;
    return JXLH_OK;
  }
  // the extra channels handed over: 0 .. nec - 1, converted, at the result's size
  uint32_t nec = 0;
  while (nec < JXLH_MAX_EXTRA_CHANNELS && ctx->extra[nec].set) nec++;
  for (uint32_t i = nec; i < JXLH_MAX_EXTRA_CHANNELS; i++)
    if (ctx->extra[i].set) return JXLH_ERR_UNSUPPORTED;
  for (uint32_t i = 0; i < nec; i++) {
    const jxlh_ctx::ExtraChannel& e = ctx->extra[i];
    if (!e.done) return JXLH_ERR_BAD_STATE;
    if (e.out_w != w || e.out_h != h) return JXLH_ERR_UNSUPPORTED;
  }
  jxlh_ctx::RefSlot& r = ctx->refs[slot];
  const size_t dstride = round_up(w, 64);
  const uint32_t nch = 3 + nec;
  if (jxlh_status st = ensure(ctx, r.buf, dstride * h * nch)) return st;
  for (uint32_t c = 0; c < nch; c++) {
    const float* src;
    size_t sstride;
    if (c < 3) {
      src = ctx->frame.result[c];
      sstride = ctx->res_stride;
    } else {
      const jxlh_ctx::ExtraChannel& e = ctx->extra[c - 3];
      src = e.pat_ready ? e.pat.p : ec_base(e);
      sstride = e.out_stride;
    }
    HIPCHK(ctx, hipMemcpy2DAsync(r.buf.p + c * dstride * h, dstride * sizeof(float), src, sstride * sizeof(float),
                                 (size_t)w * sizeof(float), h, hipMemcpyDeviceToDevice, ctx->stream));
  }
  r.set = true;
  r.n_channels = nch;
  r.w = w;
  r.h = h;
  r.stride = dstride;
  return JXLH_OK;
}

jxlh_status jxlh_ctx_clear_reference(jxlh_ctx* ctx, uint32_t slot) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || slot >= JXLH_MAX_REFERENCE_FRAMES) return JXLH_ERR_INVALID_ARGUMENT;
  jxlh_ctx::RefSlot& r = ctx->refs[slot];
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // (a queued patches launch may still read the slot)
  (void)r.buf.reset();
  r = jxlh_ctx::RefSlot{};
  return JXLH_OK;
}

jxlh_status jxlh_frame_set_patches(jxlh_ctx* ctx, const jxlh_patch* patches, uint32_t n,
                                   const jxlh_patch_blending* blendings, uint32_t num_ec, const uint32_t* ec_flags) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx) return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->in_frame) return JXLH_ERR_BAD_STATE;
  if (n > 0 && (!patches || !blendings || num_ec > JXLH_MAX_EXTRA_CHANNELS || (num_ec > 0 && !ec_flags)))
    return JXLH_ERR_INVALID_ARGUMENT;
  if (n > 0) {
    // extra channels handed over so far: the dictionary must cover exactly them
    uint32_t handed = 0, top = 0;
    for (uint32_t i = 0; i < JXLH_MAX_EXTRA_CHANNELS; i++)
      if (ctx->extra[i].set) {
        handed++;
        top = i + 1;
      }
    if (handed > 0 && (handed != top || handed != num_ec)) return JXLH_ERR_INVALID_ARGUMENT;
    if (num_ec > 0 && ctx->params.upsampling > 1) return JXLH_ERR_UNSUPPORTED;
    // FrameHeader::size_padded (frame_header.rs:572-581) as frame/decode.rs:317-323 passes it: whole 8x8 blocks for a
    // VarDCT frame, the coded size for a Modular one (:574-575)
    const uint64_t pw = ctx->modular ? (uint64_t)ctx->fd.xsize : (uint64_t)ctx->fd.xblocks * 8,
                   ph = ctx->modular ? (uint64_t)ctx->fd.ysize : (uint64_t)ctx->fd.yblocks * 8;
    const uint32_t stride = 1 + num_ec;
    for (uint32_t i = 0; i < n; i++) {
      const jxlh_patch& p = patches[i];
      if (p.ref_slot >= JXLH_MAX_REFERENCE_FRAMES || p.xsize == 0 || p.ysize == 0) return JXLH_ERR_INVALID_ARGUMENT;
      const jxlh_ctx::RefSlot& r = ctx->refs[p.ref_slot];
      if (!r.set || r.n_channels != 3 + num_ec) return JXLH_ERR_INVALID_ARGUMENT;
      if ((uint64_t)p.ref_x0 + p.xsize > r.w || (uint64_t)p.ref_y0 + p.ysize > r.h) return JXLH_ERR_INVALID_ARGUMENT;
      if ((uint64_t)p.x + p.xsize > pw || (uint64_t)p.y + p.ysize > ph) return JXLH_ERR_INVALID_ARGUMENT;
      for (uint32_t k = 0; k < stride; k++) {
        const jxlh_patch_blending& b = blendings[(size_t)i * stride + k];
        if (b.mode >= 8) return JXLH_ERR_INVALID_ARGUMENT;
        // read from the stream only for a mode that uses alpha and more than one extra channel (patches.rs:585-596)
        if (uses_alpha(b.mode) && num_ec > 1 && b.alpha_channel >= num_ec) return JXLH_ERR_INVALID_ARGUMENT;
      }
    }
  }
  // checked: nothing below fails on the arguments
  ctx->frame.patch_n = 0;
  ctx->frame.patch_nec = 0;
  ctx->frame.patch_slots_used = 0;
  ctx->frame.patch_ec_stale = true;
  for (auto& e : ctx->extra) e.pat_ready = false;
  ctx->patch_desc_host.clear();
  if (n == 0) return JXLH_OK;
  const uint32_t stride = 1 + num_ec;
  ctx->patch_desc_host.resize(n);
  for (int s = 0; s < JXLH_MAX_REFERENCE_FRAMES; s++) ctx->frame.patch_need_w[s] = ctx->frame.patch_need_h[s] = 0;
  for (uint32_t i = 0; i < n; i++) {
    const jxlh_patch& p = patches[i];
    PatchDev& d = ctx->patch_desc_host[i];
    d = PatchDev{};
    d.x = (int)p.x;
    d.y = (int)p.y;
    d.w = (int)p.xsize;
    d.h = (int)p.ysize;
    d.rx = (int)p.ref_x0;
    d.ry = (int)p.ref_y0;
    d.slot = (int)p.ref_slot;
    for (uint32_t k = 0; k < stride; k++) {
      const jxlh_patch_blending& b = blendings[(size_t)i * stride + k];
      // alpha_channel is read from the stream only for a mode that uses it and more than one extra channel: 0 otherwise
      const uint32_t alpha = uses_alpha(b.mode) && num_ec > 1 ? b.alpha_channel : 0;
      d.blend[k] = pack_blending(b.mode, alpha, b.clamp != 0);
    }
    ctx->frame.patch_slots_used |= 1u << p.ref_slot;
    ctx->frame.patch_need_w[p.ref_slot] = std::max(ctx->frame.patch_need_w[p.ref_slot], p.ref_x0 + p.xsize);
    ctx->frame.patch_need_h[p.ref_slot] = std::max(ctx->frame.patch_need_h[p.ref_slot], p.ref_y0 + p.ysize);
  }
  ctx->frame.patch_ec_alpha = ctx->frame.patch_ec_assoc = 0;
  for (uint32_t k = 0; k < num_ec; k++) {
    if (ec_flags[k] & JXLH_EC_ALPHA) ctx->frame.patch_ec_alpha |= 1u << k;
    if (ec_flags[k] & JXLH_EC_ALPHA_ASSOCIATED) ctx->frame.patch_ec_assoc |= 1u << k;
  }
  if (jxlh_status st = ensure(ctx, ctx->patch_desc, n)) return st;
  HIPCHK(ctx, hipMemcpyAsync(ctx->patch_desc.p, ctx->patch_desc_host.data(), n * sizeof(PatchDev),
                             hipMemcpyHostToDevice, ctx->stream));
  if (jxlh_status st = build_bins(ctx, ctx->patch_bins, ctx->fd.xsize, ctx->fd.ysize)) return st;
  ctx->patch_hook_bins.w = ctx->patch_hook_bins.h = 0;  // (binned again for the next stage-hook size)
  JXLH_SYNC(ctx);  // the host copies may change with the next call
  ctx->frame.patch_n = n;
  ctx->frame.patch_nec = num_ec;
  return JXLH_OK;
}

jxlh_status jxlh_stage_patches(jxlh_ctx* ctx, float* const planes[], uint32_t n_channels, uint32_t w, uint32_t h,
                               size_t stride) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !planes || w == 0 || h == 0 || stride < w) return JXLH_ERR_INVALID_ARGUMENT;
  if (ctx->frame.patch_n == 0) return n_channels >= 3 ? JXLH_OK : JXLH_ERR_INVALID_ARGUMENT;
  if (n_channels != 3 + ctx->frame.patch_nec) return JXLH_ERR_INVALID_ARGUMENT;
  for (uint32_t c = 0; c < n_channels; c++)
    if (!planes[c]) return JXLH_ERR_INVALID_ARGUMENT;
  if ((uint64_t)stride * h >= (1ull << 31)) return JXLH_ERR_UNSUPPORTED;
  if (!slots_ok(ctx)) return JXLH_ERR_BAD_STATE;
  jxlh_ctx::PatchBins* b = &ctx->patch_bins;
  if (b->w != (int)w || b->h != (int)h) {
    b = &ctx->patch_hook_bins;
    if (b->w != (int)w || b->h != (int)h)
      if (jxlh_status st = build_bins(ctx, *b, (int)w, (int)h)) return st;
  }
  const size_t plane = stride * h;
  if (jxlh_status st = ensure(ctx, ctx->patch_hook, plane * n_channels)) return st;
  float* hp = ctx->patch_hook.p;
  for (uint32_t c = 0; c < n_channels; c++)
    if (jxlh_status st = copy2d(ctx, hp + c * plane, stride * sizeof(float), planes[c], stride * sizeof(float),
                                (size_t)w * sizeof(float), h, ctx->stream))
      return st;
  PatchLaunch a{};
  for (int c = 0; c < 3; c++) a.col[c] = hp + c * plane;
  a.col_stride = stride;
  for (uint32_t i = 0; i < ctx->frame.patch_nec; i++) {
    a.ec_in[i] = a.ec_out[i] = hp + (3 + i) * plane;
    a.ec_stride[i] = (uint32_t)stride;
  }
  a.w = (int)w;
  a.h = (int)h;
  a.cy0 = a.ey0 = 0;
  a.cy1 = a.ey1 = (int)h;
  a.ec_alpha = ctx->frame.patch_ec_alpha;
  a.ec_assoc = ctx->frame.patch_ec_assoc;
  fill_refs(ctx, a);
  launch_bins(ctx, *b, a, 0, (int)h);
  HIPCHK(ctx, hipGetLastError());
  for (uint32_t c = 0; c < n_channels; c++)
    if (jxlh_status st = copy2d(ctx, planes[c], stride * sizeof(float), hp + c * plane, stride * sizeof(float),
                                (size_t)w * sizeof(float), h, ctx->stream))
      return st;
  JXLH_SYNC(ctx);
  return JXLH_OK;
}

}  // extern "C"
