// Multi-GPU entry points of the C ABI (include/jxl_hip.h, "multi-GPU" section).
//
// Partitioning (reference join point frame/render.rs:461-479): a frame is cut into contiguous bands
// of group rows, one band per rank; a rank runs the transforms (K1) on exactly its band, receives the block row its
// filters read across each band edge from the neighbour rank (halo EXCHANGE: one 8-pixel block row x 3 channels per
// edge, 0.8 MB at 8K -- not a recomputed group row), filters its band, and the finished bands are all-gathered so
// that every rank holds the whole frame.
//
// Two transports behind the same band logic:
//   RCCL   one process per GPU (torch.distributed.run / MPI style launch): the library owns an RCCL communicator
//          (ncclCommInitRank from a 128-byte id the caller distributes out of band); halo = grouped ncclSend/ncclRecv,
//          gather = in-place ncclAllGather per plane, all enqueued on the context's stream.  librccl is opened with
//          dlopen on first use, so a single-GPU deployment has no dependency on it.
//   local  the peers are contexts of ONE process (several GPUs driven by one decoder process, or -- for tests --
//          several contexts on one GPU): direct device-to-device copies ordered by events.
#include <dlfcn.h>

#include <chrono>
#include <cstdlib>
#include <thread>
#include <rccl/rccl.h>  // types and enums only: every function is resolved at run time

#include "jxlh_ctx.h"

namespace jxlh_host {

struct RcclApi {
  void* handle = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  ncclResult_t (*CommGetAsyncError)(ncclComm_t, ncclResult_t*) = nullptr;  // optional
  ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;                          // optional
};

static RcclApi* rccl_api(std::string* err) {
  static RcclApi api;
  static std::mutex m;
  std::lock_guard<std::mutex> lock(m);
  if (api.handle) return &api;
  // a copy another component of the process already loaded (PyTorch ships one) is reused through its soname
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  void* h = nullptr;
  for (const char* n : names) {
    h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
    if (h) break;
  }
  if (!h) {
    if (err) *err = std::string("dlopen librccl: ") + dlerror();
    return nullptr;
  }
  bool ok = true;
  auto sym = [&](const char* name) {
    void* p = dlsym(h, name);
    if (!p) {
      ok = false;
      if (err) *err = std::string("librccl lacks ") + name;
    }
    return p;
  };
  api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(sym("ncclGetUniqueId"));
  api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(sym("ncclCommInitRank"));
  api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(sym("ncclCommDestroy"));
  api.AllGather = reinterpret_cast<decltype(api.AllGather)>(sym("ncclAllGather"));
  api.Send = reinterpret_cast<decltype(api.Send)>(sym("ncclSend"));
  api.Recv = reinterpret_cast<decltype(api.Recv)>(sym("ncclRecv"));
  api.GroupStart = reinterpret_cast<decltype(api.GroupStart)>(sym("ncclGroupStart"));
  api.GroupEnd = reinterpret_cast<decltype(api.GroupEnd)>(sym("ncclGroupEnd"));
  api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(sym("ncclGetErrorString"));
  if (!ok) {
    dlclose(h);
    return nullptr;
  }
  api.CommGetAsyncError = reinterpret_cast<decltype(api.CommGetAsyncError)>(dlsym(h, "ncclCommGetAsyncError"));
  api.CommAbort = reinterpret_cast<decltype(api.CommAbort)>(dlsym(h, "ncclCommAbort"));
  api.handle = h;
  return &api;
}

struct Comm {
  int rank = 0, nranks = 1;
  ncclComm_t nccl = nullptr;          // RCCL transport
  std::vector<jxlh_ctx*> peers;       // local transport (peers[rank] == the owning context)
  Event k1_ev;                        // local: this rank's transforms are done (the neighbours copy its edge rows)
  Event done_ev;                      // local: this rank's band is finished (the peers copy it in the gather)
  Event pulled_ev;                    // local: this rank has copied its neighbours' edge rows (they may overwrite them)
  Fence gathered_ev;                  // local: this rank has copied the other bands (their owners may start the next frame)
  // what was enqueued last on the stream through this communicator: named when a wait times out (comm_wait_stream)
  std::string last_op;
  double timeout_s = 120.0;           // JXLH_COMM_TIMEOUT_S; <= 0 waits forever
  // a wait on this communicator's stream expired or RCCL reported an asynchronous error: the stream still holds the
  // stuck collective, so the communicator is ABORTED on release (ncclCommDestroy would wait for it) and every later
  // wait fails at once instead of sitting out another deadline
  bool failed = false;
};

static jxlh_status nccl_fail(jxlh_ctx* ctx, const RcclApi* api, ncclResult_t r, const char* what) {
  ctx->last_error = std::string(what) + ": " + (api && api->GetErrorString ? api->GetErrorString(r) : "rccl error");
  return JXLH_ERR_DEVICE;
}
#define NCCLCHK(ctx, api, expr)                                     \
  do {                                                              \
    ncclResult_t r_ = (expr);                                       \
    if (r_ != ncclSuccess) return nccl_fail(ctx, api, r_, #expr);   \
  } while (0)

// inside ncclGroupStart ... ncclGroupEnd: an error must not leave the group open (every later RCCL call of the thread
// would be queued into it)
#define NCCLCHK_IN_GROUP(ctx, api, expr)                            \
  do {                                                              \
    ncclResult_t r_ = (expr);                                       \
    if (r_ != ncclSuccess) {                                        \
      (void)(api)->GroupEnd();                                      \
      return nccl_fail(ctx, api, r_, #expr);                        \
    }                                                               \
  } while (0)

void comm_release(jxlh_ctx* ctx) {
  Comm* c = ctx->comm;
  if (!c) return;
  (void)hipSetDevice(ctx->device);
  if (c->nccl) {
    if (RcclApi* api = rccl_api(nullptr)) {
      // a communicator with a collective that will never complete is torn down without waiting for it
      if (c->failed && api->CommAbort) (void)api->CommAbort(c->nccl);
      else (void)api->CommDestroy(c->nccl);
    }
  }
  delete c;
  ctx->comm = nullptr;
}

// Waits for the context's stream like hipStreamSynchronize, but with a deadline when the stream may hold collectives
// of an RCCL communicator with other ranks: a peer that never arrives (crashed rank, mismatched call order, a link
// that went away) would otherwise park this process in the driver for ever.  On expiry -- or when RCCL reports an
// asynchronous error -- the call returns JXLH_ERR_DEVICE and jxlh_last_error names rank, world size and the last
// collective that was enqueued; the stream is left as it is (the caller tears the job down).
jxlh_status comm_wait_stream(jxlh_ctx* ctx) {
  Comm* c = ctx->comm;
  if (!c || !c->nccl || c->nranks <= 1 || c->timeout_s <= 0.0) {
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return JXLH_OK;
  }
  if (c->failed) {
    ctx->last_error = "rank " + std::to_string(c->rank) + " of " + std::to_string(c->nranks) +
                      ": the communicator failed earlier (" + c->last_op + "); destroy it (jxlh_comm_destroy / jxlh_ctx_destroy)";
    return JXLH_ERR_DEVICE;
  }
  RcclApi* api = rccl_api(nullptr);
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spins = 0;; spins++) {
    const hipError_t q = hipStreamQuery(ctx->stream);
    if (q == hipSuccess) return JXLH_OK;
    if (q != hipErrorNotReady) return fail(ctx, q, "hipStreamQuery");
    (void)hipGetLastError();
    if (api && api->CommGetAsyncError) {
      ncclResult_t ar = ncclSuccess;
      if (api->CommGetAsyncError(c->nccl, &ar) == ncclSuccess && ar != ncclSuccess && ar != ncclInProgress) {
        ctx->last_error = "rank " + std::to_string(c->rank) + " of " + std::to_string(c->nranks) + ": RCCL asynchronous error (" +
                          (api->GetErrorString ? api->GetErrorString(ar) : "?") + ") after: " + c->last_op;
        c->failed = true;
        return JXLH_ERR_DEVICE;
      }
    }
    const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (el > c->timeout_s) {
      ctx->last_error = "rank " + std::to_string(c->rank) + " of " + std::to_string(c->nranks) + ": the stream did not finish within " +
                        std::to_string((int)c->timeout_s) + " s (JXLH_COMM_TIMEOUT_S); last collective enqueued: " +
                        (c->last_op.empty() ? std::string("none") : c->last_op);
      c->failed = true;
      return JXLH_ERR_DEVICE;
    }
    if (spins > 2000) std::this_thread::sleep_for(std::chrono::microseconds(spins > 20000 ? 1000 : 50));
  }
}

int comm_nranks(const jxlh_ctx* ctx) { return ctx->comm ? ctx->comm->nranks : 1; }

// This rank's share of the protocol (shard_plan.h): the band, the edges to trade when the run exchanges them, and both
// forms of the gather.  A gather passes exchange = false: the edges belong to the run.
static ShardPlan shard_plan(const jxlh_ctx* ctx, bool exchange, size_t bytes_per_row = 0) {
  const FrameDev& f = ctx->fd;
  ShardIn in;
  in.ygroups = f.ygroups, in.ysize = f.ysize, in.nranks = comm_nranks(ctx);
  in.tiled = f.tiled != 0, in.xblocks = f.xblocks, in.plane_stride = f.plane_stride;
  in.exchange = exchange;
  in.result_in_tmp = stage_list(ctx).result_in_tmp();
  in.bytes_per_row = bytes_per_row;
  return plan_shard_rank(in, ctx->comm ? ctx->comm->rank : 0);
}

// transforms of the own band (plus recomputed halo group rows when the exchange does not apply: plan_shard)
static jxlh_status shard_k1(jxlh_ctx* ctx, RunPlan* plan, ShardPlan* sp) {
  if (!ctx->in_frame || ctx->modular || !ctx->tables_set) return JXLH_ERR_BAD_STATE;
  if (ctx->params.upsampling > 1) return JXLH_ERR_UNSUPPORTED;  // the 5x5 upsampling window crosses bands: run whole
  const Comm* c = ctx->comm;
  // patches on a sharded frame: a patch crosses band edges and its reference slot is per context (not supported)
  // (splines likewise: a segment crosses band edges)
  if (draws_in_place(ctx) && c->nranks > 1) return JXLH_ERR_UNSUPPORTED;
  if (jxlh_status st = patches_check_run(ctx)) return st;
  const ShardBand band = shard_band(ctx->fd.ygroups, ctx->fd.ysize, c->nranks, c->rank);
  *plan = plan_shard(run_inputs(ctx), band.r0, band.r1);
  bool sparse_k1 = false;
  if (jxlh_status st = run_prologue(ctx, false, plan->tiled, &sparse_k1)) return st;
  *plan = resolve_strip(*plan, sparse_k1);
  *sp = shard_plan(ctx, plan->exchange);  // (behind the prologue: it sets the layout the transforms write)
  if (band.empty()) return JXLH_OK;
  return run_k1(ctx, *plan);
}

// the peers of an in-process call are the communicator's contexts in rank order: every loop below takes peers[i] for
// rank i (a permuted list would gather other ranks' bands)
static jxlh_status check_local_peers(jxlh_ctx* const peers[], int n, bool need_frame) {
  for (int i = 0; i < n; i++) {
    const jxlh_ctx* p = peers[i];
    if (!p || !p->comm || p->comm->nccl || p->comm->nranks != n || p->comm->rank != i || (need_frame && !p->in_frame))
      return JXLH_ERR_BAD_STATE;
  }
  return JXLH_OK;
}

}  // namespace jxlh_host

extern "C" {

jxlh_status jxlh_comm_unique_id(uint8_t id[JXLH_COMM_ID_BYTES]) {
  if (!id) return JXLH_ERR_INVALID_ARGUMENT;
  static_assert(JXLH_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "id size");
  RcclApi* api = rccl_api(nullptr);
  if (!api) return JXLH_ERR_DEVICE;
  ncclUniqueId u;
  if (api->GetUniqueId(&u) != ncclSuccess) return JXLH_ERR_DEVICE;
  std::memcpy(id, u.internal, JXLH_COMM_ID_BYTES);
  return JXLH_OK;
}

jxlh_status jxlh_comm_init(jxlh_ctx* ctx, const uint8_t id[JXLH_COMM_ID_BYTES], int32_t rank, int32_t nranks) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !id || nranks < 1 || rank < 0 || rank >= nranks) return JXLH_ERR_INVALID_ARGUMENT;
  if (ctx->comm || ctx->in_frame) return JXLH_ERR_BAD_STATE;  // before the first jxlh_frame_begin: it sizes the planes
  std::string err;
  RcclApi* api = rccl_api(&err);
  if (!api) {
    ctx->last_error = err;
    return JXLH_ERR_DEVICE;
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Comm* c = new (std::nothrow) Comm();
  if (!c) return JXLH_ERR_OUT_OF_MEMORY;
  c->rank = rank;
  c->nranks = nranks;
  if (const char* e = getenv("JXLH_COMM_TIMEOUT_S")) c->timeout_s = atof(e);
  ncclUniqueId u;
  std::memcpy(u.internal, id, JXLH_COMM_ID_BYTES);
  const ncclResult_t r = api->CommInitRank(&c->nccl, nranks, u, rank);
  if (r != ncclSuccess) {
    delete c;
    return nccl_fail(ctx, api, r, "ncclCommInitRank");
  }
  ctx->comm = c;
  return JXLH_OK;
}

jxlh_status jxlh_comm_init_local(jxlh_ctx* const peers[], int32_t nranks) {
  if (!peers || nranks < 1) return JXLH_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < nranks; i++) {
    if (!peers[i]) return JXLH_ERR_INVALID_ARGUMENT;
    if (peers[i]->comm || peers[i]->in_frame) return JXLH_ERR_BAD_STATE;
    for (int k = 0; k < i; k++)
      if (peers[k] == peers[i]) return JXLH_ERR_INVALID_ARGUMENT;
  }
  for (int i = 0; i < nranks; i++) {
    jxlh_ctx* ctx = peers[i];
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Comm* c = new (std::nothrow) Comm();
    if (!c) return JXLH_ERR_OUT_OF_MEMORY;
    c->rank = i;
    c->nranks = nranks;
    c->peers.assign(peers, peers + nranks);
    if (c->k1_ev.create() != hipSuccess || c->done_ev.create() != hipSuccess || c->pulled_ev.create() != hipSuccess ||
        c->gathered_ev.ev.create() != hipSuccess) {
      delete c;
      return JXLH_ERR_DEVICE;
    }
    // peers on other GPUs: direct access for the copies (already-enabled is fine)
    for (int k = 0; k < nranks; k++) {
      if (peers[k]->device != ctx->device) {
        (void)hipDeviceEnablePeerAccess(peers[k]->device, 0);
        (void)hipGetLastError();
      }
    }
    ctx->comm = c;
  }
  return JXLH_OK;
}

jxlh_status jxlh_comm_destroy(jxlh_ctx* ctx) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx) return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->comm) return JXLH_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  comm_release(ctx);
  return JXLH_OK;
}

jxlh_status jxlh_comm_band(jxlh_ctx* ctx, int32_t* rank, int32_t* nranks, uint32_t* group_row0, uint32_t* group_row1) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx) return JXLH_ERR_INVALID_ARGUMENT;
  const int n = ctx->comm ? ctx->comm->nranks : 1, r = ctx->comm ? ctx->comm->rank : 0;
  if (rank) *rank = r;
  if (nranks) *nranks = n;
  if (group_row0 || group_row1) {
    if (!ctx->in_frame) return JXLH_ERR_BAD_STATE;
    const ShardBand band = shard_band(ctx->fd.ygroups, ctx->fd.ysize, n, r);
    if (group_row0) *group_row0 = (uint32_t)band.r0;
    if (group_row1) *group_row1 = (uint32_t)band.r1;
  }
  return JXLH_OK;
}

// ---- RCCL transport ------------------------------------------------------------------------------------------
jxlh_status jxlh_frame_run_sharded(jxlh_ctx* ctx) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx) return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->comm || !ctx->comm->nccl) return JXLH_ERR_BAD_STATE;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Comm* c = ctx->comm;
  RcclApi* api = rccl_api(nullptr);
  RunPlan plan;
  ShardPlan sp;
  if (jxlh_status st = shard_k1(ctx, &plan, &sp)) return st;
  const FrameDev& f = ctx->fd;
  if (sp.n_edges > 0) {
    c->last_op = "halo exchange of the band edges (ncclSend/ncclRecv with rank";
    for (int e = 0; e < sp.n_edges; e++) c->last_op += " " + std::to_string(sp.edge[e].peer);
    c->last_op += ", group rows " + std::to_string(sp.band.r0) + ".." + std::to_string(sp.band.r1) + ")";
    NCCLCHK(ctx, api, api->GroupStart());
    for (int ch = 0; ch < 3; ch++) {
      for (int e = 0; e < sp.n_edges; e++) {  // my edge block row goes to the neighbour, the block row beyond the edge comes back
        const ShardEdge& g = sp.edge[e];
        NCCLCHK_IN_GROUP(ctx, api, api->Send(f.planes[ch] + g.send.off, g.send.n, ncclFloat32, g.peer, c->nccl, ctx->stream));
        NCCLCHK_IN_GROUP(ctx, api, api->Recv(f.planes[ch] + g.recv.off, g.recv.n, ncclFloat32, g.peer, c->nccl, ctx->stream));
      }
    }
    NCCLCHK(ctx, api, api->GroupEnd());
  }
  if (sp.band.empty()) return JXLH_OK;
  return run_stages_rows(ctx, plan.stages, plan.y_lo, plan.y_hi, plan.whole);
}

// where a band run left the finished planes (a rank whose band is empty ran no stage: the plan says where the result
// lives) + the geometry the read-out stages use
static void set_band_result(jxlh_ctx* ctx, const ShardPlan& sp) {
  const FrameDev& f = ctx->fd;
  for (int ch = 0; ch < 3; ch++) ctx->frame.result[ch] = sp.result_in_tmp ? f.tmp[ch] : f.planes[ch];
  ctx->res_w = f.xsize;
  ctx->res_h = f.ysize;
  ctx->res_stride = f.plane_stride;
}

jxlh_status jxlh_frame_allgather(jxlh_ctx* ctx) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx) return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->comm || !ctx->comm->nccl || !ctx->in_frame) return JXLH_ERR_BAD_STATE;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Comm* c = ctx->comm;
  RcclApi* api = rccl_api(nullptr);
  const ShardPlan sp = shard_plan(ctx, false);
  set_band_result(ctx, sp);
  const ShardSpan slot = sp.slot_planes;
  c->last_op = "ncclAllGather of the finished planes (" + std::to_string(slot.n * 4) + " bytes per rank and plane)";
  NCCLCHK(ctx, api, api->GroupStart());
  for (int ch = 0; ch < 3; ch++)
    NCCLCHK_IN_GROUP(ctx, api, api->AllGather(ctx->frame.result[ch] + slot.off, ctx->frame.result[ch], slot.n, ncclFloat32, c->nccl, ctx->stream));
  NCCLCHK(ctx, api, api->GroupEnd());
  return JXLH_OK;
}

jxlh_status jxlh_frame_allgather_output(jxlh_ctx* ctx, const jxlh_output_desc* d, void* out, size_t bytes_per_row) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !d || !out) return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->comm || !ctx->comm->nccl || !ctx->in_frame) return JXLH_ERR_BAD_STATE;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Comm* c = ctx->comm;
  RcclApi* api = rccl_api(nullptr);
  const FrameDev& f = ctx->fd;
  if (bytes_per_row < (size_t)f.xsize * d->channels * (d->bits / 8)) return JXLH_ERR_INVALID_ARGUMENT;
  const ShardPlan sp = shard_plan(ctx, false, bytes_per_row);
  set_band_result(ctx, sp);
  if (jxlh_status st = convert_band_to_output(ctx, d, (uint32_t)sp.band.y0, (uint32_t)sp.band.y1, out, bytes_per_row)) return st;
  const ShardSpan slot = sp.slot_image;
  c->last_op = "ncclAllGather of the converted image (" + std::to_string(slot.n) + " bytes per rank)";
  NCCLCHK(ctx, api, api->AllGather(static_cast<char*>(out) + slot.off, out, slot.n, ncclUint8, c->nccl, ctx->stream));
  return JXLH_OK;
}

jxlh_status jxlh_frames_allgather_output_local(jxlh_ctx* const peers[], int32_t n, const jxlh_output_desc* d,
                                               void* const outs[], size_t bytes_per_row) {
  if (!peers || !outs || !d || n < 1) return JXLH_ERR_INVALID_ARGUMENT;
  if (jxlh_status st = check_local_peers(peers, n, true)) return st;
  for (int i = 0; i < n; i++)
    if (!outs[i]) return JXLH_ERR_BAD_STATE;
  // every rank converts its band into its own image buffer ...
  std::vector<ShardPlan> sp(n);
  for (int i = 0; i < n; i++) {
    jxlh_ctx* c = peers[i];
    HIPCHK(c, hipSetDevice(c->device));
    if (bytes_per_row < (size_t)c->fd.xsize * d->channels * (d->bits / 8)) return JXLH_ERR_INVALID_ARGUMENT;
    sp[i] = shard_plan(c, false, bytes_per_row);
    set_band_result(c, sp[i]);
    if (jxlh_status st = convert_band_to_output(c, d, (uint32_t)sp[i].band.y0, (uint32_t)sp[i].band.y1, outs[i], bytes_per_row))
      return st;
    HIPCHK(c, hipEventRecord(c->comm->done_ev, c->stream));
  }
  // ... and pulls the other ranks' bands
  for (int i = 0; i < n; i++) {
    jxlh_ctx* dst = peers[i];
    HIPCHK(dst, hipSetDevice(dst->device));
    for (const ShardPull& pull : sp[i].pulls) {
      HIPCHK(dst, hipStreamWaitEvent(dst->stream, peers[pull.peer]->comm->done_ev, 0));
      HIPCHK(dst, hipMemcpyAsync(static_cast<char*>(outs[i]) + pull.image.off,
                                 static_cast<const char*>(outs[pull.peer]) + pull.image.off, pull.image.n,
                                 hipMemcpyDefault, dst->stream));
    }
  }
  return JXLH_OK;
}

jxlh_status jxlh_comm_allgather(jxlh_ctx* ctx, void* buf, size_t bytes_per_rank) {
  JXLH_ON_DEVICE(ctx);
  if (!ctx || !buf) return JXLH_ERR_INVALID_ARGUMENT;
  if (!ctx->comm || !ctx->comm->nccl) return JXLH_ERR_BAD_STATE;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Comm* c = ctx->comm;
  RcclApi* api = rccl_api(nullptr);
  c->last_op = "jxlh_comm_allgather (" + std::to_string(bytes_per_rank) + " bytes per rank)";
  NCCLCHK(ctx, api, api->AllGather(static_cast<char*>(buf) + (size_t)c->rank * bytes_per_rank, buf, bytes_per_rank,
                                   ncclUint8, c->nccl, ctx->stream));
  return JXLH_OK;
}

jxlh_status jxlh_comm_allgather_local(jxlh_ctx* const peers[], int32_t n, void* const bufs[], size_t bytes_per_rank) {
  if (!peers || !bufs || n < 1) return JXLH_ERR_INVALID_ARGUMENT;
  if (jxlh_status st = check_local_peers(peers, n, false)) return st;
  for (int i = 0; i < n; i++)
    if (!bufs[i]) return JXLH_ERR_BAD_STATE;
  // every rank's part is final once its stream reaches this point ...
  for (int i = 0; i < n; i++) {
    HIPCHK(peers[i], hipSetDevice(peers[i]->device));
    HIPCHK(peers[i], hipEventRecord(peers[i]->comm->done_ev, peers[i]->stream));
  }
  // ... and every rank pulls the other ranks' parts
  for (int i = 0; i < n; i++) {
    jxlh_ctx* dst = peers[i];
    HIPCHK(dst, hipSetDevice(dst->device));
    for (int k = 0; k < n; k++) {
      if (k == i) continue;
      HIPCHK(dst, hipStreamWaitEvent(dst->stream, peers[k]->comm->done_ev, 0));
      HIPCHK(dst, hipMemcpyAsync(static_cast<char*>(bufs[i]) + (size_t)k * bytes_per_rank,
                                 static_cast<const char*>(bufs[k]) + (size_t)k * bytes_per_rank, bytes_per_rank,
                                 hipMemcpyDefault, dst->stream));
    }
  }
  return JXLH_OK;
}

// ---- local transport -----------------------------------------------------------------------------------------
jxlh_status jxlh_frames_run_sharded_local(jxlh_ctx* const peers[], int32_t n) {
  if (!peers || n < 1) return JXLH_ERR_INVALID_ARGUMENT;
  if (jxlh_status st = check_local_peers(peers, n, false)) return st;
  std::vector<RunPlan> plan(n);
  std::vector<ShardPlan> sp(n);
  // phase 1: every rank's transforms
  for (int i = 0; i < n; i++) {
    jxlh_ctx* ctx = peers[i];
    HIPCHK(ctx, hipSetDevice(ctx->device));
    for (int k = 0; k < n; k++)  // the previous frame's gather may still be reading this rank's band
      if (k != i) HIPCHK(ctx, peers[k]->comm->gathered_ev.wait(ctx->stream));
    if (jxlh_status st = shard_k1(ctx, &plan[i], &sp[i])) return st;
    HIPCHK(ctx, hipEventRecord(ctx->comm->k1_ev, ctx->stream));
  }
  for (int i = 0; i < n; i++)
    for (int e = 0; e < sp[i].n_edges; e++)
      if (!same_layout(sp[i], sp[sp[i].edge[e].peer])) return JXLH_ERR_BAD_STATE;  // the peers decode the same frame
  // phase 2: every rank pulls the edge block rows it reads across its band edges from the neighbours ...
  for (int i = 0; i < n; i++) {
    jxlh_ctx* ctx = peers[i];
    HIPCHK(ctx, hipSetDevice(ctx->device));
    for (int e = 0; e < sp[i].n_edges; e++) {
      const ShardEdge& g = sp[i].edge[e];
      jxlh_ctx* src = peers[g.peer];
      HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, src->comm->k1_ev, 0));
      for (int ch = 0; ch < 3; ch++)
        HIPCHK(ctx, hipMemcpyAsync(ctx->fd.planes[ch] + g.recv.off, src->fd.planes[ch] + g.recv.off, g.recv.n * sizeof(float),
                                   hipMemcpyDefault, ctx->stream));
    }
    HIPCHK(ctx, hipEventRecord(ctx->comm->pulled_ev, ctx->stream));
  }
  // ... phase 3: and filters its band once the neighbours have taken their copies (a stage list that ends in
  // `planes` overwrites the rows they read)
  for (int i = 0; i < n; i++) {
    jxlh_ctx* ctx = peers[i];
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (sp[i].band.empty()) continue;
    if (i > 0) HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, peers[i - 1]->comm->pulled_ev, 0));
    if (i + 1 < n) HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, peers[i + 1]->comm->pulled_ev, 0));
    if (jxlh_status st = run_stages_rows(ctx, plan[i].stages, plan[i].y_lo, plan[i].y_hi, plan[i].whole)) return st;
  }
  for (int i = 0; i < n; i++) {
    jxlh_ctx* ctx = peers[i];
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipEventRecord(ctx->comm->done_ev, ctx->stream));
  }
  return JXLH_OK;
}

jxlh_status jxlh_frames_allgather_local(jxlh_ctx* const peers[], int32_t n) {
  if (!peers || n < 1) return JXLH_ERR_INVALID_ARGUMENT;
  if (jxlh_status st = check_local_peers(peers, n, true)) return st;
  for (int i = 0; i < n; i++) {
    jxlh_ctx* dst = peers[i];
    HIPCHK(dst, hipSetDevice(dst->device));
    const ShardPlan sp = shard_plan(dst, false);
    set_band_result(dst, sp);
    for (const ShardPull& pull : sp.pulls) {
      jxlh_ctx* src = peers[pull.peer];
      HIPCHK(dst, hipStreamWaitEvent(dst->stream, src->comm->done_ev, 0));
      for (int c = 0; c < 3; c++) {  // (the plane set is a property of the stage list, identical on every peer)
        const float* s = (sp.result_in_tmp ? src->fd.tmp[c] : src->fd.planes[c]) + pull.planes.off;
        HIPCHK(dst, hipMemcpyAsync(dst->frame.result[c] + pull.planes.off, s, pull.planes.n * sizeof(float), hipMemcpyDefault,
                                   dst->stream));
      }
    }
    HIPCHK(dst, dst->comm->gathered_ev.record(dst->stream));
  }
  return JXLH_OK;
}

}  // extern "C"
