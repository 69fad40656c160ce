// The shard plan (jxl_rs_amd/csrc/shard_plan.h) on its own: plain C++, no device, no library -- also the program a
// sanitizer build runs (tests/test_shard_plan_cpu.py).  Every rank of every world is planned: ygroups 1..9, 1..8 ranks,
// a frame that ends in the middle of its last group row and one that fills it, both plane layouts, the exchange on and
// off, both result plane sets.  Checked per world:
//   same as before   the index arithmetic comm.hip carried inline (band_of, the has_up / has_dn selection, the `side` loop,
//                    block_row_span, the four gathers), transcribed below with its own constants: every field of every
//                    plan equals it
//   pairing          the ranks' sends and receives, in the order comm.hip issues them, matched per ordered pair of ranks
//                    the way NCCL matches them: equal numbers, equal counts, nothing left over
//   data movement    model planes tagged (rank, channel, row): after the exchange every band holds its neighbours' edge
//                    block rows; after either form of the gather every rank holds every row with its owner's tag -- the
//                    f32 planes in floats, the converted image in bytes
//   bounds           everything the plan names lies inside what plan_frame (the real frame_plan.h) sized
//   shard_plan dump  prints `band YGROUPS NRANKS YSIZE RANK R0 R1 Y0 Y1 PER` for the test to hold jxl_rs_amd/shard.py to
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../jxl_rs_amd/csrc/frame_plan.h"
#include "../../jxl_rs_amd/csrc/shard_plan.h"

using namespace jxlh;

namespace {

int g_fail = 0;
long g_plans = 0;
#define CHECK(c, ...)                          \
  do {                                         \
    if (!(c)) {                                \
      if (g_fail++ < 20) {                     \
        std::printf("FAIL line %d %s: ", __LINE__, #c); \
        std::printf(__VA_ARGS__);              \
        std::printf("\n");                     \
      }                                        \
    }                                          \
  } while (0)

// ---- the code the plan replaced, as it stood in comm.hip
namespace old {
constexpr int kGroupDim = 256, kGroupBlocks = 32;
struct FrameDev {
  int ygroups, ysize, tiled, xblocks;
  size_t plane_stride;
};
int rows_per_rank(int ygroups, int nranks) { return (ygroups + nranks - 1) / nranks; }
void band_of(int ygroups, int nranks, int rank, int* r0, int* r1) {
  const int per = rows_per_rank(ygroups, nranks);
  *r0 = std::min(rank * per, ygroups);
  *r1 = std::min((rank + 1) * per, ygroups);
}
void block_row_span(const FrameDev& f, int by, size_t* off, size_t* count) {
  if (f.tiled) {
    *off = (size_t)by * f.xblocks * 64;
    *count = (size_t)f.xblocks * 64;
  } else {
    *off = (size_t)by * 8 * f.plane_stride;
    *count = 8 * f.plane_stride;
  }
}
struct Op {  // one ncclSend / ncclRecv, or one copy of the in-process transport (send = false: into the own planes)
  bool send;
  int ch, peer;
  size_t off, cnt;
};
// jxlh_frame_run_sharded: what it passed to ncclSend / ncclRecv, in order
std::vector<Op> run_sharded(const FrameDev& f, int nranks, int rank, bool exchange) {
  std::vector<Op> ops;
  int r0, r1;
  band_of(f.ygroups, nranks, rank, &r0, &r1);
  if (exchange && nranks > 1) {
    int up0, up1, dn0, dn1;
    const bool mine = r0 < r1;
    bool has_up = false, has_dn = false;
    if (mine && rank > 0) {
      band_of(f.ygroups, nranks, rank - 1, &up0, &up1);
      has_up = up0 < up1;
    }
    if (mine && rank + 1 < nranks) {
      band_of(f.ygroups, nranks, rank + 1, &dn0, &dn1);
      has_dn = dn0 < dn1;
    }
    if (has_up || has_dn) {
      for (int ch = 0; ch < 3; ch++) {
        size_t off, cnt;
        if (has_up) {
          block_row_span(f, r0 * kGroupBlocks, &off, &cnt);
          ops.push_back({true, ch, rank - 1, off, cnt});
          block_row_span(f, r0 * kGroupBlocks - 1, &off, &cnt);
          ops.push_back({false, ch, rank - 1, off, cnt});
        }
        if (has_dn) {
          block_row_span(f, r1 * kGroupBlocks - 1, &off, &cnt);
          ops.push_back({true, ch, rank + 1, off, cnt});
          block_row_span(f, r1 * kGroupBlocks, &off, &cnt);
          ops.push_back({false, ch, rank + 1, off, cnt});
        }
      }
    }
  }
  return ops;
}
// jxlh_frames_run_sharded_local, phase 2 of rank i: the copies from peers[nb], same offset on both sides
std::vector<Op> run_sharded_local(const FrameDev& f, int n, int i, bool exchange) {
  std::vector<Op> ops;
  int r0, r1;
  band_of(f.ygroups, n, i, &r0, &r1);  // plan[i].group_row0, group_row1
  if (r0 < r1 && exchange) {
    for (int side = 0; side < 2; side++) {
      const int nb = side == 0 ? i - 1 : i + 1;
      int n0 = 0, n1 = 0;
      if (nb >= 0 && nb < n) band_of(f.ygroups, n, nb, &n0, &n1);
      if (nb < 0 || nb >= n || n0 >= n1) continue;
      const int by = side == 0 ? r0 * kGroupBlocks - 1 : r1 * kGroupBlocks;
      size_t off, cnt;
      block_row_span(f, by, &off, &cnt);
      for (int ch = 0; ch < 3; ch++) ops.push_back({false, ch, nb, off, cnt});
    }
  }
  return ops;
}
struct Span {
  int peer;
  size_t off, n;
};
// jxlh_frame_allgather: the send offset and the count of ncclAllGather
Span allgather(const FrameDev& f, int nranks, int rank) {
  const size_t count = (size_t)rows_per_rank(f.ygroups, nranks) * kGroupDim * f.plane_stride;
  return {rank, (size_t)rank * count, count};
}
// jxlh_frame_allgather_output: the rows converted, then the same in bytes
Span allgather_output(const FrameDev& f, int nranks, int rank, size_t bytes_per_row, uint32_t* y0, uint32_t* y1) {
  int r0, r1;
  band_of(f.ygroups, nranks, rank, &r0, &r1);
  *y0 = (uint32_t)std::min(r0 * kGroupDim, f.ysize);
  *y1 = (uint32_t)std::min(r1 * kGroupDim, f.ysize);
  const size_t count = (size_t)rows_per_rank(f.ygroups, nranks) * kGroupDim * bytes_per_row;
  return {rank, (size_t)rank * count, count};
}
// jxlh_frames_allgather_output_local: the copies of rank i
std::vector<Span> allgather_output_local(const FrameDev& f, int n, int i, size_t bytes_per_row) {
  std::vector<Span> v;
  for (int k = 0; k < n; k++) {
    if (k == i) continue;
    int r0, r1;
    band_of(f.ygroups, n, k, &r0, &r1);
    const size_t y0 = (size_t)std::min(r0 * kGroupDim, f.ysize), y1 = (size_t)std::min(r1 * kGroupDim, f.ysize);
    if (y0 >= y1) continue;
    v.push_back({k, y0 * bytes_per_row, (y1 - y0) * bytes_per_row});
  }
  return v;
}
// jxlh_frames_allgather_local: the copies of rank i, per channel
std::vector<Span> allgather_local(const FrameDev& f, int n, int i) {
  std::vector<Span> v;
  for (int k = 0; k < n; k++) {
    if (k == i) continue;
    int r0, r1;
    band_of(f.ygroups, n, k, &r0, &r1);
    if (r0 >= r1) continue;
    const size_t off = (size_t)r0 * kGroupDim * f.plane_stride;
    const size_t rows = (size_t)std::min(r1 * kGroupDim, f.ysize) - (size_t)r0 * kGroupDim;
    v.push_back({k, off, rows * f.plane_stride});
  }
  return v;
}
}  // namespace old

struct Case {
  int ygroups, nranks, ysize;
  bool tiled, exchange;
  int result_in_tmp;
  FramePlan fp;          // what jxlh_frame_begin sizes for this frame and world
  size_t bytes_per_row;  // of the converted image: RGB8 rows, not a multiple of anything
};

constexpr uint32_t kXsize = 8;

jxlh_frame_params frame_params(uint32_t ysize) {
  jxlh_frame_params p;
  std::memset(&p, 0, sizeof p);
  p.abi_version = JXLH_ABI_VERSION;
  p.xsize = kXsize, p.ysize = ysize;
  p.global_scale = 21845, p.quant_lf = 16, p.color_factor = 84;
  p.quant_biases[0] = p.quant_biases[1] = p.quant_biases[2] = 0.9f;
  return p;
}

ShardIn shard_in(const Case& c) {
  ShardIn in;
  in.ygroups = c.ygroups, in.ysize = c.ysize, in.nranks = c.nranks;
  in.tiled = c.tiled, in.xblocks = c.fp.xblocks, in.plane_stride = c.fp.plane_stride;
  in.exchange = c.exchange, in.result_in_tmp = c.result_in_tmp, in.bytes_per_row = c.bytes_per_row;
  return in;
}

// the sends and receives of one rank in the order jxlh_frame_run_sharded issues them: per channel, per edge, send, recv
std::vector<old::Op> issue_order(const ShardPlan& p) {
  std::vector<old::Op> ops;
  for (int ch = 0; ch < 3; ch++)
    for (int e = 0; e < p.n_edges; e++) {
      ops.push_back({true, ch, p.edge[e].peer, p.edge[e].send.off, p.edge[e].send.n});
      ops.push_back({false, ch, p.edge[e].peer, p.edge[e].recv.off, p.edge[e].recv.n});
    }
  return ops;
}
bool same(const old::Op& a, const old::Op& b) {
  return a.send == b.send && a.ch == b.ch && a.peer == b.peer && a.off == b.off && a.cnt == b.cnt;
}

#define WHERE_FMT "ygroups %d ranks %d ysize %d tiled %d exchange %d tmp %d rank %d"
#define WHERE_ARGS c.ygroups, c.nranks, c.ysize, (int)c.tiled, (int)c.exchange, c.result_in_tmp, r
#define WHERE WHERE_FMT, WHERE_ARGS

void check_same_as_before(const Case& c, const std::vector<ShardPlan>& plans) {
  const old::FrameDev f{c.ygroups, c.ysize, c.tiled ? 1 : 0, c.fp.xblocks, c.fp.plane_stride};
  for (int r = 0; r < c.nranks; r++) {
    const ShardPlan& p = plans[r];
    int r0, r1;
    old::band_of(c.ygroups, c.nranks, r, &r0, &r1);
    CHECK(p.rank == r && p.nranks == c.nranks && p.band.r0 == r0 && p.band.r1 == r1, WHERE);
    CHECK(p.rows_per_rank == old::rows_per_rank(c.ygroups, c.nranks) && p.rows_per_rank == c.fp.rows_per_rank, WHERE);
    CHECK(p.result_in_tmp == c.result_in_tmp, WHERE);
    // RCCL run: the same calls in the same order
    const std::vector<old::Op> was = old::run_sharded(f, c.nranks, r, c.exchange), now = issue_order(p);
    CHECK(was.size() == now.size(), WHERE);
    for (size_t i = 0; i < was.size() && i < now.size(); i++) CHECK(same(was[i], now[i]), WHERE);
    // local run: per edge, three copies of the received block row from the edge's peer
    const std::vector<old::Op> lwas = old::run_sharded_local(f, c.nranks, r, c.exchange);
    CHECK(lwas.size() == (size_t)3 * p.n_edges, WHERE);
    for (size_t i = 0; i < lwas.size() && i < (size_t)3 * p.n_edges; i++) {
      const ShardEdge& e = p.edge[i / 3];
      CHECK(same(lwas[i], old::Op{false, (int)(i % 3), e.peer, e.recv.off, e.recv.n}), WHERE);
    }
    // the four gathers
    const old::Span a = old::allgather(f, c.nranks, r);
    CHECK(p.slot_planes.off == a.off && p.slot_planes.n == a.n, WHERE);
    uint32_t y0, y1;
    const old::Span ao = old::allgather_output(f, c.nranks, r, c.bytes_per_row, &y0, &y1);
    CHECK(p.slot_image.off == ao.off && p.slot_image.n == ao.n && (uint32_t)p.band.y0 == y0 && (uint32_t)p.band.y1 == y1, WHERE);
    const std::vector<old::Span> lo = old::allgather_output_local(f, c.nranks, r, c.bytes_per_row), lp = old::allgather_local(f, c.nranks, r);
    CHECK(lo.size() == p.pulls.size() && lp.size() == p.pulls.size(), WHERE);
    for (size_t i = 0; i < p.pulls.size() && i < lo.size() && i < lp.size(); i++) {
      CHECK(p.pulls[i].peer == lo[i].peer && p.pulls[i].image.off == lo[i].off && p.pulls[i].image.n == lo[i].n, WHERE);
      CHECK(p.pulls[i].peer == lp[i].peer && p.pulls[i].planes.off == lp[i].off && p.pulls[i].planes.n == lp[i].n, WHERE);
    }
  }
}

// NCCL matches the operations between one pair of ranks in the order each side issued them
void check_pairing(const Case& c, const std::vector<ShardPlan>& plans) {
  std::vector<std::vector<old::Op>> ops;
  for (const ShardPlan& p : plans) ops.push_back(issue_order(p));
  for (int r = 0; r < c.nranks; r++) {
    CHECK((plans[r].n_edges == 0) == ops[r].empty(), WHERE);
    if (!c.exchange || plans[r].band.empty()) CHECK(plans[r].n_edges == 0, WHERE);
    for (int e = 0; e < plans[r].n_edges; e++) {
      const int peer = plans[r].edge[e].peer;
      CHECK((peer == r - 1 || peer == r + 1) && peer >= 0 && peer < c.nranks, WHERE);
      if (e > 0) CHECK(peer > plans[r].edge[e - 1].peer, WHERE);  // the upper edge first
    }
    for (int to = 0; to < c.nranks; to++) {  // r's sends to `to` against `to`'s receives from r
      std::vector<old::Op> sends, recvs;
      for (const old::Op& o : ops[r])
        if (o.send && o.peer == to) sends.push_back(o);
      if (to != r)
        for (const old::Op& o : ops[to])
          if (!o.send && o.peer == r) recvs.push_back(o);
      CHECK(sends.size() == recvs.size(), WHERE);
      for (size_t i = 0; i < sends.size() && i < recvs.size(); i++) CHECK(sends[i].cnt == recvs[i].cnt && sends[i].ch == recvs[i].ch, WHERE);
    }
  }
}

// ---- the model frame.  Nothing below uses the header's arithmetic: rows and owners are worked out here.
uint32_t tag(int rank, int ch, int row) { return (uint32_t)(rank + 1) << 24 | (uint32_t)ch << 16 | (uint32_t)row; }
int owner_of_group_row(const Case& c, int gy) { return gy / ((c.ygroups + c.nranks - 1) / c.nranks); }
int last_rank_with_rows(const Case& c) { return owner_of_group_row(c, c.ygroups - 1); }

void check_exchange(const Case& c, const std::vector<ShardPlan>& plans) {
  const size_t row_n = c.tiled ? (size_t)c.fp.xblocks * 64 : 8 * c.fp.plane_stride;  // one block row in K1's layout
  // planes[rank][ch]: what each rank's transforms wrote, block row by block row
  std::vector<std::vector<std::vector<uint32_t>>> planes(c.nranks);
  for (int r = 0; r < c.nranks; r++)
    for (int ch = 0; ch < 3; ch++) {
      planes[r].emplace_back(c.fp.yblocks * row_n, 0u);  // (check_bounds holds every block row named below yblocks)
      for (int by = 0; by < c.fp.yblocks; by++)
        if (owner_of_group_row(c, by / 32) == r) std::fill_n(planes[r][ch].begin() + by * row_n, row_n, tag(r, ch, by));
    }
  auto local = planes;
  const size_t cap = c.fp.yblocks * row_n;
  // RCCL: the k-th send of a to b lands in the k-th receive b posted for a
  for (int a = 0; a < c.nranks; a++)
    for (int b = 0; b < c.nranks; b++) {
      std::vector<old::Op> sends, recvs;
      for (const old::Op& o : issue_order(plans[a]))
        if (o.send && o.peer == b) sends.push_back(o);
      for (const old::Op& o : issue_order(plans[b]))
        if (!o.send && o.peer == a) recvs.push_back(o);
      for (size_t i = 0; i < sends.size() && i < recvs.size(); i++)
        if (sends[i].cnt == recvs[i].cnt && sends[i].off + sends[i].cnt <= cap && recvs[i].off + recvs[i].cnt <= cap)
          std::copy_n(planes[a][sends[i].ch].begin() + sends[i].off, sends[i].cnt, planes[b][recvs[i].ch].begin() + recvs[i].off);
    }
  // local: a rank copies the block row beyond its edge out of the neighbour's planes, same offset
  for (int r = 0; r < c.nranks; r++)
    for (int e = 0; e < plans[r].n_edges; e++) {
      const ShardEdge& g = plans[r].edge[e];
      if (g.recv.off + g.recv.n > cap) continue;  // (reported by check_bounds)
      for (int ch = 0; ch < 3; ch++) std::copy_n(local[g.peer][ch].begin() + g.recv.off, g.recv.n, local[r][ch].begin() + g.recv.off);
    }
  // every band holds its own block rows and, with the exchange, the block row on the far side of each inner edge; nothing else
  for (int r = 0; r < c.nranks; r++)
    for (int ch = 0; ch < 3; ch++)
      for (int by = 0; by < c.fp.yblocks; by++) {
        const int o = owner_of_group_row(c, by / 32);
        const bool mine = o == r;
        const bool halo = c.exchange && r <= last_rank_with_rows(c) &&
                          ((o == r - 1 && (by + 1) % 32 == 0 && owner_of_group_row(c, (by + 1) / 32) == r) ||
                           (o == r + 1 && by % 32 == 0 && owner_of_group_row(c, (by - 1) / 32) == r));
        const uint32_t want = mine || halo ? tag(o, ch, by) : 0u;
        for (const auto* model : {&planes, &local}) {  // the whole block row is `want`: its first entry is, and all are alike
          const uint32_t* row = (*model)[r][ch].data() + by * row_n;
          CHECK(row[0] == want && std::equal(row, row + row_n - 1, row + 1), WHERE);
        }
      }
}

// One buffer per rank of `total` units (floats of a plane, or bytes of the image), rows of `stride` units.  Every rank
// holds its own band; after either form of the gather every rank holds rows [0, ysize) with their owners' tags.
template <class Slot, class Pull>
void check_gather(const Case& c, const std::vector<ShardPlan>& plans, size_t stride, size_t total, Slot slot, Pull pull, const char* what) {
  std::vector<uint32_t> frame((size_t)c.ysize * stride);  // the whole frame: every row with its owner's tag
  for (int y = 0; y < c.ysize; y++) std::fill_n(frame.begin() + y * stride, stride, tag(owner_of_group_row(c, y / 256), 0, y));
  std::vector<std::vector<uint32_t>> own(c.nranks);
  for (int r = 0; r < c.nranks; r++) {
    own[r].assign(total, 0u);
    for (int y = 0; y < c.ysize; y++)
      if (owner_of_group_row(c, y / 256) == r) std::copy_n(frame.begin() + y * stride, stride, own[r].begin() + y * stride);
  }
  auto whole = [&](const std::vector<std::vector<uint32_t>>& buf, const char* form) {
    for (int r = 0; r < c.nranks; r++)
      CHECK(std::equal(frame.begin(), frame.end(), buf[r].begin()), "%s, %s: " WHERE_FMT, what, form, WHERE_ARGS);
  };
  {  // equal slots: an in-place all-gather takes `n` units at the own slot and leaves rank k's at k * n
    auto buf = own;
    const size_t n = slot(plans[0]).n;
    bool ok = (size_t)c.nranks * n <= total;
    for (int r = 0; r < c.nranks; r++) ok = ok && slot(plans[r]).n == n && slot(plans[r]).off == (size_t)r * n;
    int r = -1;
    CHECK(ok, "%s: " WHERE_FMT, what, WHERE_ARGS);
    if (ok) {
      for (int k = 0; k < c.nranks; k++)
        for (int d = 0; d < c.nranks; d++)
          if (d != k) std::copy_n(own[k].begin() + slot(plans[k]).off, n, buf[d].begin() + (size_t)k * n);
      whole(buf, "equal slots");
    }
  }
  {  // existing rows: every rank copies the spans of its plan out of their owners' buffers, same offset
    auto buf = own;
    for (int r = 0; r < c.nranks; r++)
      for (const ShardPull& p : plans[r].pulls)
        if (pull(p).off + pull(p).n <= total) std::copy_n(own[p.peer].begin() + pull(p).off, pull(p).n, buf[r].begin() + pull(p).off);
    whole(buf, "existing rows");
  }
}

void check_bounds(const Case& c, const std::vector<ShardPlan>& plans) {
  const FramePlan& fp = c.fp;
  const size_t row_n = c.tiled ? (size_t)fp.xblocks * 64 : 8 * fp.plane_stride;
  const size_t result_n = c.result_in_tmp ? fp.tmp_n : fp.planes_n;
  const size_t image_n = (size_t)c.nranks * fp.rows_per_rank * 256 * c.bytes_per_row;  // what the caller allocates (jxl_hip.h)
  for (int r = 0; r < c.nranks; r++) {
    const ShardPlan& p = plans[r];
    for (int e = 0; e < p.n_edges; e++) {  // the transforms' planes
      const ShardEdge& g = p.edge[e];
      CHECK(g.send.n == row_n && g.recv.n == row_n && g.send.off % row_n == 0 && g.recv.off % row_n == 0, WHERE);
      CHECK(g.send.off + g.send.n <= fp.planes_n && g.recv.off + g.recv.n <= fp.planes_n, WHERE);
      CHECK(g.send.off / row_n < (size_t)fp.yblocks && g.recv.off / row_n < (size_t)fp.yblocks, WHERE);
    }
    CHECK(p.slot_planes.off + p.slot_planes.n <= fp.gather_elems && fp.gather_elems <= result_n, WHERE);
    CHECK((size_t)c.nranks * p.slot_planes.n <= fp.planes_n && (size_t)c.nranks * p.slot_planes.n <= fp.tmp_n, WHERE);
    CHECK(p.slot_image.off + p.slot_image.n <= image_n, WHERE);
    // the other ranks' spans and the own band: disjoint, ascending, and together exactly the rows that exist
    size_t rows = (size_t)(p.band.y1 - p.band.y0), end = 0, end_image = 0;
    bool own_seen = false;
    for (const ShardPull& q : p.pulls) {
      CHECK(q.peer != r && q.peer >= 0 && q.peer < c.nranks && q.planes.n > 0 && q.image.n > 0, WHERE);
      if (q.peer > r && !own_seen) end += rows * fp.plane_stride, end_image += rows * c.bytes_per_row, own_seen = true;
      CHECK(q.planes.off == end && q.image.off == end_image, WHERE);
      end = q.planes.off + q.planes.n, end_image = q.image.off + q.image.n;
      CHECK(end <= fp.plane_elems && end <= result_n && end_image <= image_n, WHERE);
    }
    if (!own_seen) end += rows * fp.plane_stride, end_image += rows * c.bytes_per_row;
    CHECK(end == (size_t)c.ysize * fp.plane_stride && end_image == (size_t)c.ysize * c.bytes_per_row, WHERE);
  }
}

template <class F>
void for_each_world(F f) {
  for (int ygroups = 1; ygroups <= 9; ygroups++)
    for (int nranks = 1; nranks <= 8; nranks++)
      for (int full = 0; full < 2; full++) {
        const int ysize = full ? ygroups * 256 : (ygroups - 1) * 256 + 100;
        f(ygroups, nranks, ysize);
      }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "dump")) {
    for_each_world([](int ygroups, int nranks, int ysize) {
      for (int r = 0; r < nranks; r++) {
        const ShardBand b = shard_band(ygroups, ysize, nranks, r);
        std::printf("band %d %d %d %d %d %d %d %d %d\n", ygroups, nranks, ysize, r, b.r0, b.r1, b.y0, b.y1, rows_per_rank(ygroups, nranks));
      }
    });
    return 0;
  }
  for_each_world([](int ygroups, int nranks, int ysize) {
    for (int layout = 0; layout < 2; layout++)
      for (int exchange = 0; exchange < 2; exchange++)
        for (int tmp = 0; tmp < 2; tmp++) {
          Case c{ygroups, nranks, ysize, layout != 0, exchange != 0, tmp, plan_frame(frame_params((uint32_t)ysize), nranks, false), kXsize * 3};
          int r = -1;
          CHECK(c.fp.status == JXLH_OK && c.fp.ygroups == ygroups, WHERE);
          if (c.fp.status != JXLH_OK) continue;
          std::vector<ShardPlan> plans;
          for (r = 0; r < nranks; r++) plans.push_back(plan_shard_rank(shard_in(c), r));
          g_plans += nranks;
          check_same_as_before(c, plans);
          check_pairing(c, plans);
          check_bounds(c, plans);
          if (g_fail) continue;  // (the models index with what the checks above hold in bounds)
          // (without the exchange no rank has an edge -- check_pairing -- and nothing moves; with it the transforms' planes
          // move, whichever set the result ends in)
          if (exchange && !tmp) check_exchange(c, plans);
          if (exchange && !tmp) {  // the gathers read neither the layout of the transforms' planes ...
            if (layout) continue;  // ... nor the exchange; the plane set only picks the buffer, whose size check_bounds holds
            check_gather(c, plans, c.fp.plane_stride, c.fp.gather_elems,
                         [](const ShardPlan& p) { return p.slot_planes; }, [](const ShardPull& p) { return p.planes; }, "planes");
            check_gather(c, plans, c.bytes_per_row, (size_t)nranks * c.fp.rows_per_rank * 256 * c.bytes_per_row,
                         [](const ShardPlan& p) { return p.slot_image; }, [](const ShardPull& p) { return p.image; }, "image");
          }
        }
  });
  if (g_fail) {
    std::printf("shard plan: %d FAILED\n", g_fail);
    return 1;
  }
  std::printf("shard plan: ok (%ld plans)\n", g_plans);
  return 0;
}
