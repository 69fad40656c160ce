// The protocol of a sharded frame: which group rows a rank owns, which block rows it trades with which neighbours
// between the transforms and the filters, and where the finished bands go in the gather -- decided here for one rank,
// issued by comm.hip through either transport (RCCL or the in-process copies).  Plain C++: the planner is host logic,
// reads no context, and is tested without a device for every world size (tests/cpp/shard_plan.cc).
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

namespace jxlh {

// contiguous bands: ceil(ygroups / nranks) group rows per rank; trailing ranks may own nothing
inline int rows_per_rank(int ygroups, int nranks) { return (ygroups + nranks - 1) / nranks; }

// group rows [r0, r1) = pixel rows [y0, y1) of the frame
struct ShardBand {
  int r0 = 0, r1 = 0, y0 = 0, y1 = 0;
  bool empty() const { return r0 >= r1; }
};
inline ShardBand shard_band(int ygroups, int ysize, int nranks, int rank) {
  const int per = rows_per_rank(ygroups, nranks);
  ShardBand b;
  b.r0 = std::min(rank * per, ygroups);
  b.r1 = std::min((rank + 1) * per, ygroups);
  b.y0 = std::min(b.r0 * 256, ysize);
  b.y1 = std::min(b.r1 * 256, ysize);
  return b;
}

// What the decisions read.  tiled, xblocks, plane_stride: the layout the transforms wrote the planes in (FrameDev's
// fields after the run's prologue).  exchange: RunPlan::exchange of the run (a gather has no edges: false).
// result_in_tmp: StageList::result_in_tmp().  bytes_per_row: of the converted image (0: there is none).
struct ShardIn {
  int ygroups = 1, ysize = 1, nranks = 1;
  bool tiled = false;
  int xblocks = 0;
  size_t plane_stride = 0;
  bool exchange = false;
  int result_in_tmp = 0;
  size_t bytes_per_row = 0;
};

struct ShardSpan { size_t off = 0, n = 0; };  // f32 planes: floats; the converted image: bytes

// One band edge with a neighbour that owns rows: the own edge block row (8 pixel rows, in the layout the transforms
// wrote) goes to `peer`, the block row beyond the edge comes from it -- at the same offset there, which is what the
// in-process transport copies.
struct ShardEdge {
  int peer = 0;
  ShardSpan send, recv;
};

// Another rank's finished band, where it lies in every rank's buffers: the rows that exist, no padding.
struct ShardPull {
  int peer = 0;
  ShardSpan planes, image;
};

struct ShardPlan {
  int rank = 0, nranks = 1;
  ShardBand band;
  int rows_per_rank = 0;
  // the geometry the spans were computed in: peers that trade rows must agree on it (same_layout)
  bool tiled = false;
  int xblocks = 0;
  size_t plane_stride = 0;
  // halo exchange, in issue order: the upper edge, then the lower one
  int n_edges = 0;
  ShardEdge edge[2];
  // gather, equal-slot form (in-place all-gather): off = the own slot, n = what every rank contributes, padding included
  ShardSpan slot_planes, slot_image;
  // gather, existing-rows form: the other ranks' bands, ascending, empty ones left out
  std::vector<ShardPull> pulls;
  int result_in_tmp = 0;  // the plane set the finished bands are in (1 = tmp, 0 = planes), run or not
};

inline bool same_layout(const ShardPlan& a, const ShardPlan& b) {
  return a.tiled == b.tiled && a.xblocks == b.xblocks && a.plane_stride == b.plane_stride;
}

inline ShardPlan plan_shard_rank(const ShardIn& in, int rank) {
  ShardPlan p;
  p.rank = rank, p.nranks = in.nranks;
  p.band = shard_band(in.ygroups, in.ysize, in.nranks, rank);
  p.rows_per_rank = rows_per_rank(in.ygroups, in.nranks);
  p.tiled = in.tiled, p.xblocks = in.xblocks, p.plane_stride = in.plane_stride;
  p.result_in_tmp = in.result_in_tmp;
  // one block row of a plane in the layout K1 just wrote
  const size_t row_n = in.tiled ? (size_t)in.xblocks * 64 : 8 * in.plane_stride;
  auto block_row = [&](int by) { return ShardSpan{(size_t)by * row_n, row_n}; };
  // neighbours = the adjacent NON-EMPTY bands (empty bands only trail)
  if (in.exchange && !p.band.empty()) {
    const int up = p.band.r0 * 32, dn = p.band.r1 * 32;  // the first block row of the band, and the first one below it
    if (rank > 0 && !shard_band(in.ygroups, in.ysize, in.nranks, rank - 1).empty())
      p.edge[p.n_edges++] = {rank - 1, block_row(up), block_row(up - 1)};
    if (rank + 1 < in.nranks && !shard_band(in.ygroups, in.ysize, in.nranks, rank + 1).empty())
      p.edge[p.n_edges++] = {rank + 1, block_row(dn - 1), block_row(dn)};
  }
  const size_t slot_rows = (size_t)p.rows_per_rank * 256;
  p.slot_planes = {(size_t)rank * slot_rows * in.plane_stride, slot_rows * in.plane_stride};
  p.slot_image = {(size_t)rank * slot_rows * in.bytes_per_row, slot_rows * in.bytes_per_row};
  for (int k = 0; k < in.nranks; k++) {
    const ShardBand b = shard_band(in.ygroups, in.ysize, in.nranks, k);
    if (k == rank || b.empty()) continue;
    const size_t y0 = (size_t)b.y0, rows = (size_t)(b.y1 - b.y0);
    p.pulls.push_back({k, {y0 * in.plane_stride, rows * in.plane_stride}, {y0 * in.bytes_per_row, rows * in.bytes_per_row}});
  }
  return p;
}

}  // namespace jxlh
