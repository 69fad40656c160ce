// The inverse squeeze of a batch of groups (jxl_hip_local_squeeze.h): a group's squeeze is closed inside the group
// (apply_local.rs:295-348: in_next_avg and out_prev are None), so every image channel of every group is a chain of its
// own -- a base plane and one residual plane per level, all coded channels in the arena.  Two kernels, both with a lane
// per line as in k_squeeze.hip (the recurrence along the squeezed axis is serial):
//   k_modular_local_squeeze_lds    one workgroup per chain walks the levels whose planes fit LDS, k6_unsqueeze_levels'
//                                  way: the running plane in LDS, a level's residuals prefetched into registers while
//                                  the level before runs, only the last of these levels written out.
//   k_modular_local_squeeze_level  one launch per level index beyond those for the whole batch: 64 lines per workgroup;
//                                  vertical steps are coalesced (lanes = adjacent columns), horizontal ones walk rows.
// The arena is read with 4-byte accesses at any alignment.  A chain's last level writes the group's rect of its
// destination plane, any other the chain's own scratch plane; nothing else is written.  No workgroup waits on another.
#include "modular_local_desc.h"
#include "squeeze_device.h"
#include "squeeze_plan.h"  // JXLH_SQL_MAX: the host's fit rule is squeeze_levels_fit

namespace jxlh {
namespace {

__device__ __forceinline__ int32_t* ls_plane(const LsLaunch& a, uint32_t slot) {
  // (a select chain: indexing the kernel argument dynamically would copy it to scratch)
  return slot == 0 ? a.out[0] : slot == 1 ? a.out[1] : slot == 2 ? a.out[2] : a.out[3];
}
// ... and its row stride: a frame plane's and an extra channel's sample store differ (jxl_hip_local_extra.h)
__device__ __forceinline__ size_t ls_stride(const LsLaunch& a, uint32_t slot) {
  return slot == 0 ? a.slot_stride[0] : slot == 1 ? a.slot_stride[1] : slot == 2 ? a.slot_stride[2] : a.slot_stride[3];
}

// one line: n_out outputs from n_out - n_out / 2 averages and n_out / 2 residuals (hsqueeze_scalar / vsqueeze_scalar,
// squeeze.rs:389-437, :576-644, with out_prev = in_next_avg = None).  Element i of the line is at p[i * ep].
template <int U, class Ta, class Tr, class To>
__device__ __forceinline__ void ls_line(Ta a, size_t aep, Tr r, size_t rep, To o, size_t oep, int n_out) {
  const int w = n_out / 2;
  if (w == 0) {  // single output sample (squeeze.rs:468-476, :672-675)
    o[0] = a[0];
    return;
  }
  const bool has_tail = n_out & 1;
  const int n_main = has_tail ? w : w - 1;  // steps whose next_avg = avg[i + 1] exists
  int32_t cur = a[0], d = 0;                // the first `prev` is avg[0] itself
  int i = 0;
  for (; i + U <= n_main; i += U) {  // the operands of U steps in one round trip
    int32_t nx[U], rr[U], va[U], vb[U];
#pragma unroll
    for (int k = 0; k < U; k++) {
      nx[k] = a[(size_t)(i + k + 1) * aep];
      rr[k] = r[(size_t)(i + k) * rep];
    }
#pragma unroll
    for (int k = 0; k < U; k++) {
      unsqueeze_step(cur, rr[k], nx[k], d, va[k], vb[k]);
      cur = nx[k];
    }
#pragma unroll
    for (int k = 0; k < U; k++) {
      o[(size_t)(2 * (i + k)) * oep] = va[k];
      o[(size_t)(2 * (i + k) + 1) * oep] = vb[k];
    }
  }
  for (; i < n_main; i++) {
    const int32_t nx = a[(size_t)(i + 1) * aep];
    int32_t va, vb;
    unsqueeze_step(cur, r[(size_t)i * rep], nx, d, va, vb);
    o[(size_t)(2 * i) * oep] = va;
    o[(size_t)(2 * i + 1) * oep] = vb;
    cur = nx;
  }
  if (!has_tail) {  // last pair: next_avg = avg itself (squeeze.rs:423-433, :608-616)
    int32_t va, vb;
    unsqueeze_step(cur, r[(size_t)(w - 1) * rep], cur, d, va, vb);
    o[(size_t)(2 * w - 2) * oep] = va;
    o[(size_t)(2 * w - 1) * oep] = vb;
  } else {  // odd size: the trailing average is copied (squeeze.rs:434-437, :641-643)
    o[(size_t)(2 * w) * oep] = cur;
  }
}

__global__ __launch_bounds__(256) void k_modular_local_squeeze_lds(const LsLaunch A) {
  // Two plane buffers, swapped per level.  A level's output is twice its input, so only the buffer the LAST level
  // writes has to hold a full tile; the other one (and the residual tile) hold half planes.  Row pitch = width | 1
  // (odd: lane = row and lane = column are both conflict-free).
  constexpr int kFull = kLsTile * (kLsTile + 1), kHalf = kLsTile * (kLsTile / 2 + 1);
  static_assert(kLsTile == JXLH_SQL_MAX && kLsLevels <= JXLH_SQL_LEVELS, "the host decides the fit with squeeze_levels_fit");
  static_assert(kLsTile <= 256 && kLsTile * kLsTile / 256 <= 64 && (kFull + 2 * kHalf) * 4 <= 160 * 1024,
                "a lane per line of 256 threads, <= kResPasses residual passes, the three tiles in LDS");
  __shared__ int32_t s_big[kFull], s_half[kHalf], s_r[kHalf];
  const int tid = threadIdx.x;
  const LsChainDev& C = A.chains[A.items[blockIdx.x].group];
  const int n = (int)C.n_lds;
  // level i reads buf[(i + off) & 1] and writes the other one; the last level must write s_big (index 0)
  const int off = n & 1;
  auto buf = [&](int k) { return (k & 1) ? s_half : s_big; };
  int cw = (int)C.base_w, ch = (int)C.base_h;
  // plane <-> thread mapping without divisions: tx = tid % TW, TW = the power of two >= the plane's width
  auto tile_log2 = [](int width) { return width <= 1 ? 0 : 32 - __builtin_clz((unsigned)(width - 1)); };
  {
    int32_t* b0 = buf(off);
    const int32_t* __restrict__ base = A.arena + C.base_off;
    const uint32_t bstride = C.base_stride;
    const int pc = cw | 1, lg = tile_log2(cw), tx = tid & ((1 << lg) - 1), ty = tid >> lg, rpp = 256 >> lg;
    for (int y = ty; y < ch; y += rpp)
      if (tx < cw) b0[y * pc + tx] = base[(size_t)y * bstride + tx];
  }
  constexpr int kResPasses = 64;
  int32_t rq[kResPasses];
  auto fetch_res = [&](int lv) {
    const int horizontal = (int)C.lv[lv].horizontal, ow = (int)C.lv[lv].out_w, oh = (int)C.lv[lv].out_h;
    const int rw = horizontal ? ow / 2 : ow, rh = horizontal ? oh : oh / 2;
    if (rw == 0 || rh == 0) return;  // a one-sample axis has no residuals (and no plane to read)
    const int32_t* __restrict__ res = A.arena + C.lv[lv].res_off;
    const uint32_t rstride = C.lv[lv].res_stride;
    const int lg = tile_log2(rw), tx = tid & ((1 << lg) - 1), ty = tid >> lg, rpp = 256 >> lg;
    const int txc = min(tx, rw - 1);
#pragma unroll
    for (int j = 0; j < kResPasses; j++) {
      const int y = ty + j * rpp;
      if (j * rpp >= rh) break;  // uniform
      rq[j] = res[(size_t)min(y, rh - 1) * rstride + txc];  // past the plane: a valid sample, never staged
    }
  };
  fetch_res(0);
  for (int lv = 0; lv < n; lv++) {
    const int horizontal = (int)C.lv[lv].horizontal, ow = (int)C.lv[lv].out_w, oh = (int)C.lv[lv].out_h;
    const int rw = horizontal ? ow / 2 : ow, rh = horizontal ? oh : oh / 2;
    const int pc = cw | 1, po = ow | 1, pr = rw | 1;
    {
      const int lg = tile_log2(rw), tx = tid & ((1 << lg) - 1), ty = tid >> lg, rpp = 256 >> lg;
#pragma unroll
      for (int j = 0; j < kResPasses; j++) {
        const int y = ty + j * rpp;
        if (j * rpp >= rh) break;  // uniform
        if (tx < rw && y < rh) s_r[y * pr + tx] = rq[j];
      }
    }
    __syncthreads();
    if (lv + 1 < n) fetch_res(lv + 1);
    const int32_t* cur_buf = buf(lv + off);
    int32_t* nxt_buf = buf(lv + off + 1);
    const int n_lines = horizontal ? oh : ow, n_out = horizontal ? ow : oh;
    if (tid < n_lines)  // element i of line `tid`: horizontal = row tid, vertical = column tid
      ls_line<4>(cur_buf + (horizontal ? tid * pc : tid), (size_t)(horizontal ? 1 : pc), s_r + (horizontal ? tid * pr : tid),
                 (size_t)(horizontal ? 1 : pr), nxt_buf + (horizontal ? tid * po : tid), (size_t)(horizontal ? 1 : po), n_out);
    __syncthreads();
    cw = ow;
    ch = oh;
  }
  {
    const int32_t* fin = buf(n + off);  // = s_big
    int32_t* __restrict__ out;
    size_t ostride;
    if ((uint32_t)n == C.n_levels) {
      ostride = ls_stride(A, C.slot);
      out = ls_plane(A, C.slot) + (size_t)C.y0 * ostride + C.x0;
    } else {
      out = A.scratch + C.scratch_off[(n - 1) & 1];
      ostride = (size_t)cw;
    }
    const int pc = cw | 1, lg = tile_log2(cw), tx = tid & ((1 << lg) - 1), ty = tid >> lg, rpp = 256 >> lg;
    for (int y = ty; y < ch; y += rpp)
      if (tx < cw) out[(size_t)y * ostride + tx] = fin[y * pc + tx];
  }
}

__global__ __launch_bounds__(kLsLines) void k_modular_local_squeeze_level(const LsLaunch A) {
  const LocalItem item = A.items[blockIdx.x];
  const LsChainDev& C = A.chains[item.group];
  const uint32_t i = C.n_lds + A.step;  // (the host lists only chains that have this level)
  const LsLevelDev& L = C.lv[i];
  const bool horizontal = L.horizontal != 0;
  const uint32_t n_lines = horizontal ? L.out_h : L.out_w, n_out = horizontal ? L.out_w : L.out_h;
  const uint32_t l = item.row0 + threadIdx.x;
  if (l >= n_lines) return;
  const int32_t* __restrict__ avg;
  size_t astride;
  if (i == 0) {
    avg = A.arena + C.base_off;
    astride = C.base_stride;
  } else {  // level i - 1's output: rows of its out_w = this level's average width
    avg = A.scratch + C.scratch_off[(i - 1) & 1];
    astride = horizontal ? (L.out_w + 1) / 2 : L.out_w;
  }
  int32_t* __restrict__ out;
  size_t ostride;
  if (i + 1 == C.n_levels) {
    ostride = ls_stride(A, C.slot);
    out = ls_plane(A, C.slot) + (size_t)C.y0 * ostride + C.x0;
  } else {
    out = A.scratch + C.scratch_off[i & 1];
    ostride = L.out_w;
  }
  const int32_t* __restrict__ res = A.arena + L.res_off;
  const size_t rstride = L.res_stride;
  if (horizontal) ls_line<8>(avg + (size_t)l * astride, (size_t)1, res + (size_t)l * rstride, (size_t)1, out + (size_t)l * ostride, (size_t)1, (int)n_out);
  else ls_line<8>(avg + l, astride, res + l, rstride, out + l, ostride, (int)n_out);
}

}  // namespace

void launch_modular_local_squeeze_lds(hipStream_t s, const LsLaunch& a) {
  if (a.n_items == 0) return;
  hipLaunchKernelGGL(k_modular_local_squeeze_lds, dim3(a.n_items), dim3(256), 0, s, a);
}

void launch_modular_local_squeeze_level(hipStream_t s, const LsLaunch& a) {
  if (a.n_items == 0) return;
  hipLaunchKernelGGL(k_modular_local_squeeze_level, dim3(a.n_items), dim3(kLsLines), 0, s, a);
}

}  // namespace jxlh
