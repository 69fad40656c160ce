// K1, family D: the 8x8 special transforms of a frame (see k_vardct_scan.hip for the binning that feeds them).
#include "k_vardct_common.h"

namespace jxlh {
namespace {

// family D: the nine 8x8 special transform types (IDENTITY, DCT2X2, DCT4X4, DCT4X8, DCT8X4, AFV0-3).
// Each lane transforms one block of one channel with the block's 64 coefficients in registers, so a wavefront must
// hold blocks of ONE code path or the nine paths serialise.  The special work list is in raster order (mixed types): a
// wave takes a (chunk of 512 items, type bin) pair, compacts the chunk's items of its bin through a ballot, and runs
// them in batches of kSpecBlk = 21 blocks.  Round 3: the three channels of a batch are transformed TOGETHER -- lane =
// (channel, block), 63 of 64 lanes busy in one pass of the (long, fully unrolled) per-type code -- where round 2 ran the
// transform once per channel on 32 lanes; the tile is in place (a lane reads its row into registers, writes the
// pixels over it) and the dequantised Y a batch's X / B rows need stays in 24 registers.  16K all types: 394 -> see
// profiles/r03_d_large_path.txt.  (kSpecWaves, kSpecThreads, kSpecChunk: k1_plan.h, the grid reads them)
constexpr int kSpecBins = 9;
constexpr int kSpecBlk = 21;                       // blocks per batch: 3 x 21 = 63 transform lanes
constexpr int kSpecIters = (kSpecBlk * 16 + 63) / 64;  // 16-byte groups of one channel of a batch, per lane
__device__ __forceinline__ int special_bin(int type) {  // 1, 2, 3, 12, 13, 14, 15, 16, 17 -> 0..8
  return type <= 3 ? type - 1 : type - 9;
}

// one lane: its block's 64 coefficients into registers, pixels written over them
template <int TYPE>
__device__ __forceinline__ void special_8x8_inplace(float* __restrict__ row, const float* __restrict__ afv_basis = kAfvBasisDev) {
  float c[64], o[64];
#pragma unroll
  for (int i = 0; i < 64; i++) c[i] = row[i];
  special_8x8_t<TYPE>(c, o, afv_basis);
#pragma unroll
  for (int i = 0; i < 64; i++) row[i] = o[i];
}

// BIN0 .. BIN1: the type bins one instantiation handles.  Round 5: two launches -- IDENTITY / DCT2X2 / DCT4X4 / DCT4X8 /
// DCT8X4 (bins 0-4) and AFV0-3 (bins 5-8) -- instead of one: the kernel's registers are the maximum over its bodies, and
// the AFV bodies (a 16 x 16 basis product on top of the 4x4 and 4x8 transforms) set it for everybody (230 VGPRs, 355
// spilled SGPRs, two waves per SIMD).
template <int BIN0, int BIN1>
__global__ __launch_bounds__(kSpecThreads) void k1_special(const FrameDev f, const WorkLists wl) {
  __shared__ float s_tile[kSpecWaves][64 * kSpecPitch];
  __shared__ BlockInfo s_binfo[kSpecWaves][kSpecBlk];
  __shared__ int s_idx[kSpecWaves][kSpecChunk];
  __shared__ AdjTable s_adj;
  __shared__ float s_afv[BIN1 > 5 ? 256 : 1];  // the AFV basis (bins 5-8 only)
  if constexpr (BIN1 > 5)
    for (int i = threadIdx.x; i < 256; i += kSpecThreads) s_afv[i] = kAfvBasisDev[i];
  build_adj_table(f, &s_adj, threadIdx.x, kSpecThreads);  // (ends with a workgroup barrier)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const WorkItem* __restrict__ items = wl.items[kClsSpecial];
  const int count = wl.counts[(kClsSpecial) * kCountPitch];
  float* tile = s_tile[wave];
  BlockInfo* binfo = s_binfo[wave];
  int* mine = s_idx[wave];
  constexpr int kBins = BIN1 - BIN0;
  const int npairs = ((count + kSpecChunk - 1) / kSpecChunk) * kBins;
  for (int pair = blockIdx.x * kSpecWaves + wave; pair < npairs; pair += gridDim.x * kSpecWaves) {
    const int chunk = pair / kBins, bin = BIN0 + pair % kBins;
    // ---- this wave's items of the chunk: the ones whose type falls in `bin`
    int nmine = 0;
    uint32_t packed[kSpecChunk / 64];
#pragma unroll
    for (int i = 0; i < kSpecChunk / 64; i++) {  // all loads in flight before the first ballot
      const int idx = chunk * kSpecChunk + i * 64 + lane;
      packed[i] = items[min(idx, max(count - 1, 0))].packed;
    }
#pragma unroll
    for (int i = 0; i < kSpecChunk / 64; i++) {
      const int idx = chunk * kSpecChunk + i * 64 + lane;
      const bool m = idx < count && special_bin((int)(packed[i] >> 20) & 31) == bin;
      const unsigned long long mask = __ballot(m);
      if (m) mine[nmine + __popcll(mask & ((1ull << lane) - 1ull))] = idx;
      nmine += __popcll(mask);
    }
    wave_sync();
    // every item of the pair has a type of this bin, and the types of a bin share one dequant table
    // (quant_weights.rs:321-343): a wave-uniform pointer instead of a per-lane lookup
    constexpr int kBinType[kSpecBins] = {1, 2, 3, 12, 13, 14, 15, 16, 17};
    int bin_type = kBinType[0];
#pragma unroll
    for (int i = 1; i < kSpecBins; i++) bin_type = bin == i ? kBinType[i] : bin_type;
    const float* __restrict__ bin_table = f.tables + f.table_offset[quant_table_for_type(bin_type)];
    const int k0 = (lane & 15) * 4;  // the four coefficient positions this lane stages, in every block it touches
    for (int b0 = 0; b0 < nmine; b0 += kSpecBlk) {
      const int nb = min(kSpecBlk, nmine - b0);
      if (lane < nb) {
        const WorkItem it = items[mine[b0 + lane]];
        decode_item(f, it, &binfo[lane]);
      }
      wave_sync();
      // ---- stage the three channels: row = ch * kSpecBlk + block, reference order Y, X, B (group.rs:223)
      float dy[4 * kSpecIters];
      auto stage_channel = [&](auto ch_tag) {
        constexpr int CH = decltype(ch_tag)::value;
        const float4 tv = *reinterpret_cast<const float4*>(bin_table + CH * 64 + k0);
        int4 qv[kSpecIters];
        float b_sdy[kSpecIters], b_xcc[kSpecIters], b_bcc[kSpecIters];
#pragma unroll
        for (int j = 0; j < kSpecIters; j++) {  // every global load of the channel in flight first
          const int b = min(j * 4 + (lane >> 4), nb - 1);  // lanes past the batch re-read its last block (discarded)
          const BlockInfo* bp = &binfo[b];
          b_sdy[j] = bp->sdy;
          b_xcc[j] = bp->x_cc;
          b_bcc[j] = bp->b_cc;
          qv[j] = gload_i4<JXLH_NT_COEF>(f.coeffs + bp->coef_off + CH * kGroupArea + k0);
        }
#pragma unroll
        for (int j = 0; j < kSpecIters; j++) {
          const int b = j * 4 + (lane >> 4);
          float d4[4] = {dy[j * 4], dy[j * 4 + 1], dy[j * 4 + 2], dy[j * 4 + 3]};
          BlockInfo bi;
          bi.sdy = b_sdy[j];
          bi.x_cc = b_xcc[j];
          bi.b_cc = b_bcc[j];
          const float4 v = dequant4t<CH>(f, qv[j], tv, bi, &s_adj, d4);
          if constexpr (CH == 1) {
            dy[j * 4] = d4[0];
            dy[j * 4 + 1] = d4[1];
            dy[j * 4 + 2] = d4[2];
            dy[j * 4 + 3] = d4[3];
          }
          if (b < nb) {
            float* dst = tile + (CH * kSpecBlk + b) * kSpecPitch + k0;
            dst[0] = v.x;
            dst[1] = v.y;
            dst[2] = v.z;
            dst[3] = v.w;
          }
        }
      };
      stage_channel(std::integral_constant<int, 1>{});
      stage_channel(std::integral_constant<int, 0>{});
      stage_channel(std::integral_constant<int, 2>{});
      // ---- transform: lane = (channel, block); transform_buffer[0] = lf[0] first
      const int tch = lane / kSpecBlk, tb = lane % kSpecBlk;
      const bool on = tch < 3 && tb < nb;
      const float lf0 = f.lf[min(tch, 2)][binfo[min(tb, nb - 1)].lf_off[min(tch, 2)]];
      wave_sync();
      if (on) {
        float* row = tile + lane * kSpecPitch;  // lane == tch * kSpecBlk + tb
        row[0] = lf0;
        auto in_range = [](int b) { return b >= BIN0 && b < BIN1; };
        // (wave-uniform; only the bodies of this instantiation's bins are compiled in)
        if (in_range(0) && bin == 0) special_8x8_inplace<1>(row);
        if (in_range(1) && bin == 1) special_8x8_inplace<2>(row);
        if (in_range(2) && bin == 2) special_8x8_inplace<3>(row);
        if (in_range(3) && bin == 3) special_8x8_inplace<12>(row);
        if (in_range(4) && bin == 4) special_8x8_inplace<13>(row);
        if (in_range(5) && bin == 5) special_8x8_inplace<14>(row, s_afv);
        if (in_range(6) && bin == 6) special_8x8_inplace<15>(row, s_afv);
        if (in_range(7) && bin == 7) special_8x8_inplace<16>(row, s_afv);
        if (in_range(8) && bin == 8) special_8x8_inplace<17>(row, s_afv);
      }
      wave_sync();
      // ---- store: gather first, then store: all stores of the lane issue back to back
#pragma unroll
      for (int ch = 0; ch < 3; ch++) {
        float* __restrict__ plane = f.planes[ch];
        float4 ov[kSpecIters];
        int oo[kSpecIters];
#pragma unroll
        for (int j = 0; j < kSpecIters; j++) {
          const int b = min(j * 4 + (lane >> 4), nb - 1), p = k0;
          const int px = binfo[b].px_off[ch];
          const float* r = tile + (ch * kSpecBlk + b) * kSpecPitch;
          if (f.tiled) {  // memory order inside the block is (y & 4) * 8 + x * 4 + (y & 3)
            const int x = (p & 31) >> 2, y0 = (p >> 5) * 4;
            const float* src = r + y0 * 8 + x;
            ov[j] = make_float4(src[0], src[8], src[16], src[24]);
            oo[j] = px + p;
          } else {
            ov[j] = make_float4(r[p], r[p + 1], r[p + 2], r[p + 3]);
            oo[j] = px + (p / 8) * (int)f.plane_stride + (p % 8);
          }
        }
#pragma unroll
        for (int j = 0; j < kSpecIters; j++)
          if (j * 4 + (lane >> 4) < nb) *reinterpret_cast<float4*>(plane + oo[j]) = ov[j];
      }
      wave_sync();
    }
    wave_sync();  // `mine` is rewritten by the next pair
  }
}

}  // namespace

void launch_k1_special(hipStream_t s, const K1Step& step, const FrameDev& f, const WorkLists& wl) {
  static constexpr K1ClassKernel kTable[] = {k1_special<0, 5>, k1_special<5, 9>};
  static_assert(sizeof(kTable) / sizeof(kTable[0]) == kK1ClassEnd - kK1Special0, "one kernel per id of k1_plan.h");
  hipLaunchKernelGGL(kTable[step.kernel - kK1Special0], dim3(step.grid), dim3(step.block), 0, s, f, wl);
}

}  // namespace jxlh
