// K6 inverse Squeeze on whole i32 planes (squeeze.rs:107-141, :171-185, :389-437, :576-644): the one-wave, tiled, dataflow,
// fused step + RCT and LDS-resident kernels.  squeeze_plan.h decides which one runs; a launcher launches what it is told.
//
// Squeeze is a non-associative recurrence along the squeezed axis (the previous output b
// feeds the next tendency), so the only parallelism is across lines: one lane per line,
// loads software-pipelined ahead of the dependent chain.  Vertical steps are naturally
// coalesced (lanes = adjacent columns); horizontal steps walk rows (lanes = adjacent rows)
// and lean on L1/L2 for the 128-byte lines they share across iterations.
#include "jxlh_internal.h"
#include "modular_ops_device.h"  // wadd / wsub, rct_op, rct_permute
#include "squeeze_device.h"      // smooth_tendency, unsqueeze_step

namespace jxlh {
namespace {

// One lane per line; up to 3 planes (the channels of one squeeze step) per launch via blockIdx.y.
// Element i of line l lives at p[l*line_pitch + i*elem_pitch].  n_res = floor(n_out/2) residuals
// per line, n_avg = n_out - n_res averages.  The recurrence itself is ~100 dependent cycles per
// step; what must not be exposed is memory latency, so the loads of the NEXT block of U steps
// are in flight while the current block runs (register double buffering).  HVEC: horizontal step
// with 16-byte aligned rows -> int4 loads / stores (a lane walks along its row).
struct SqueezePlanes {
  const int32_t* avg[3];
  const int32_t* res[3];
  int32_t* out[3];
};

#ifndef JXLH_SQ_U
#define JXLH_SQ_U 16
#endif
template <bool HVEC>
__global__ __launch_bounds__(64) void k6_unsqueeze(const SqueezePlanes pl, size_t avg_lp, size_t avg_ep, size_t res_lp,
                                                   size_t res_ep, size_t out_lp, size_t out_ep, int n_lines,
                                                   int n_out) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= n_lines) return;
  const int32_t* __restrict__ a = pl.avg[blockIdx.y] + (size_t)l * avg_lp;
  const int32_t* __restrict__ r = pl.res[blockIdx.y] + (size_t)l * res_lp;
  int32_t* __restrict__ o = pl.out[blockIdx.y] + (size_t)l * out_lp;
  const int w = n_out / 2;
  if (w == 0) {  // single output sample (squeeze.rs:468-476, :672-675)
    o[0] = a[0];
    return;
  }
  const bool has_tail = n_out & 1;
  int32_t cur = a[0];
  int32_t d = 0;  // prev - avg; the first `prev` is avg[0] itself (squeeze.rs:411-414, :591-594)
  constexpr int U = JXLH_SQ_U;  // steps whose inputs are requested ahead (two such blocks are in flight)
  // main body: next_avg = avg[i+1] exists for i < w-1 (or i < w with a tail)
  const int n_main = has_tail ? w : w - 1;
  const int n_blocks = n_main / U;
  int32_t na[U], rr[U], nb[U], rb[U];
  auto load_block = [&](int i0, int32_t(&xa)[U], int32_t(&xr)[U]) {
    if constexpr (HVEC) {
      // avg[i0+1 .. i0+U] is misaligned by one element: fetch avg[i0 .. i0+U+3] as int4 and shift
      int32_t t[U + 4];
#pragma unroll
      for (int k = 0; k < U / 4 + 1; k++) {
        const int4 v = *reinterpret_cast<const int4*>(a + i0 + 4 * k);
        t[4 * k] = v.x; t[4 * k + 1] = v.y; t[4 * k + 2] = v.z; t[4 * k + 3] = v.w;
      }
#pragma unroll
      for (int k = 0; k < U; k++) xa[k] = t[k + 1];
#pragma unroll
      for (int k = 0; k < U / 4; k++) {
        const int4 v = *reinterpret_cast<const int4*>(r + i0 + 4 * k);
        xr[4 * k] = v.x; xr[4 * k + 1] = v.y; xr[4 * k + 2] = v.z; xr[4 * k + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < U; k++) {
        xa[k] = a[(size_t)(i0 + k + 1) * avg_ep];
        xr[k] = r[(size_t)(i0 + k) * res_ep];
      }
    }
  };
  auto run_block = [&](int i0, const int32_t(&xa)[U], const int32_t(&xr)[U]) {
    int32_t va[U], vb[U];
#pragma unroll
    for (int k = 0; k < U; k++) {
      unsqueeze_step(cur, xr[k], xa[k], d, va[k], vb[k]);
      cur = xa[k];
    }
    if constexpr (HVEC) {
#pragma unroll
      for (int k = 0; k < U; k += 2)
        *reinterpret_cast<int4*>(o + 2 * (i0 + k)) = make_int4(va[k], vb[k], va[k + 1], vb[k + 1]);
    } else {
#pragma unroll
      for (int k = 0; k < U; k++) {
        o[(size_t)(2 * (i0 + k)) * out_ep] = va[k];
        o[(size_t)(2 * (i0 + k) + 1) * out_ep] = vb[k];
      }
    }
  };
  // HVEC over-reads avg by up to 3 elements past i0+U: keep the last block(s) for the scalar tail
  const int vec_blocks = HVEC ? max(0, (n_main - 4) / U) : n_blocks;
  int i = 0;
  if (vec_blocks > 0) {
    load_block(0, na, rr);
    int blk = 0;
    for (; blk + 2 <= vec_blocks; blk += 2) {
      load_block((blk + 1) * U, nb, rb);
      run_block(blk * U, na, rr);
      if (blk + 2 < vec_blocks) load_block((blk + 2) * U, na, rr);
      run_block((blk + 1) * U, nb, rb);
    }
    if (blk < vec_blocks) run_block(blk * U, na, rr);
    i = vec_blocks * U;
  }
  for (; i < n_main; i++) {
    const int32_t nxt = a[(size_t)(i + 1) * avg_ep];
    int32_t va, vb;
    unsqueeze_step(cur, r[(size_t)i * res_ep], nxt, d, va, vb);
    o[(size_t)(2 * i) * out_ep] = va;
    o[(size_t)(2 * i + 1) * out_ep] = vb;
    cur = nxt;
  }
  if (!has_tail) {  // last pair: next_avg = avg itself (squeeze.rs:423-433, :608-616)
    int32_t va, vb;
    unsqueeze_step(cur, r[(size_t)(w - 1) * res_ep], cur, d, va, vb);
    o[(size_t)(2 * w - 2) * out_ep] = va;
    o[(size_t)(2 * w - 1) * out_ep] = vb;
  } else {  // odd size: trailing average is copied (squeeze.rs:434-437, :641-643)
    o[(size_t)(2 * w) * out_ep] = cur;
  }
}

}  // namespace

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for the wave's outstanding global
// stores (vmcnt(0)); in the mover / chain kernels below nothing in the workgroup ever reads those back.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// The same recurrence with the memory traffic taken off the chain wave.  In k6_unsqueeze a lane fetches and stores
// its own line: for a horizontal step that is 64 different cache lines per memory instruction, and in both directions
// the address arithmetic and the memory instructions sit in the one instruction stream whose length is the step time.
// Here a workgroup is one CHAIN wave (lane = line, 64 lines) and three MOVER waves: the movers stream chunks of
// JXLH_SQT_S steps through LDS -- coalesced along whichever axis is contiguous in memory, transposed by the LDS layout
// for the horizontal step (the CPU does this with register transposes, squeeze.rs:249-283) -- double-buffered against
// the chain wave, which touches only LDS: 128-bit reads / writes for the horizontal layout (line pitch = 4 mod 32
// dwords: conflict-free), one dword per lane and step for the vertical one.
static_assert(JXLH_SQT_S == 32, "squeeze_plan.h: the vector movers' 8 slots of 64 quads are one 64 x 32 chunk");
#define JXLH_SQT_PI (JXLH_SQT_S + 4)     // line pitch of the input tiles, horizontal layout
#define JXLH_SQT_PO (2 * JXLH_SQT_S + 4) // ... of the output tile
// One workgroup's share of a tiled step: 64 lines of one plane.  Offsets are 32-bit (the launchers keep planes of 2^31
// samples or more on k6_unsqueeze).
struct TiledLines {
  const int32_t* ga;
  const int32_t* gr;
  int32_t* go;
  uint32_t alp, aep, rlp, rep, olp, oep;  // line / element pitches of the average, residual and output planes
  int n_lines, n_out, l0;
  int vec;  // 16-byte accesses are possible: plane bases and the pitches of the non-contiguous axis are multiples of 16
            // bytes, and every byte offset inside a plane fits 32 bits (squeeze_tiled_vec)
};
// Dataflow form (k6_unsqueeze_flow): the averages of this step are the outputs of the step before it, which is still
// RUNNING in other workgroups of the same launch.  Every 64-line group of a step keeps one progress word = output
// samples complete (stored and acknowledged) along ITS lines; a consumer reads the words of the groups its next chunk
// touches before it requests the chunk.  Producer and consumer sit on different XCDs, whose L2s are not coherent:
// outputs are written through and averages read at agent scope (as in k5_palette_delta), so "acknowledged" is
// "visible" and the words need no fence.
struct FlowLink {
  const int* dep;      // the producing step's progress words for this plane (kFlowWordStride apart); nullptr: complete
  int dep_same_axis;   // its lines run along this step's lines (two steps of one direction in a row): same group index
  int* mine;           // this group's progress word
  int* error;          // JXLH_ERR_DEVICE if a wait outlasts the deadline (the result is then undefined, but the launch ends)
  unsigned long long deadline_ticks;  // s_memrealtime ticks (100 MHz)
  unsigned long long wait_ticks;      // out: time this lane spent polling; polls: loads of a progress word
  unsigned int polls;
  // never read, but zeroed by k6_unsqueeze_flow: without these dead stores the compiler allocates the kernel's scalar
  // registers differently and the chain measured 0.17 % slower; left for a change of its own
  unsigned long long phase[6];
};
template <bool FLOW>
__device__ __forceinline__ int32_t ld_avg(const int32_t* p) {
  if constexpr (FLOW) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return *p;
}
template <bool FLOW>
__device__ __forceinline__ void st_out(int32_t* p, int32_t v) {
  if constexpr (FLOW) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}

template <bool HORIZ, bool FLOW>
__device__ __forceinline__ void unsqueeze_tiled_lines(const TiledLines& T, int32_t* __restrict__ s_avg,
                                                      int32_t* __restrict__ s_res, int32_t* __restrict__ s_out,
                                                      FlowLink& F, int* s_pub) {
  constexpr int S = JXLH_SQT_S, PI = JXLH_SQT_PI, PO = JXLH_SQT_PO;
  constexpr int IN_ELEMS = HORIZ ? 64 * PI : 64 * S, OUT_ELEMS = HORIZ ? 64 * PO : 64 * 2 * S;
  const int tid = threadIdx.x;
  const int l0 = T.l0, n_lines = T.n_lines, n_out = T.n_out;
  const int32_t* __restrict__ ga = T.ga;
  const int32_t* __restrict__ gr = T.gr;
  int32_t* __restrict__ go = T.go;
  // w steps produce 2 w samples; an odd line ends with a copied sample.  EVERY step runs through the chunk pipeline
  // (round 2 left the last n % S steps and the closing pair to the chain lane's own global loads: with power-of-two
  // planes that is 31 steps per level whose memory latency sat in the dependent instruction stream, ~10 us per level):
  // the step without a following average (even lines: next_avg = avg itself, squeeze.rs:423-430) is staged with the
  // average index clamped to the last one, and the last chunk may be partial.
  const int w = n_out / 2;
  const bool has_tail = n_out & 1;
  const int n_avg = n_out - w;
  const int n_chunks = (n_out + 2 * S - 1) / (2 * S);   // chunks of 2 S output samples; the last may hold fewer steps
  auto steps_of = [&](int c) { return max(0, min(S, w - c * S)); };
  const bool chain = tid < 64;
  if (chain) __builtin_amdgcn_s_setprio(3);  // the step time IS this wave's issue latency
  const int m = tid - 64;  // mover index 0..191

  // movers: chunk c of the inputs (next_avg = avg[i0 + 1 + k], res[i0 + k]) -> registers -> LDS, in two halves so that
  // all of a chunk's loads are in flight together (and the previous chunk's stores are issued under them)
  // Offsets are 32-bit (the launcher keeps planes of 2^31 samples or more on k6_unsqueeze) and affine in the slot j.
  // Three mover waves: with the chain wave that is one wave per SIMD, and two workgroups share a CU (a fifth wave
  // doubles up on a SIMD and the second workgroup no longer fits: measured, 384 workgroups took two rounds).
  constexpr int NM = 192, NIN = (64 * S + NM - 1) / NM, NOUT = (64 * 2 * S + NM - 1) / NM;
  // horizontal: the element index is the contiguous axis (32 elements of one line per half wave);
  // vertical: the line index is (64 lines of one element row per wave)
  const int in_r0 = HORIZ ? m / S : m % 64, in_k0 = HORIZ ? m % S : m / 64;
  constexpr int IN_DR = HORIZ ? NM / S : 0, IN_DK = HORIZ ? 0 : NM / 64;
  const int out_r0 = HORIZ ? m / (2 * S) : m % 64, out_k0 = HORIZ ? m % (2 * S) : m / 64;
  constexpr int OUT_DR = HORIZ ? NM / (2 * S) : 0, OUT_DK = HORIZ ? 0 : NM / 64;
  const uint32_t alp = T.alp, aep = T.aep, rlp = T.rlp, rep = T.rep, olp = T.olp, oep = T.oep;
  const uint32_t a_off0 = (uint32_t)(l0 + in_r0) * alp + (uint32_t)(1 + in_k0) * aep;
  const uint32_t r_off0 = (uint32_t)(l0 + in_r0) * rlp + (uint32_t)in_k0 * rep;
  const uint32_t o_off0 = (uint32_t)(l0 + out_r0) * olp + (uint32_t)out_k0 * oep;
  const uint32_t a_dj = IN_DR * alp + IN_DK * aep, r_dj = IN_DR * rlp + IN_DK * rep, o_dj = OUT_DR * olp + OUT_DK * oep;
  const int in_lds0 = HORIZ ? in_r0 * PI + in_k0 : in_k0 * 64 + in_r0;
  constexpr int IN_LDS_DJ = HORIZ ? IN_DR * PI : IN_DK * 64;
  const int out_lds0 = HORIZ ? out_r0 * PO + out_k0 : out_k0 * 64 + out_r0;
  constexpr int OUT_LDS_DJ = HORIZ ? OUT_DR * PO : OUT_DK * 64;
  // ---- dataflow form: wait until the producing step has stored the averages [e_lo, e_hi] of this group's lines
  // (each wave that requests averages asks for itself: lane 0 polls, the wave goes on from the reconvergence point)
  int dep_groups_ok = 0, dep_avail = 0;  // wave-uniform: producer groups seen complete for our lines / samples seen
  bool dep_dead = false;
  auto flow_spin = [&](const int* word, int need) -> int {
    int v = need;
    if ((tid & 63) == 0) {
      const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
      int spins = 0;
      F.polls++;
      while ((v = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) < need) {
        F.polls++;
        // back off: hundreds of workgroups of the later levels wait for most of the launch, and their polls all end
        // at the memory channels that hold the words the running levels publish and peek at
#ifndef JXLH_FLOW_NAP
#define JXLH_FLOW_NAP 96
#endif
        if (++spins < 8) __builtin_amdgcn_s_sleep(4);
        else if (spins < 24) __builtin_amdgcn_s_sleep(JXLH_FLOW_NAP < 24 ? JXLH_FLOW_NAP : 24);
        else __builtin_amdgcn_s_sleep(JXLH_FLOW_NAP);
        if ((spins & 255) == 0 && __builtin_amdgcn_s_memrealtime() - t0 > F.deadline_ticks) {
          atomicExch(F.error, JXLH_ERR_DEVICE);
          v = -1;
          break;
        }
      }
      F.wait_ticks += __builtin_amdgcn_s_memrealtime() - t0;
    }
    asm volatile("" ::: "memory");
    return __builtin_amdgcn_readfirstlane(v);
  };
  // The word the NEXT request will ask about is read one iteration ahead (flow_peek, issued behind the iteration's
  // loads and stores): a poll is a round trip to the coherence point, and in front of a chunk's requests it would sit
  // in every iteration's critical sequence (poll, then loads, then the next iteration's staging: measured 5.4 us per
  // chunk instead of 1.7).  A producer that is ahead -- the steady state -- is then seen without waiting.
  int pk_idx = -1, pk_v = 0;  // pk_v: per lane (every lane loads the same word), made uniform where it is used
  auto flow_peek = [&]() {
    if constexpr (FLOW) {
      if (!F.dep || dep_dead) return;
      pk_idx = F.dep_same_axis ? (l0 >> 6) : dep_groups_ok;
      pk_v = __hip_atomic_load(F.dep + pk_idx * kFlowWordStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  };
  auto flow_wait = [&](int e_lo, int e_hi) {
    if constexpr (FLOW) {
      if (!F.dep || dep_dead) return;
      if (F.dep_same_axis) {
        if (pk_idx >= 0) dep_avail = max(dep_avail, __builtin_amdgcn_readfirstlane(pk_v));
        if (dep_avail < e_hi + 1) {
          dep_avail = flow_spin(F.dep + (l0 >> 6) * kFlowWordStride, e_hi + 1);
          dep_dead = dep_avail < 0;
        }
      } else {
        const int need = min(l0 + 64, n_lines);
        dep_groups_ok = max(dep_groups_ok, e_lo >> 6);  // (a wave that joins late -- the scalar tail after vector chunks)
        while (!dep_dead && dep_groups_ok <= (e_hi >> 6)) {
          if (!(pk_idx == dep_groups_ok && __builtin_amdgcn_readfirstlane(pk_v) >= need))
            dep_dead = flow_spin(F.dep + dep_groups_ok * kFlowWordStride, need) < 0;
          dep_groups_ok++;
        }
      }
      pk_idx = -1;
      // nothing the compiler places behind this point may move in front of the reads of the progress word above -- on the
      // path that saw the producer ahead through the peeked word as well as on the spinning one (the
      // hardware side: the word's value has returned before it is compared, and the data was acknowledged at the
      // coherence point before the producer raised the word)
      __atomic_signal_fence(__ATOMIC_SEQ_CST);
    }
  };
  // ... and report: `done` output samples of every line of the group are stored AND acknowledged (the caller's wave
  // has waited for vmcnt(0)); the last of the three mover waves to say so raises the word
  auto flow_publish = [&](int done) {
    if constexpr (FLOW) {
      if ((tid & 63) == 0 && (atomicAdd(s_pub, 1) % 3) == 2)
        __hip_atomic_store(F.mine, done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  };
  auto fetch_chunk = [&](int c, int32_t(&va)[NIN], int32_t(&vr)[NIN]) {
    flow_wait(c * S, min(c * S + S, n_avg - 1));
    if (c * S + S <= w - 1) {  // every next average and residual of the chunk exists: affine offsets
      const uint32_t ca = a_off0 + (uint32_t)(c * S) * aep, cr = r_off0 + (uint32_t)(c * S) * rep;
#pragma unroll
      for (int j = 0; j < NIN; j++) {
        const bool ok = l0 + in_r0 + j * IN_DR < n_lines && m + j * NM < 64 * S;
        va[j] = ok ? ld_avg<FLOW>(ga + (ca + j * a_dj)) : 0;
        vr[j] = ok ? gr[cr + j * r_dj] : 0;
      }
    } else {  // the line's end: clamp the element indices (next_avg of the last step = the last average)
#pragma unroll
      for (int j = 0; j < NIN; j++) {
        const int row = in_r0 + j * IN_DR, k = in_k0 + j * IN_DK;
        const bool ok = l0 + row < n_lines && m + j * NM < 64 * S && c * S + k < w;
        const int ia = min(c * S + 1 + k, n_avg - 1), ir = min(c * S + k, max(w - 1, 0));
        va[j] = ok ? ld_avg<FLOW>(ga + ((uint32_t)(l0 + row) * alp + (uint32_t)ia * aep)) : 0;
        vr[j] = ok ? gr[(uint32_t)(l0 + row) * rlp + (uint32_t)ir * rep] : 0;
      }
    }
  };
  auto stage_chunk = [&](int c, const int32_t(&va)[NIN], const int32_t(&vr)[NIN]) {
#pragma unroll
    for (int j = 0; j < NIN; j++) {
      if (m + j * NM < 64 * S) {
        s_avg[(c & 1) * IN_ELEMS + in_lds0 + j * IN_LDS_DJ] = va[j];
        s_res[(c & 1) * IN_ELEMS + in_lds0 + j * IN_LDS_DJ] = vr[j];
      }
    }
  };
  auto store_chunk = [&](int c) {
    const int32_t* so = s_out + (c & 1) * OUT_ELEMS;
    const uint32_t co = o_off0 + (uint32_t)(2 * c * S) * oep;
    const int count = min(2 * S, n_out - 2 * c * S);  // samples of the chunk (the last one may be partial)
    int32_t v[NOUT];
#pragma unroll
    for (int j = 0; j < NOUT; j++) v[j] = m + j * NM < 64 * 2 * S ? so[out_lds0 + j * OUT_LDS_DJ] : 0;
#pragma unroll
    for (int j = 0; j < NOUT; j++)
      if (l0 + out_r0 + j * OUT_DR < n_lines && m + j * NM < 64 * 2 * S && out_k0 + j * OUT_DK < count)
        st_out<FLOW>(go + (co + j * o_dj), v[j]);
  };


  // ---- vector movers.  The dword movers above spend ~2.1 us of instruction issue per chunk (44 memory instructions
  // per lane, each behind its own bounds test and address arithmetic: measured per phase, profiles/r05_i_*) against
  // the chain wave's 1.6-1.7 us: every tiled step was bound by its MOVERS.  Where the planes allow 16-byte accesses,
  // the group is complete and every step of the chunk has a following average (all but the last one or two chunks of
  // a line), a chunk moves as 16 + 16 + 16 buffer instructions of 128 bits with offsets affine in the slot, split by
  // role as in k6_unsqueeze_rct: wave 1 loads (only loads outstanding: its wait at the staging is for requests a whole
  // iteration old), waves 2 and 3 store (only stores outstanding: exactly eight per iteration, so "all but the newest
  // eight acknowledged" is a precise vmcnt(8) -- what the dataflow form publishes on).
  const bool vec_ok = T.vec && l0 + 64 <= n_lines;
  const int n_fast = vec_ok && w >= 1 ? (w - 1) / S : 0;  // chunks c with c S + S <= w - 1 (a prefix of the line)
  const bool vloader = tid >= 64 && tid < 128;
  const int ms = tid - 128;  // vector storer index 0..127
  constexpr int kAuxCoherent = 16;  // sc1: agent scope (write-through store / load at the coherence point)
  constexpr int kAuxLd = FLOW ? kAuxCoherent : 0, kAuxSt = kAuxLd;
  // (the bases are the same for the whole workgroup; said explicitly, or the dataflow kernel -- where they come out of a
  // level table indexed by the ticket -- gets a readfirstlane loop around every buffer instruction)
  auto uniform_ptr = [](const int32_t* p) {
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    typedef __attribute__((address_space(1))) int32_t global_i32;
    return (int32_t*)(global_i32*)((uint64_t)hi << 32 | lo);
  };
  const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(ga + (size_t)l0 * alp), 0, -1, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_r = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(gr + (size_t)l0 * rlp), 0, -1, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_o = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(go + (size_t)l0 * olp), 0, -1, 0x00020000);
  // loader slot j = 0..7: horizontal (line (m >> 3) + 8 j, quad m & 7), vertical (row (m >> 4) + 4 j, quad m & 15)
  const uint32_t vl_a0 = HORIZ ? ((uint32_t)(m >> 3) * alp + 4u * (m & 7)) * 4u : ((uint32_t)(m >> 4) * aep + 4u * (m & 15)) * 4u;
  const uint32_t vl_r0 = HORIZ ? ((uint32_t)(m >> 3) * rlp + 4u * (m & 7)) * 4u : ((uint32_t)(m >> 4) * rep + 4u * (m & 15)) * 4u;
  const uint32_t vl_adj = HORIZ ? 32u * alp : 16u * aep, vl_rdj = HORIZ ? 32u * rlp : 16u * rep;
  const int vl_lds0 = HORIZ ? (m >> 3) * PI + 4 * (m & 7) : (m >> 4) * 64 + 4 * (m & 15);
  constexpr int VL_LDS_DJ = HORIZ ? 8 * PI : 4 * 64;
  // storer slot j = 0..7: horizontal (line (ms >> 4) + 8 j, quad ms & 15), vertical (row (ms >> 4) + 8 j, quad ms & 15)
  const uint32_t vs_o0 = HORIZ ? ((uint32_t)(ms >> 4) * olp + 4u * (ms & 15)) * 4u : ((uint32_t)(ms >> 4) * oep + 4u * (ms & 15)) * 4u;
  const uint32_t vs_odj = HORIZ ? 32u * olp : 32u * oep;
  const int vs_lds0 = HORIZ ? (ms >> 4) * PO + 4 * (ms & 15) : (ms >> 4) * 64 + 4 * (ms & 15);
  constexpr int VS_LDS_DJ = HORIZ ? 8 * PO : 8 * 64;
  jxlh_i32x4 qa[8], qr[8];
  int32_t qt = 0;  // horizontal: the 33rd average of the line (element c S + 32), one line per lane
  auto fetch_fast = [&](int c) {
    flow_wait(c * S, min(c * S + S, n_avg - 1));
    // horizontal: the aligned quads avg[c S + 4 q ..] (next_avg[k] = avg[c S + 1 + k] is one element further: the
    // staging shifts); vertical: rows c S + 1 + row
    const uint32_t sa = HORIZ ? (uint32_t)(c * S) * 4u : (uint32_t)(c * S + 1) * aep * 4u;
    const uint32_t sr = HORIZ ? (uint32_t)(c * S) * 4u : (uint32_t)(c * S) * rep * 4u;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      qa[j] = __builtin_amdgcn_raw_buffer_load_b128(rs_a, vl_a0 + j * vl_adj, sa, kAuxLd);
      qr[j] = __builtin_amdgcn_raw_buffer_load_b128(rs_r, vl_r0 + j * vl_rdj, sr, 0);
    }
    if constexpr (HORIZ) qt = __builtin_amdgcn_raw_buffer_load_b32(rs_a, (uint32_t)m * alp * 4u, sa + 4u * S, kAuxLd);
  };
  auto stage_fast = [&](int c) {
    int32_t* da = s_avg + (c & 1) * IN_ELEMS + vl_lds0;
    int32_t* dr = s_res + (c & 1) * IN_ELEMS + vl_lds0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      *reinterpret_cast<jxlh_i32x4*>(dr + j * VL_LDS_DJ) = qr[j];
      if constexpr (HORIZ) {
        int32_t* q = da + j * VL_LDS_DJ - 1;  // position k = 4 q + t - 1 of the line
        if ((m & 7) != 0) q[0] = qa[j].x;
        q[1] = qa[j].y;
        q[2] = qa[j].z;
        q[3] = qa[j].w;
      } else {
        *reinterpret_cast<jxlh_i32x4*>(da + j * VL_LDS_DJ) = qa[j];
      }
    }
    if constexpr (HORIZ) s_avg[(c & 1) * IN_ELEMS + m * PI + S - 1] = qt;
  };
  auto store_fast = [&](int c) {
    const int32_t* so = s_out + (c & 1) * OUT_ELEMS + vs_lds0;
    const uint32_t soff = HORIZ ? (uint32_t)(2 * c * S) * 4u : (uint32_t)(2 * c * S) * oep * 4u;
    jxlh_i32x4 v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = *reinterpret_cast<const jxlh_i32x4*>(so + j * VS_LDS_DJ);
#pragma unroll
    for (int j = 0; j < 8; j++) __builtin_amdgcn_raw_buffer_store_b128(v[j], rs_o, vs_o0 + j * vs_odj, soff, kAuxSt);
  };

  const int l = l0 + tid;  // chain lanes
  int32_t cur = 0, d = 0;
  if (chain) {
    flow_wait(0, 0);
    if (l < n_lines) cur = ld_avg<FLOW>(ga + (uint32_t)l * alp);
  }
  // mover schedule, iteration c: stage chunk c + 1 (fetched during iteration c - 1: its latency is a whole iteration
  // old), fetch chunk c + 2 into registers, drain the outputs of chunk c - 1
  int32_t pa[NIN], pr[NIN];
  if (!chain && steps_of(0) > 0) {
    if (0 < n_fast) {
      if (vloader) {
        fetch_fast(0);
        stage_fast(0);
      }
    } else {
      fetch_chunk(0, pa, pr);
      stage_chunk(0, pa, pr);
    }
    if (steps_of(1) > 0) {
      if (1 < n_fast) {
        if (vloader) fetch_fast(1);
      } else {
        fetch_chunk(1, pa, pr);
      }
    }
    if (steps_of(2) > 0 && (vloader || 2 >= n_fast)) flow_peek();
  }
  lds_barrier();
  // the chain wave's chunk c: LDS in, LDS out
  auto chain_chunk = [&](int c) {
    const int32_t* ia = s_avg + (c & 1) * IN_ELEMS;
    const int32_t* ir = s_res + (c & 1) * IN_ELEMS;
    int32_t* oa = s_out + (c & 1) * OUT_ELEMS;
    const int sc = steps_of(c);
    if (sc == S) {
      int32_t xa[S], xr[S];
      if constexpr (HORIZ) {
#pragma unroll
        for (int j = 0; j < S / 4; j++) {
          const int4 va = *reinterpret_cast<const int4*>(ia + tid * PI + 4 * j);
          const int4 vr = *reinterpret_cast<const int4*>(ir + tid * PI + 4 * j);
          xa[4 * j] = va.x; xa[4 * j + 1] = va.y; xa[4 * j + 2] = va.z; xa[4 * j + 3] = va.w;
          xr[4 * j] = vr.x; xr[4 * j + 1] = vr.y; xr[4 * j + 2] = vr.z; xr[4 * j + 3] = vr.w;
        }
      } else {
#pragma unroll
        for (int k = 0; k < S; k++) {
          xa[k] = ia[k * 64 + tid];
          xr[k] = ir[k * 64 + tid];
        }
      }
#pragma unroll
      for (int k = 0; k < S; k += 2) {
        int32_t a0, b0, a1, b1;
        unsqueeze_step(cur, xr[k], xa[k], d, a0, b0);
        unsqueeze_step(xa[k], xr[k + 1], xa[k + 1], d, a1, b1);
        cur = xa[k + 1];
        if constexpr (HORIZ) {
          *reinterpret_cast<int4*>(oa + tid * PO + 2 * k) = make_int4(a0, b0, a1, b1);
        } else {
          oa[(2 * k) * 64 + tid] = a0;
          oa[(2 * k + 1) * 64 + tid] = b0;
          oa[(2 * k + 2) * 64 + tid] = a1;
          oa[(2 * k + 3) * 64 + tid] = b1;
        }
      }
    } else {  // the line's last chunk: fewer steps, one by one; an odd line's copied sample behind them
      for (int k = 0; k < sc; k++) {
        const int32_t nxt = HORIZ ? ia[tid * PI + k] : ia[k * 64 + tid];
        const int32_t rs = HORIZ ? ir[tid * PI + k] : ir[k * 64 + tid];
        int32_t va, vb;
        unsqueeze_step(cur, rs, nxt, d, va, vb);
        cur = nxt;
        if constexpr (HORIZ) {
          oa[tid * PO + 2 * k] = va;
          oa[tid * PO + 2 * k + 1] = vb;
        } else {
          oa[(2 * k) * 64 + tid] = va;
          oa[(2 * k + 1) * 64 + tid] = vb;
        }
      }
      if (has_tail) {  // n_out odd: sample 2 w = avg[w] (squeeze.rs:434-437), always in the last chunk
        if constexpr (HORIZ) oa[tid * PO + 2 * sc] = cur;
        else oa[(2 * sc) * 64 + tid] = cur;
      }
    }
    };
  // the movers' iteration c in general (any mix of vector and dword chunks, the line's end)
  auto mover_general = [&](int c) {
    if (steps_of(c + 1) > 0) {
      if (c + 1 < n_fast) {
        if (vloader) stage_fast(c + 1);
      } else {
        stage_chunk(c + 1, pa, pr);
      }
    }
    if constexpr (FLOW) {
      // Report chunk c - 3, stored during iteration c - 2.  No wait of its own: vector memory operations of a wave
      // complete in the order they were issued, the staging above has just consumed loads issued AFTER those stores
      // (iteration c - 1), so they are acknowledged.  A wait for the stores themselves -- vmcnt(0) here -- would
      // also wait for the stores of iteration c - 1, a write-through round trip that is longer than the chain
      // wave's chunk: measured 3.0-3.2 us per chunk instead of 1.7.  Where that argument has a hole (nothing staged
      // at a line's end; a group with fewer than 64 lines, where a wave may hold stores but no loads) the wait is
      // explicit.
      // Vector chunks: chunks c - 3 and c - 2 both went out as the storer waves' eight stores per iteration, so
      // "all but the newest eight acknowledged" is exact (the loader wave has no stores to wait for).
      if (c >= 3) {
        if (c - 2 < n_fast) {
          if (!vloader) __builtin_amdgcn_s_waitcnt(0x0f78);  // vmcnt(8)
        } else if (n_fast > 0 || steps_of(c + 1) == 0 || l0 + 64 > n_lines) {
          __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0)
        }
        asm volatile("" ::: "memory");
        flow_publish(min(n_out, 2 * S * (c - 2)));
      }
    }
    if (steps_of(c + 2) > 0) {
      if (c + 2 < n_fast) {
        if (vloader) fetch_fast(c + 2);
      } else {
        fetch_chunk(c + 2, pa, pr);
      }
    }
    // (before the stores: reading it back must not wait for them)
    if (steps_of(c + 3) > 0 && (vloader || c + 3 >= n_fast)) flow_peek();
    if (c >= 1) {
      if (c - 1 < n_fast) {
        if (!vloader) store_fast(c - 1);
      } else {
        store_chunk(c - 1);
      }
    }
  };
  // ... and while chunks c - 1, c + 1 and c + 2 are all vector chunks: the same schedule with nothing but the vector
  // movers in the loop.  Kept apart because the compiler's wait insertion does not follow which path a wave took: with
  // the dword movers' registers and requests in the same loop it put a wait for ALL outstanding memory operations
  // in front of the loader's next request (0.9 us per iteration, profiles/r05_i_*).
  auto mover_steady = [&](int c) {
    if (vloader) {
      stage_fast(c + 1);
      if constexpr (FLOW) {
        if (c >= 3) flow_publish(min(n_out, 2 * S * (c - 2)));
      }
      fetch_fast(c + 2);
      if (steps_of(c + 3) > 0) flow_peek();
    } else {
      if constexpr (FLOW) {
        if (c >= 3) {
          __builtin_amdgcn_s_waitcnt(0x0f78);  // vmcnt(8): everything but the previous iteration's eight stores
          asm volatile("" ::: "memory");
          flow_publish(min(n_out, 2 * S * (c - 2)));
        }
      }
      if (c >= 1) store_fast(c - 1);
    }
  };
  int c = 0;
  for (; c + 2 < n_fast; c++) {
    if (chain) chain_chunk(c);
    else mover_steady(c);
    lds_barrier();
  }
  for (; c < n_chunks; c++) {
    if (chain) chain_chunk(c);
    else mover_general(c);
    lds_barrier();
  }
  if (!chain && n_chunks > 0) {
    if (n_chunks - 1 < n_fast) {
      if (!vloader) store_fast(n_chunks - 1);
    } else {
      store_chunk(n_chunks - 1);
    }
    if constexpr (FLOW) {
      __builtin_amdgcn_s_waitcnt(0x0f70);
      flow_publish(n_out);
    }
  }
}


template <bool HORIZ>
__global__ __launch_bounds__(256) void k6_unsqueeze_tiled(const SqueezePlanes pl, size_t avg_lp, size_t avg_ep,
                                                          size_t res_lp, size_t res_ep, size_t out_lp, size_t out_ep,
                                                          int n_lines, int n_out, int vec) {
  constexpr int S = JXLH_SQT_S, PI = JXLH_SQT_PI, PO = JXLH_SQT_PO;
  constexpr int IN_ELEMS = HORIZ ? 64 * PI : 64 * S, OUT_ELEMS = HORIZ ? 64 * PO : 64 * 2 * S;
  __shared__ __attribute__((aligned(16))) int32_t s_avg[2 * IN_ELEMS];
  __shared__ __attribute__((aligned(16))) int32_t s_res[2 * IN_ELEMS];
  __shared__ __attribute__((aligned(16))) int32_t s_out[2 * OUT_ELEMS];
  TiledLines T;
  T.ga = pl.avg[blockIdx.y];
  T.gr = pl.res[blockIdx.y];
  T.go = pl.out[blockIdx.y];
  T.alp = (uint32_t)avg_lp; T.aep = (uint32_t)avg_ep; T.rlp = (uint32_t)res_lp; T.rep = (uint32_t)res_ep;
  T.olp = (uint32_t)out_lp; T.oep = (uint32_t)out_ep;
  T.n_lines = n_lines; T.n_out = n_out; T.l0 = blockIdx.x * 64;
  T.vec = vec;
  FlowLink F{};
  unsqueeze_tiled_lines<HORIZ, false>(T, s_avg, s_res, s_out, F, nullptr);
}

// ---- The streamed levels of a squeeze chain as ONE launch (dataflow).  Run level by level, a chain costs the SUM of
// its levels' line lengths in dependent steps (16 368 for 8192^2: every level waits for the whole level before it).
// But a step only needs the averages NEAR its own position: row group g of a horizontal step can start as soon as the
// vertical step before it has finished rows [64 g, 64 g + 64) -- in all its column groups, which advance together --
// and a column group of the NEXT vertical step follows the row groups of this one at half their speed.  The critical
// path is then monotone in both image axes: about one line of the finest horizontal level plus one of the finest
// vertical one, not the sum over the levels; coarse levels finish under the start of the fine ones.
// Workgroups take tickets (an atomic counter) and tickets are handed out level by level, lowest group first: a
// workgroup only ever waits for lower tickets, which are running or done -- no residency assumption, no deadlock.
// Each level writes its own plane set (no ping-pong: level i + 2 would overwrite what level i + 1 still reads).
struct FlowLevel {
  const int32_t* avg[3];
  const int32_t* res[3];
  int32_t* out[3];
  uint32_t avg_lp, avg_ep, res_lp, res_ep, out_lp, out_ep;
  int n_lines, n_out;
  int horiz;
  int first_wg;  // ticket of the level's first workgroup; workgroup = group * n_planes + plane
  int groups;    // 64-line groups per plane
  int flag0;     // index of the level's first progress word (plane-major)
  int dep_same_axis;
  int vec;  // TiledLines::vec
};
struct FlowArgs {
  int n_levels, n_planes;
  int* ticket;    // zero at launch
  int* progress;  // zero at launch
  int* error;
  unsigned long long deadline_ticks;
  // optional profile (nullptr: none), five rows of kFlowMaxLevels: first start (min, preset to ~0), last end (max), time
  // the first mover wave of every workgroup spent polling (sum), its polls (sum), workgroup lifetimes (sum);
  // s_memrealtime ticks
  unsigned long long* prof;
  FlowLevel lv[kFlowMaxLevels];
};
__global__ __launch_bounds__(256) void k6_unsqueeze_flow(const FlowArgs A) {
  constexpr int PI = JXLH_SQT_PI, PO = JXLH_SQT_PO;
  __shared__ __attribute__((aligned(16))) int32_t s_avg[2 * 64 * PI];
  __shared__ __attribute__((aligned(16))) int32_t s_res[2 * 64 * PI];
  __shared__ __attribute__((aligned(16))) int32_t s_out[2 * 64 * PO];
  __shared__ int s_ticket, s_pub;
  if (threadIdx.x == 0) {
    s_ticket = atomicAdd(A.ticket, 1);
    s_pub = 0;
  }
  __syncthreads();
  const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
  const int t = __builtin_amdgcn_readfirstlane(s_ticket);
  int li = 0;
  for (int i = 1; i < A.n_levels; i++) li = t >= A.lv[i].first_wg ? i : li;
  const FlowLevel& L = A.lv[li];
  // everything below is the same for the whole workgroup; the compiler does not see it (the level is found by the
  // ticket, the ticket comes out of LDS) and would do the address arithmetic per lane: said explicitly
  auto uni = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane(v); };
  auto uni_ptr = [&](const int32_t* p) {
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    // (through a global-address-space pointer: rebuilt from an integer it would be a generic one, and every access
    // through it a flat_ instruction, which counts on both memory counters)
    typedef __attribute__((address_space(1))) int32_t global_i32;
    return (int32_t*)(global_i32*)((uint64_t)uni((uint32_t)(v >> 32)) << 32 | uni((uint32_t)v));
  };
  const int local = t - (int)uni(L.first_wg), n_planes = (int)uni(A.n_planes);
  const int plane = (int)uni(local % n_planes), g = (int)uni(local / n_planes);
  TiledLines T;
  T.ga = uni_ptr(L.avg[plane]);
  T.gr = uni_ptr(L.res[plane]);
  T.go = uni_ptr(L.out[plane]);
  T.alp = uni(L.avg_lp); T.aep = uni(L.avg_ep); T.rlp = uni(L.res_lp); T.rep = uni(L.res_ep);
  T.olp = uni(L.out_lp); T.oep = uni(L.out_ep);
  T.n_lines = (int)uni(L.n_lines); T.n_out = (int)uni(L.n_out); T.l0 = g * 64;
  T.vec = (int)uni(L.vec);
  FlowLink F;
  F.dep = li > 0 ? uni_ptr(A.progress + (A.lv[li - 1].flag0 + plane * A.lv[li - 1].groups) * kFlowWordStride) : nullptr;
  F.dep_same_axis = (int)uni(L.dep_same_axis);
  F.mine = uni_ptr(A.progress + (L.flag0 + plane * L.groups + g) * kFlowWordStride);
  F.error = A.error;
  F.deadline_ticks = A.deadline_ticks;
  F.wait_ticks = 0;
  F.polls = 0;
  for (int i = 0; i < 6; i++) F.phase[i] = 0;
  if (uni(L.horiz)) unsqueeze_tiled_lines<true, true>(T, s_avg, s_res, s_out, F, &s_pub);
  else unsqueeze_tiled_lines<false, true>(T, s_avg, s_res, s_out, F, &s_pub);
  if (A.prof && threadIdx.x == 64) {
    atomicMin(&A.prof[li], t_start);
    atomicMax(&A.prof[kFlowMaxLevels + li], (unsigned long long)__builtin_amdgcn_s_memrealtime());
    atomicAdd(&A.prof[2 * kFlowMaxLevels + li], F.wait_ticks);
    atomicAdd(&A.prof[3 * kFlowMaxLevels + li], (unsigned long long)F.polls);
    atomicAdd(&A.prof[4 * kFlowMaxLevels + li], (unsigned long long)__builtin_amdgcn_s_memrealtime() - t_start);
  }
}

// The last step of a colour image's squeeze chain is an unsqueeze of three channels at full size (vertical for square
// and tall images, horizontal for wide ones: default_squeeze, squeeze.rs:71-105), and the transform that follows it in
// the inverse chain is the RCT on the same three channels: a second full read and write of the image.  Fused form:
// the chain wave's lanes are 3 planes x NL lines, so that the three channel values of every output sample meet in one
// workgroup's LDS tile, and the movers apply rct_op while they drain it.  NL = 21 lines for the horizontal step (63
// lanes); 16 columns for the vertical one (48 lanes), so that the per-plane row segments the movers touch are whole
// 64-byte sectors.  The remainder of a line (what k6_unsqueeze_tiled leaves to the chain lane's own stores) goes
// through the tile as well, as a partial chunk.
// NCW = chain waves: 2 widens the vertical tile to 32 columns per plane (96 chain lanes in two waves), so that the
// movers touch whole 128-byte lines of every plane row; vector movers only.
template <bool HORIZ, bool VEC, int NCW = 1>
__global__ __launch_bounds__(64 * (3 * NCW + 1)) void k6_unsqueeze_rct(const SqueezePlanes pl, uint32_t avg_lp, uint32_t avg_ep,
                                                        uint32_t res_lp, uint32_t res_ep, uint32_t out_lp,
                                                        uint32_t out_ep, int n_lines, int n_out, int op, int perm) {
  static_assert(NCW == 1 || (VEC && !HORIZ), "two chain waves: vertical step with the vector movers");
  constexpr int S = JXLH_SQT_S, PI = JXLH_SQT_PI, PO = JXLH_SQT_PO, NL = HORIZ ? 21 : 16 * NCW, NM = 192;
  constexpr int RP = 64 * NCW;   // tile rows (= chain lanes) of the vertical layout
  constexpr int QN = NL / 4;     // 4-column quads per plane row (vector movers)
  constexpr int NLW = NCW;       // loader waves of the vector movers (the wide tile has twice the slots)
  constexpr int NIN = VEC ? 4 * ((S * 3 * QN + 64 * NLW - 1) / (64 * NLW)) : (64 * S + NM - 1) / NM, NPIX = (NL * 2 * S + NM - 1) / NM;
  constexpr int IN_ELEMS = HORIZ ? 64 * PI : RP * S, OUT_ELEMS = HORIZ ? 64 * PO : RP * 2 * S;
  __shared__ __attribute__((aligned(16))) int32_t s_avg[2][IN_ELEMS];
  __shared__ __attribute__((aligned(16))) int32_t s_res[2][IN_ELEMS];
  __shared__ __attribute__((aligned(16))) int32_t s_out[2][OUT_ELEMS];
  const int tid = threadIdx.x;
  const int l0 = blockIdx.x * NL;
  // every step through the chunk pipeline, the last chunk possibly partial (see k6_unsqueeze_tiled)
  const int w = n_out / 2;
  const bool has_tail = n_out & 1;
  const int n_avg = n_out - w;
  const int n_chunks = (n_out + 2 * S - 1) / (2 * S);
  auto steps_of = [&](int c) { return max(0, min(S, w - c * S)); };
  const bool chain = tid < 64 * NCW;
  if (chain) __builtin_amdgcn_s_setprio(3);  // the step time IS this wave's issue latency
  // Mover roles.  The scalar movers (m = 0..191) both load and store.  The vector movers are split, NCW waves loading
  // and NCW + 1 waves storing: a wave with loads and stores outstanding waits for the stores' acknowledgements whenever it
  // needs a loaded value (one in-order vmcnt), which with a handful of wide instructions per chunk is all it does.
  constexpr int MB = 64 * NCW;  // first mover thread
  const bool loader = VEC ? (tid >= MB && tid < MB + 64 * NLW) : !chain, storer = VEC ? tid >= MB + 64 * NLW : !chain;
  const int m = VEC ? (tid < MB + 64 * NLW ? tid - MB : tid - MB - 64 * NLW) : tid - 64;
  constexpr int NML = VEC ? 64 * NLW : 192, NMS = VEC ? 64 * (NCW + 1) : 192;  // storer waves: 2 (3 for the wide tile)
  // perm: which output plane receives w0 / w1 / w2 (as k4_rct)
  int32_t *o0, *o1, *o2;
  switch (perm) {
    default:
    case 0: o0 = pl.out[0]; o1 = pl.out[1]; o2 = pl.out[2]; break;
    case 1: o0 = pl.out[1]; o1 = pl.out[2]; o2 = pl.out[0]; break;
    case 2: o0 = pl.out[2]; o1 = pl.out[0]; o2 = pl.out[1]; break;
    case 3: o0 = pl.out[0]; o1 = pl.out[2]; o2 = pl.out[1]; break;
    case 4: o0 = pl.out[1]; o1 = pl.out[0]; o2 = pl.out[2]; break;
    case 5: o0 = pl.out[2]; o1 = pl.out[1]; o2 = pl.out[0]; break;
  }
  // plane p of a channel triple as base + masked byte offsets (a select chain over three pointers is turned into a
  // table in scratch memory by the compiler, and a scratch load in front of every global load)
  const int64_t a_d1 = (const char*)pl.avg[1] - (const char*)pl.avg[0], a_d2 = (const char*)pl.avg[2] - (const char*)pl.avg[0];
  const int64_t r_d1 = (const char*)pl.res[1] - (const char*)pl.res[0], r_d2 = (const char*)pl.res[2] - (const char*)pl.res[0];
  auto plane_ptr = [](const int32_t* base, int64_t d1, int64_t d2, int p) {
    const int64_t off = (-(int64_t)(p == 1) & d1) | (-(int64_t)(p == 2) & d2);
    return (const int32_t*)((const char*)base + off);
  };
  // tile row r = plane * NL + line; rows from 3 NL on are unused
  auto row_of = [&](int r, int& p, int& q) {
    p = r / NL;
    q = r - p * NL;
    return r < 3 * NL && l0 + q < n_lines;
  };
  // tile position of (row r, element k): one line per row of PI / PO dwords for the horizontal step (the chain lane
  // reads its row with 128-bit accesses), one element row of 64 lanes for the vertical one
  auto in_idx = [](int r, int k) { return HORIZ ? r * PI + k : k * RP + r; };
  auto out_idx = [](int r, int k) { return HORIZ ? r * PO + k : k * RP + r; };
  // VEC (vertical step, 16-byte aligned planes, column count a multiple of 4): a mover slot is four columns of one
  // plane's element row -- 16 row segments of 64 bytes per wave instruction instead of three (or four, when storing),
  // which is what this step's throughput hangs on once three planes stream through every workgroup.  The register
  // arrays then hold int4 slots: (k, plane, quad) for the inputs, (k, quad) for the outputs.
  static_assert(!(VEC && HORIZ), "the vector movers are for the vertical step");
  constexpr int NVIN = (S * 3 * QN + NML - 1) / NML, NVOUT = (2 * S * QN + NMS - 1) / NMS;
  auto fetch_chunk = [&](int c, int32_t(&va)[NIN], int32_t(&vr)[NIN]) {
    if constexpr (VEC) {
#pragma unroll
      for (int j = 0; j < NVIN; j++) {
        const int f = m + j * NML, k = f / (3 * QN), rem = f - k * (3 * QN), p = rem / QN, qq = rem % QN;
        // slots past the tile (the last j) and quads past the last column read a valid address instead of being
        // predicated (a select between a load and a constant becomes a load through a selected POINTER, via scratch);
        // what they fetch is never staged / never stored
        const int kk = min(k, S - 1);
        const uint32_t col = (uint32_t)(l0 + 4 * qq < n_lines ? l0 + 4 * qq : l0);
        const int32_t* ap = plane_ptr(pl.avg[0], a_d1, a_d2, p);
        const int32_t* rp = plane_ptr(pl.res[0], r_d1, r_d2, p);
        // the line's end: next_avg of the last step of an even line is the last average itself (index clamped);
        // steps past the line fetch valid rows that are never used
        const int ia = min(c * S + 1 + kk, n_avg - 1), ir = min(c * S + kk, max(w - 1, 0));
#ifndef JXLH_SQRCT_NT
#define JXLH_SQRCT_NT false
#endif
        const int4 xa = gload_i4<JXLH_SQRCT_NT>(ap + (uint32_t)ia * avg_ep + col);
        const int4 xr = gload_i4<JXLH_SQRCT_NT>(rp + (uint32_t)ir * res_ep + col);
        va[4 * j] = xa.x; va[4 * j + 1] = xa.y; va[4 * j + 2] = xa.z; va[4 * j + 3] = xa.w;
        vr[4 * j] = xr.x; vr[4 * j + 1] = xr.y; vr[4 * j + 2] = xr.z; vr[4 * j + 3] = xr.w;
      }
      return;
    }
#pragma unroll
    for (int j = 0; j < NIN; j++) {
      const int f = m + j * NM, r = HORIZ ? f / S : f % 64, k = HORIZ ? f % S : f / 64;
      int p, q;
      const bool ok = row_of(r, p, q) && f < 64 * S && c * S + k < w;
      const int32_t* ap = plane_ptr(pl.avg[0], a_d1, a_d2, p);
      const int32_t* rp = plane_ptr(pl.res[0], r_d1, r_d2, p);
      const int ia = min(c * S + 1 + k, n_avg - 1), ir = min(c * S + k, max(w - 1, 0));
      va[j] = ok ? ap[(uint32_t)(l0 + q) * avg_lp + (uint32_t)ia * avg_ep] : 0;
      vr[j] = ok ? rp[(uint32_t)(l0 + q) * res_lp + (uint32_t)ir * res_ep] : 0;
    }
  };
  auto stage_chunk = [&](int c, const int32_t(&va)[NIN], const int32_t(&vr)[NIN]) {
    if constexpr (VEC) {
#pragma unroll
      for (int j = 0; j < NVIN; j++) {
        const int f = m + j * NML, k = f / (3 * QN), rem = f - k * (3 * QN), p = rem / QN, qq = rem % QN;
        if (f < S * 3 * QN) {
          const int idx = k * RP + p * NL + 4 * qq;
          *reinterpret_cast<int4*>(&s_avg[c & 1][idx]) = make_int4(va[4 * j], va[4 * j + 1], va[4 * j + 2], va[4 * j + 3]);
          *reinterpret_cast<int4*>(&s_res[c & 1][idx]) = make_int4(vr[4 * j], vr[4 * j + 1], vr[4 * j + 2], vr[4 * j + 3]);
        }
      }
      return;
    }
#pragma unroll
    for (int j = 0; j < NIN; j++) {
      const int f = m + j * NM, r = HORIZ ? f / S : f % 64, k = HORIZ ? f % S : f / 64;
      if (f < 64 * S) {
        s_avg[c & 1][in_idx(r, k)] = va[j];
        s_res[c & 1][in_idx(r, k)] = vr[j];
      }
    }
  };
  // drain `count` (<= 2 S) output samples per line of chunk c, through the RCT
  auto rct4 = [&](const int4& v0, const int4& v1, const int4& v2, int4& x, int4& y, int4& z) {
    switch (op) {
#define JXLH_RCT4(OP)                          \
  case OP:                                     \
    rct_op<OP>(v0.x, v1.x, v2.x, x.x, y.x, z.x); \
    rct_op<OP>(v0.y, v1.y, v2.y, x.y, y.y, z.y); \
    rct_op<OP>(v0.z, v1.z, v2.z, x.z, y.z, z.z); \
    rct_op<OP>(v0.w, v1.w, v2.w, x.w, y.w, z.w); \
    break;
      JXLH_RCT4(0) JXLH_RCT4(1) JXLH_RCT4(2) JXLH_RCT4(3) JXLH_RCT4(4) JXLH_RCT4(5)
      default:
      JXLH_RCT4(6)
#undef JXLH_RCT4
    }
  };
  auto store_chunk = [&](int c, int count) {
    const int32_t* so = s_out[c & 1];
    if constexpr (VEC) {
#pragma unroll
      for (int j = 0; j < NVOUT; j++) {
        const int f = m + j * NMS, k = f / QN, qq = f % QN;
        if (f < 2 * S * QN && l0 + 4 * qq < n_lines && k < count) {
          const int4 v0 = *reinterpret_cast<const int4*>(so + k * RP + 4 * qq);
          const int4 v1 = *reinterpret_cast<const int4*>(so + k * RP + NL + 4 * qq);
          const int4 v2 = *reinterpret_cast<const int4*>(so + k * RP + 2 * NL + 4 * qq);
          int4 x, y, z;
          rct4(v0, v1, v2, x, y, z);
          const uint32_t off = (uint32_t)(2 * c * S + k) * out_ep + (uint32_t)(l0 + 4 * qq);
          gstore_i4<JXLH_SQRCT_NT>(o0 + off, x);
          gstore_i4<JXLH_SQRCT_NT>(o1 + off, y);
          gstore_i4<JXLH_SQRCT_NT>(o2 + off, z);
        }
      }
      return;
    }
#pragma unroll
    for (int j = 0; j < NPIX; j++) {
      const int f = m + j * NM, q = HORIZ ? f / (2 * S) : f % NL, k = HORIZ ? f % (2 * S) : f / NL;
      if (f < NL * 2 * S && l0 + q < n_lines && k < count) {
        const int32_t v0 = so[out_idx(q, k)], v1 = so[out_idx(NL + q, k)], v2 = so[out_idx(2 * NL + q, k)];
        int32_t x, y, z;
        switch (op) {
          case 0: rct_op<0>(v0, v1, v2, x, y, z); break;
          case 1: rct_op<1>(v0, v1, v2, x, y, z); break;
          case 2: rct_op<2>(v0, v1, v2, x, y, z); break;
          case 3: rct_op<3>(v0, v1, v2, x, y, z); break;
          case 4: rct_op<4>(v0, v1, v2, x, y, z); break;
          case 5: rct_op<5>(v0, v1, v2, x, y, z); break;
          default: rct_op<6>(v0, v1, v2, x, y, z); break;
        }
        const uint32_t off = (uint32_t)(l0 + q) * out_lp + (uint32_t)(2 * c * S + k) * out_ep;
        o0[off] = x;
        o1[off] = y;
        o2[off] = z;
      }
    }
  };

  int cp, cq;
  const bool live = chain && row_of(tid, cp, cq);
  int32_t cur = 0, d = 0;
  if (live) cur = (plane_ptr(pl.avg[0], a_d1, a_d2, cp) + (size_t)(l0 + cq) * avg_lp)[0];
  auto count_of = [&](int c) { return min(2 * S, n_out - 2 * c * S); };
  int32_t pa[NIN], pr[NIN];
  if (loader && steps_of(0) > 0) {
    fetch_chunk(0, pa, pr);
    stage_chunk(0, pa, pr);
    if (steps_of(1) > 0) fetch_chunk(1, pa, pr);
  }
  lds_barrier();
  for (int c = 0; c < n_chunks; c++) {
    if (!chain) {
      if (loader && steps_of(c + 1) > 0) stage_chunk(c + 1, pa, pr);
      if (loader && steps_of(c + 2) > 0) fetch_chunk(c + 2, pa, pr);
      if (storer && c >= 1) store_chunk(c - 1, count_of(c - 1));
    } else {
      const int32_t* ia = s_avg[c & 1];
      const int32_t* ir = s_res[c & 1];
      int32_t* oa = s_out[c & 1];
      const int sc = steps_of(c);
      if (sc == S) {
        int32_t xa[S], xr[S];
        if constexpr (HORIZ) {
#pragma unroll
          for (int j = 0; j < S / 4; j++) {
            const int4 va = *reinterpret_cast<const int4*>(ia + tid * PI + 4 * j);
            const int4 vr = *reinterpret_cast<const int4*>(ir + tid * PI + 4 * j);
            xa[4 * j] = va.x; xa[4 * j + 1] = va.y; xa[4 * j + 2] = va.z; xa[4 * j + 3] = va.w;
            xr[4 * j] = vr.x; xr[4 * j + 1] = vr.y; xr[4 * j + 2] = vr.z; xr[4 * j + 3] = vr.w;
          }
        } else {
#pragma unroll
          for (int k = 0; k < S; k++) {
            xa[k] = ia[k * RP + tid];
            xr[k] = ir[k * RP + tid];
          }
        }
#pragma unroll
        for (int k = 0; k < S; k += 2) {
          int32_t a0, b0, a1, b1;
          unsqueeze_step(cur, xr[k], xa[k], d, a0, b0);
          unsqueeze_step(xa[k], xr[k + 1], xa[k + 1], d, a1, b1);
          cur = xa[k + 1];
          if constexpr (HORIZ) {
            *reinterpret_cast<int4*>(oa + tid * PO + 2 * k) = make_int4(a0, b0, a1, b1);
          } else {
            oa[(2 * k) * RP + tid] = a0;
            oa[(2 * k + 1) * RP + tid] = b0;
            oa[(2 * k + 2) * RP + tid] = a1;
            oa[(2 * k + 3) * RP + tid] = b1;
          }
        }
      } else if (live) {  // the line's last chunk: fewer steps, one by one; an odd line's copied sample behind them
        for (int k = 0; k < sc; k++) {
          const int32_t nxt = ia[in_idx(tid, k)], rs = ir[in_idx(tid, k)];
          int32_t va, vb;
          unsqueeze_step(cur, rs, nxt, d, va, vb);
          cur = nxt;
          oa[out_idx(tid, 2 * k)] = va;
          oa[out_idx(tid, 2 * k + 1)] = vb;
        }
        if (has_tail) oa[out_idx(tid, 2 * sc)] = cur;  // sample 2 w = avg[w] (squeeze.rs:434-437, :468-476)
      }
    }
    lds_barrier();
  }
  if (storer && n_chunks > 0) store_chunk(n_chunks - 1, count_of(n_chunks - 1));
}

// the step's planes as the kernels take them (squeeze_plan.h carries them as addresses)
static SqueezePlanes planes_of(const SqueezeStep& st) {
  SqueezePlanes pl{};
  for (int i = 0; i < st.n_planes && i < 3; i++) {
    pl.avg[i] = reinterpret_cast<const int32_t*>(st.avg[i]);
    pl.res[i] = reinterpret_cast<const int32_t*>(st.res[i]);
    pl.out[i] = reinterpret_cast<int32_t*>(st.out[i]);
  }
  return pl;
}
// One step over its n_planes (<= 3) planes, on the kernel and in the variant `how` names (kTiled, kOneWave)
void launch_unsqueeze(hipStream_t s, const SqueezeLaunch& how, const SqueezeStep& st) {
  if (st.out_w == 0 || st.out_h == 0 || st.n_planes <= 0) return;
  const SqueezePlanes pl = planes_of(st);
  const bool hz = st.horizontal;
  const int n_lines = (int)(hz ? st.out_h : st.out_w), n_out = (int)(hz ? st.out_w : st.out_h);
  const dim3 grid((n_lines + 63) / 64, st.n_planes);
  // element i of line l at p[l * lp + i * ep]
  const size_t one = 1, alp = hz ? st.avg_stride : one, aep = hz ? one : st.avg_stride;
  const size_t rlp = hz ? st.res_stride : one, rep = hz ? one : st.res_stride;
  const size_t olp = hz ? st.out_stride : one, oep = hz ? one : st.out_stride;
#define JXLH_SQ_LAUNCH(K, B, ...) hipLaunchKernelGGL(K, grid, dim3(B), 0, s, pl, alp, aep, rlp, rep, olp, oep, n_lines, n_out, ##__VA_ARGS__)
  if (how.kind == SqueezeLaunch::kTiled) {
    if (hz) JXLH_SQ_LAUNCH(k6_unsqueeze_tiled<true>, 256, how.vec);
    else JXLH_SQ_LAUNCH(k6_unsqueeze_tiled<false>, 256, how.vec);
  } else if (how.vec) {
    JXLH_SQ_LAUNCH(k6_unsqueeze<true>, 64);
  } else {
    JXLH_SQ_LAUNCH(k6_unsqueeze<false>, 64);
  }
#undef JXLH_SQ_LAUNCH
}

// ---- the regular runs of a partly arrived level (jxlh_unsqueeze_chain_preview_tiles, squeeze_preview_plan.h).  A run is a
// stretch of pairs [pair0, pair0 + n_pairs) of the lines [line0, line0 + n_lines): regular cells side by side along the
// squeezed axis.  One launch over the listed runs, groups_per_run workgroups each (a ragged last cell row sends the
// surplus home), lanes are lines in groups of 64, the plane in blockIdx.y.  The recurrence starts from the output sample
// in front of the run -- the smooth launch ahead in the stream wrote it -- or from avg[0] at the channel's start, and ends
// on the average across the run's edge (avg[x + 1]; at the channel's end avg[x] itself).  Residuals outside the run are
// never read.  Loads of the next U steps are in flight while the current U run, as in k6_unsqueeze.
namespace {
static_assert(JXLH_SQC_LINES == 64, "squeeze_preview_plan.h counts the workgroups of a run");
template <bool HORIZ>
__global__ __launch_bounds__(64) void k6_unsqueeze_runs(const SqueezePlanes pl, size_t avg_stride, size_t res_stride, size_t out_stride,
                                                        int n_out, const SqTileRun* __restrict__ runs, uint32_t groups_per_run) {
  const uint32_t run = blockIdx.x / groups_per_run, grp = blockIdx.x - run * groups_per_run;
  const SqTileRun rn = runs[run];
  const int l = (int)grp * 64 + (int)threadIdx.x;
  if (l >= (rn.n_lines_tail >> 1)) return;
  const size_t line = (size_t)(rn.line0 + l);
  const size_t alp = HORIZ ? avg_stride : 1, aep = HORIZ ? 1 : avg_stride;
  const size_t rlp = HORIZ ? res_stride : 1, rep = HORIZ ? 1 : res_stride;
  const size_t olp = HORIZ ? out_stride : 1, oep = HORIZ ? 1 : out_stride;
  const int32_t* __restrict__ a = pl.avg[blockIdx.y] + line * alp;
  const int32_t* __restrict__ r = pl.res[blockIdx.y] + line * rlp;
  int32_t* o = pl.out[blockIdx.y] + line * olp;
  const int last_avg = n_out - n_out / 2 - 1;
  int i = rn.pair0;
  const int end = rn.pair0 + rn.n_pairs;
  if (rn.n_pairs > 0) {
    int32_t cur = a[(size_t)i * aep];
    const int32_t prev = i == 0 ? cur : o[(size_t)(2 * i - 1) * oep];
    int32_t d = wsub(prev, cur);
    constexpr int U = 8;
    int32_t na[U], rr[U], nb[U], rb[U];
    auto load_block = [&](int i0, int32_t(&xa)[U], int32_t(&xr)[U]) {
#pragma unroll
      for (int k = 0; k < U; k++) {
        xa[k] = a[(size_t)min(i0 + k + 1, last_avg) * aep];
        xr[k] = r[(size_t)(i0 + k) * rep];
      }
    };
    auto run_block = [&](int i0, const int32_t(&xa)[U], const int32_t(&xr)[U]) {
#pragma unroll
      for (int k = 0; k < U; k++) {
        int32_t va, vb;
        unsqueeze_step(cur, xr[k], xa[k], d, va, vb);
        o[(size_t)(2 * (i0 + k)) * oep] = va;
        o[(size_t)(2 * (i0 + k) + 1) * oep] = vb;
        cur = xa[k];
      }
    };
    const int n_blocks = rn.n_pairs / U;
    if (n_blocks > 0) {
      load_block(i, na, rr);
      int blk = 0;
      for (; blk + 2 <= n_blocks; blk += 2) {
        load_block(i + (blk + 1) * U, nb, rb);
        run_block(i + blk * U, na, rr);
        if (blk + 2 < n_blocks) load_block(i + (blk + 2) * U, na, rr);
        run_block(i + (blk + 1) * U, nb, rb);
      }
      if (blk < n_blocks) run_block(i + blk * U, na, rr);
      i += n_blocks * U;
    }
    for (; i < end; i++) {
      const int32_t nxt = a[(size_t)min(i + 1, last_avg) * aep];
      int32_t va, vb;
      unsqueeze_step(cur, r[(size_t)i * rep], nxt, d, va, vb);
      o[(size_t)(2 * i) * oep] = va;
      o[(size_t)(2 * i + 1) * oep] = vb;
      cur = nxt;
    }
  }
  if (rn.n_lines_tail & 1) o[(size_t)(2 * end) * oep] = a[(size_t)end * aep];  // odd size: the trailing average is copied
}
}  // namespace
void launch_unsqueeze_runs(hipStream_t s, const SqueezeStep& st, const SqTileRun* runs, uint32_t n_runs, uint32_t groups_per_run) {
  if (n_runs == 0 || st.n_planes <= 0) return;
  const SqueezePlanes pl = planes_of(st);
  const dim3 grid(n_runs * groups_per_run, st.n_planes);
  if (st.horizontal)
    hipLaunchKernelGGL(k6_unsqueeze_runs<true>, grid, dim3(64), 0, s, pl, st.avg_stride, st.res_stride, st.out_stride, (int)st.out_w, runs,
                       groups_per_run);
  else
    hipLaunchKernelGGL(k6_unsqueeze_runs<false>, grid, dim3(64), 0, s, pl, st.avg_stride, st.res_stride, st.out_stride, (int)st.out_h, runs,
                       groups_per_run);
}

// ---- dataflow launch of consecutive tiled steps (see k6_unsqueeze_flow)
static_assert(sizeof(FlowArgs) <= 4096, "kFlowMaxLevels levels (squeeze_plan.h) travel as kernel arguments");
void launch_unsqueeze_flow(hipStream_t s, int n_steps, const SqueezeStep* steps, const uint8_t* vec, int* scratch, int* error,
                           float deadline_s, unsigned long long* prof) {
  const int n_planes = steps[0].n_planes;
  FlowArgs A{};
  A.n_levels = n_steps;
  A.n_planes = n_planes;
  A.ticket = scratch;
  A.progress = scratch + kFlowWordStride;
  A.error = error;
  A.deadline_ticks = (unsigned long long)(deadline_s * 1.0e8);
  int wg = 0, flag = 0;
  for (int i = 0; i < n_steps; i++) {
    const SqueezeStep& st = steps[i];
    FlowLevel& L = A.lv[i];
    const SqueezePlanes pl = planes_of(st);
    for (int p = 0; p < 3; p++) {  // (a level names three planes whatever n_planes is)
      const int q = p < n_planes ? p : 0;
      L.avg[p] = pl.avg[q];
      L.res[p] = pl.res[q];
      L.out[p] = pl.out[q];
    }
    const bool hz = st.horizontal;
    L.avg_lp = hz ? (uint32_t)st.avg_stride : 1u;
    L.avg_ep = hz ? 1u : (uint32_t)st.avg_stride;
    L.res_lp = hz ? (uint32_t)st.res_stride : 1u;
    L.res_ep = hz ? 1u : (uint32_t)st.res_stride;
    L.out_lp = hz ? (uint32_t)st.out_stride : 1u;
    L.out_ep = hz ? 1u : (uint32_t)st.out_stride;
    L.n_lines = (int)(hz ? st.out_h : st.out_w);
    L.n_out = (int)(hz ? st.out_w : st.out_h);
    L.horiz = hz;
    L.groups = (L.n_lines + 63) / 64;
    L.first_wg = wg;
    L.flag0 = flag;
    L.dep_same_axis = i > 0 && steps[i - 1].horizontal == hz;
    L.vec = vec[i];
    wg += L.groups * n_planes;
    flag += L.groups * n_planes;
  }
  (void)hipMemsetAsync(scratch, 0, sizeof(int) * (size_t)(1 + flag) * kFlowWordStride, s);
  A.prof = prof;
  if (prof) {
    (void)hipMemsetAsync(prof, 0xff, sizeof(unsigned long long) * kFlowMaxLevels, s);
    (void)hipMemsetAsync(prof + kFlowMaxLevels, 0, sizeof(unsigned long long) * 10 * kFlowMaxLevels, s);
  }
  hipLaunchKernelGGL(k6_unsqueeze_flow, dim3(wg), dim3(256), 0, s, A);
}

// Unsqueeze of three channels + inverse RCT on them, one pass, in the variant `how` names (kFusedRct: planes below 2^31
// samples, 32-bit offsets)
void launch_unsqueeze_rct(hipStream_t s, const SqueezeLaunch& how, const SqueezeStep& st, int op, int perm) {
  if (st.out_w == 0 || st.out_h == 0) return;
  const SqueezePlanes pl = planes_of(st);
  const uint32_t as = (uint32_t)st.avg_stride, rs = (uint32_t)st.res_stride, os = (uint32_t)st.out_stride, w = st.out_w, h = st.out_h;
  if (st.horizontal) {
    hipLaunchKernelGGL((k6_unsqueeze_rct<true, false>), dim3((h + 20) / 21), dim3(256), 0, s, pl, as, 1u, rs, 1u, os, 1u, (int)h,
                       (int)w, op, perm);
    return;
  }
#define JXLH_SQRCT_V(VEC, NCW, COLS, B) \
  hipLaunchKernelGGL((k6_unsqueeze_rct<false, VEC, NCW>), dim3((w + COLS - 1) / COLS), dim3(B), 0, s, pl, 1u, as, 1u, rs, 1u, os, (int)w, (int)h, op, perm)
  // wide planes: 32 columns per plane and workgroup (whole 128-byte lines), one workgroup per CU is enough
  if (how.ncw == 2) JXLH_SQRCT_V(true, 2, 32, 448);
  else if (how.vec) JXLH_SQRCT_V(true, 1, 16, 256);
  else JXLH_SQRCT_V(false, 1, 16, 256);
#undef JXLH_SQRCT_V
}

// The first levels of a squeeze chain are tiny (8x8 -> 16x8 -> 16x16 -> ... ) and each one, as its own launch, costs
// ~10 us however few steps it has: the eight levels up to 128 x 128 of the default chain took 83 us for 240 steps.
// Here one workgroup per plane walks ALL of them: the running average plane lives in LDS (two buffers swapped per
// level), a level's residual plane is staged through LDS with coalesced loads, lanes = lines, and only the last level
// is written out.
struct SqueezeLevels {
  int n_levels;
  int base_w, base_h;
  uint32_t base_stride, out_stride;
  const int32_t* base[3];
  int32_t* out[3];
  struct {
    int horizontal, out_w, out_h;
    uint32_t res_stride;
    const int32_t* res[3];
  } lv[JXLH_SQL_LEVELS];
};
__global__ __launch_bounds__(256) void k6_unsqueeze_levels(const SqueezeLevels L) {
  // Two plane buffers, swapped per level.  A level's output is twice its input, so only the buffer the LAST level
  // writes has to hold a full 128 x 128 plane; the other one (and the residual tile) hold half planes.  Row pitch =
  // width | 1 (odd: lane = row and lane = column are both conflict-free).
  constexpr int kFull = JXLH_SQL_MAX * (JXLH_SQL_MAX + 1), kHalf = JXLH_SQL_MAX * (JXLH_SQL_MAX / 2 + 1);
  static_assert(JXLH_SQL_MAX <= 256 && JXLH_SQL_MAX * JXLH_SQL_MAX / 256 <= 64 && (kFull + 2 * kHalf) * 4 <= 160 * 1024,
                "squeeze_plan.h: a lane per line of 256 threads, <= kResPasses residual passes, the three tiles in LDS");
  __shared__ int32_t s_big[kFull], s_half[kHalf], s_r[kHalf];
  const int tid = threadIdx.x, pl = blockIdx.x;
  // level i reads buf[(i + off) & 1] and writes the other one; the last level must write s_big (index 0)
  const int off = L.n_levels & 1;
  auto buf = [&](int k) { return (k & 1) ? s_half : s_big; };
  int cw = L.base_w, ch = L.base_h;
  // plane <-> thread mapping without divisions: tx = tid % TW, TW = the power of two >= the plane's width, 256 / TW
  // rows per pass (uniform per level); at most 64 passes for a 128-row plane
  auto tile_log2 = [](int width) { return width <= 1 ? 0 : 32 - __builtin_clz((unsigned)(width - 1)); };
  {
    int32_t* b0 = buf(off);
    const int pc = cw | 1, lg = tile_log2(cw), tx = tid & ((1 << lg) - 1), ty = tid >> lg, rpp = 256 >> lg;
    for (int y = ty; y < ch; y += rpp)
      if (tx < cw) b0[y * pc + tx] = L.base[pl][(size_t)y * L.base_stride + tx];
  }
  // a level's residuals are fetched into registers (coalesced, <= 33 per thread) while the PREVIOUS level's recurrence
  // runs, and dropped into the LDS tile at the level's start: the global round trip is off the serial path
  constexpr int kResPasses = 64;
  int32_t rq[kResPasses];
  auto fetch_res = [&](int lv) {
    const int horizontal = L.lv[lv].horizontal, ow = L.lv[lv].out_w, oh = L.lv[lv].out_h;
    const int rw = horizontal ? ow / 2 : ow, rh = horizontal ? oh : oh / 2;
    if (rw == 0 || rh == 0) return;  // a one-sample axis has no residuals (and no plane to read)
    const int32_t* __restrict__ res = L.lv[lv].res[pl];
    const uint32_t rstride = L.lv[lv].res_stride;
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
  for (int lv = 0; lv < L.n_levels; lv++) {
    const int horizontal = L.lv[lv].horizontal, ow = L.lv[lv].out_w, oh = L.lv[lv].out_h;
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
    if (lv + 1 < L.n_levels) fetch_res(lv + 1);
    const int32_t* cur_buf = buf(lv + off);
    int32_t* nxt_buf = buf(lv + off + 1);
    const int n_lines = horizontal ? oh : ow, n_out = horizontal ? ow : oh;
    if (tid < n_lines) {
      // element i of line `tid`: horizontal = row tid, vertical = column tid
      const int32_t* a = cur_buf + (horizontal ? tid * pc : tid);
      const int32_t* r = s_r + (horizontal ? tid * pr : tid);
      int32_t* o = nxt_buf + (horizontal ? tid * po : tid);
      const int aep = horizontal ? 1 : pc, rep = horizontal ? 1 : pr, oep = horizontal ? 1 : po;
      const int w = n_out / 2;
      if (w == 0) {
        o[0] = a[0];
      } else {
        const bool has_tail = n_out & 1;
        const int n_main = has_tail ? w : w - 1;
        int32_t c0 = a[0], d = 0;
        int i = 0;
        for (; i + 4 <= n_main; i += 4) {  // operands of four steps in one LDS round trip
          int32_t nx[4], rr[4], va[4], vb[4];
#pragma unroll
          for (int k = 0; k < 4; k++) {
            nx[k] = a[(i + k + 1) * aep];
            rr[k] = r[(i + k) * rep];
          }
#pragma unroll
          for (int k = 0; k < 4; k++) {
            unsqueeze_step(c0, rr[k], nx[k], d, va[k], vb[k]);
            c0 = nx[k];
          }
#pragma unroll
          for (int k = 0; k < 4; k++) {
            o[(2 * (i + k)) * oep] = va[k];
            o[(2 * (i + k) + 1) * oep] = vb[k];
          }
        }
        for (; i < n_main; i++) {
          const int32_t nx = a[(i + 1) * aep];
          int32_t va, vb;
          unsqueeze_step(c0, r[i * rep], nx, d, va, vb);
          o[(2 * i) * oep] = va;
          o[(2 * i + 1) * oep] = vb;
          c0 = nx;
        }
        if (!has_tail) {
          int32_t va, vb;
          unsqueeze_step(c0, r[(w - 1) * rep], c0, d, va, vb);
          o[(2 * w - 2) * oep] = va;
          o[(2 * w - 1) * oep] = vb;
        } else {
          o[(2 * w) * oep] = c0;
        }
      }
    }
    __syncthreads();
    cw = ow;
    ch = oh;
  }
  {
    const int32_t* fin = buf(L.n_levels + off);  // = s_big
    const int pc = cw | 1, lg = tile_log2(cw), tx = tid & ((1 << lg) - 1), ty = tid >> lg, rpp = 256 >> lg;
    for (int y = ty; y < ch; y += rpp)
      if (tx < cw) L.out[pl][(size_t)y * L.out_stride + tx] = fin[y * pc + tx];
  }
}

// The first n_levels levels of a chain that squeeze_levels_fit (squeeze_plan.h) accepts, in one launch.
void launch_unsqueeze_levels(hipStream_t s, int n_planes, int n_levels, const jxlh_squeeze_level* levels,
                             const int32_t* const base[], size_t base_stride, uint32_t base_w, uint32_t base_h,
                             int32_t* const out[], size_t out_stride) {
  SqueezeLevels L{};
  L.n_levels = n_levels;
  L.base_w = (int)base_w;
  L.base_h = (int)base_h;
  L.base_stride = (uint32_t)base_stride;
  L.out_stride = (uint32_t)out_stride;
  for (int p = 0; p < n_planes; p++) {
    L.base[p] = base[p];
    L.out[p] = out[p];
  }
  for (int i = 0; i < n_levels; i++) {
    L.lv[i].horizontal = levels[i].horizontal ? 1 : 0;
    L.lv[i].out_w = (int)levels[i].out_w;
    L.lv[i].out_h = (int)levels[i].out_h;
    L.lv[i].res_stride = (uint32_t)levels[i].res_stride;
    for (int p = 0; p < n_planes; p++) L.lv[i].res[p] = levels[i].res[p] ? levels[i].res[p] : base[0];
  }
  hipLaunchKernelGGL(k6_unsqueeze_levels, dim3(n_planes), dim3(256), 0, s, L);
}

}  // namespace jxlh
