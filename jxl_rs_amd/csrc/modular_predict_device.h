// Per-pixel pieces of the predicted palettes (do_palette_step_general, palette.rs:165-262) that the whole-plane
// wavefront kernels (k_modular.hip: k5_palette_delta, k5_palette_wp) and the group-local one
// (k_modular_local_palette.hip) share: Predictor::predict_one, the neighbour rules of PredictionData::get_rows, and one
// pixel of the self-correcting (weighted) predictor with its error update.
#pragma once
#include "jxlh_internal.h"

namespace jxlh {
namespace {

template <int predictor>
__device__ __forceinline__ int64_t predict_one(int64_t left, int64_t top, int64_t toptop, int64_t topleft,
                                               int64_t topright, int64_t leftleft, int64_t toprightright) {
  switch (predictor) {  // Predictor::predict_one, modular/predict.rs:152-198 (i64, `/` truncates)
    case 1: return left;
    case 2: return top;
    case 3: return (top + left) / 2;
    case 4: {
      const int64_t p = left + top - topleft;
      const int64_t dl = p - left < 0 ? left - p : p - left, dt = p - top < 0 ? top - p : p - top;
      return dl < dt ? left : top;
    }
    case 5: {
      const int64_t mn = left < top ? left : top, mx = left < top ? top : left;
      const int64_t grad = left + top - topleft;
      const int64_t gmax = topleft < mn ? mx : grad;
      return topleft > mx ? mn : gmax;
    }
    case 7: return topright;
    case 8: return topleft;
    case 9: return leftleft;
    case 10: return (left + topleft) / 2;
    case 11: return (top + topleft) / 2;
    case 12: return (top + topright) / 2;
    case 13: return (6 * top - 2 * toptop + 7 * left + leftleft + toprightright + 3 * topright + 8) / 16;
    default: return 0;
  }
}

// the same with the predictor in a (wavefront-uniform) register: one scalar branch per pixel
__device__ __forceinline__ int64_t predict_uniform(int predictor, int64_t left, int64_t top, int64_t toptop,
                                                   int64_t topleft, int64_t topright, int64_t leftleft,
                                                   int64_t toprightright) {
#define JXLH_PREDICT(P) \
  case P: return predict_one<P>(left, top, toptop, topleft, topright, leftleft, toprightright)
  switch (predictor) {
    JXLH_PREDICT(1); JXLH_PREDICT(2); JXLH_PREDICT(3); JXLH_PREDICT(4); JXLH_PREDICT(5); JXLH_PREDICT(7);
    JXLH_PREDICT(8); JXLH_PREDICT(9); JXLH_PREDICT(10); JXLH_PREDICT(11); JXLH_PREDICT(12); JXLH_PREDICT(13);
    default: return 0;
  }
#undef JXLH_PREDICT
}

__constant__ uint32_t kWpDivLookup[64] = {  // (1 << 24) / (i + 1), predict.rs:206-213
    16777216, 8388608, 5592405, 4194304, 3355443, 2796202, 2396745, 2097152, 1864135, 1677721, 1525201, 1398101,
    1290555,  1198372, 1118481, 1048576, 986895,  932067,  883011,  838860,  798915,  762600,  729444,  699050,
    671088,   645277,  621378,  599186,  578524,  559240,  541200,  524288,  508400,  493447,  479349,  466033,
    453438,   441505,  430185,  419430,  409200,  399457,  390167,  381300,  372827,  364722,  356962,  349525,
    342392,   335544,  328965,  322638,  316551,  310689,  305040,  299593,  294337,  289262,  284359,  279620,
    275036,   270600,  266305,  262144};

// What one pixel of the weighted predictor reads.  Values that do not exist (first rows / columns) may hold anything:
// the selects below discard them.
struct WpIn {
  int x, w;
  bool has_top, has_toptop;              // y > 0, y > 1
  int32_t left_v;                        // out(x - 1, y)
  int32_t t_m1, t_0, t_p1, tt_0;         // out(x - 1 .. x + 1, y - 1), out(x, y - 2)
  int32_t ta_m1, ta_0, ta_p1, te1;       // TE(x - 1 .. x + 1, y - 1), TE(x - 1, y)
  uint32_t ea_m1[4], ea_0[4], ea_p1[4];  // E(x - 1 .. x + 1, y - 1)
  uint32_t e1[4], e2[4];                 // E(x - 1, y), E(x - 2, y)
};
struct WpOut {
  int32_t val, te;
  uint32_t e[4];
};

// WeightedPredictorState::predict_and_property + update_errors (modular/predict.rs:312-517) for one pixel, the delta
// entry added to the prediction where idx < num_deltas.  Every row keeps its own E: err_n = E(x, y-1) + E(x-1, y),
// err_nw = E(x-1, y-1) + E(x-2, y), err_ne = E(x+1, y-1), with the reference's edge rules (pos_nw = max(x-1, 0),
// pos_ne = min(x+1, w-1) index the SAME summed slots).  s_div: kWpDivLookup, in LDS.
__device__ __forceinline__ WpOut wp_pixel(const WpParams& P, const uint32_t* s_div, const WpIn& in, int32_t idx,
                                          int num_deltas, int32_t entry) {
  const int x = in.x, w = in.w;
  const bool has_top = in.has_top;
  // PredictionData::get_rows, modular/predict.rs:96-128
  const int32_t left = x > 0 ? in.left_v : (has_top ? in.t_0 : 0);
  const int32_t top = has_top ? in.t_0 : left;
  const int32_t topleft = (x > 0 && has_top) ? in.t_m1 : left;
  const int32_t topright = (x + 1 < w && has_top) ? in.t_p1 : top;
  const int32_t toptop = in.has_toptop ? in.tt_0 : top;
  const bool at_right = !(x + 1 < w), at_left = !(x > 0);  // pos_ne == x, pos_nw == x
  // weights from the error sums (:340-377)
  uint32_t wk[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const uint32_t en = (has_top ? in.ea_0[q] : 0u) + (x > 0 ? in.e1[q] : 0u);
    const uint32_t ene = at_right ? en : (has_top ? in.ea_p1[q] : 0u);
    const uint32_t enw = at_left ? en : (has_top ? in.ea_m1[q] : 0u) + (x > 1 ? in.e2[q] : 0u);
    const uint32_t err = en + ene + enw;
    int shift = 63 - __clzll((unsigned long long)err + 1ull) - 5;
    shift = shift < 0 ? 0 : shift;
    wk[q] = 4u + ((P.w[q] * s_div[err >> shift]) >> shift);
  }
  const int64_t te_w = x > 0 ? (int64_t)in.te1 : 0;
  const int64_t te_n = has_top ? (int64_t)in.ta_0 : 0;
  const int64_t te_nw = has_top ? (int64_t)(at_left ? in.ta_0 : in.ta_m1) : 0;
  const int64_t te_ne = has_top ? (int64_t)(at_right ? in.ta_0 : in.ta_p1) : 0;
  const int64_t sum_wn = te_n + te_w;
  const int64_t n = (int64_t)top << 3, wv = (int64_t)left << 3, ne = (int64_t)topright << 3;
  const int64_t nw = (int64_t)topleft << 3, nn = (int64_t)toptop << 3;
  int64_t pk[4];
  pk[0] = wv + ne - n;
  pk[1] = n - (((sum_wn + te_ne) * (int64_t)P.p1c) >> 5);
  pk[2] = wv - (((sum_wn + te_nw) * (int64_t)P.p2c) >> 5);
  pk[3] = n - ((te_nw * (int64_t)P.p3c[0] + te_n * (int64_t)P.p3c[1] + te_ne * (int64_t)P.p3c[2] +
                (nn - n) * (int64_t)P.p3c[3] + (nw - wv) * (int64_t)P.p3c[4]) >> 5);
  const int log_weight = 63 - __clzll((unsigned long long)wk[0] + wk[1] + wk[2] + wk[3]);
  const int64_t w0s = (int64_t)(wk[0] >> (log_weight - 4)), w1s = (int64_t)(wk[1] >> (log_weight - 4));
  const int64_t w2s = (int64_t)(wk[2] >> (log_weight - 4)), w3s = (int64_t)(wk[3] >> (log_weight - 4));
  const int64_t weight_sum = w0s + w1s + w2s + w3s;
  const int64_t sum = (weight_sum >> 1) - 1 + w0s * pk[0] + w1s * pk[1] + w2s * pk[2] + w3s * pk[3];
  int64_t pred = (sum * (int64_t)s_div[(weight_sum - 1) & 63]) >> 24;
  if (((te_n ^ te_w) | (te_n ^ te_nw)) <= 0) {
    const int64_t mx = max(wv, max(ne, n)), mn = min(wv, min(ne, n));
    pred = max(mn, min(mx, pred));
  }
  const int64_t wp_pred = (pred + 3) >> 3;
  WpOut o;
  o.val = idx < num_deltas ? (int32_t)(uint32_t)(uint64_t)(wp_pred + (int64_t)entry) : entry;
  // update_errors (:472-517)
  const int64_t v = (int64_t)o.val << 3;
  o.te = (int32_t)(pred - v);
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int64_t dd = pk[q] - v;
    o.e[q] = (uint32_t)(((dd < 0 ? -dd : dd) + 3) >> 3);
  }
  return o;
}

}  // namespace
}  // namespace jxlh
