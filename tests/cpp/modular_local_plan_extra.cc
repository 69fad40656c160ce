// The destination table of the group-local transforms with extra channels (jxl_hip_local_extra.h), as
// jxl_rs_amd/csrc/modular_local_plan.h decides it: plain C++, no device, no library -- the program a sanitizer build
// runs (-fsanitize=address,undefined).  Checks
//   * the table of every layout: 3+1, 1+1, 1+3, 0+1..4, and 3+0, whose plan must be the frame form's byte for byte;
//   * every refusal with its status, text and first_bad, and that a refused plan holds no launch;
//   * that alignment is a per-plane fact that decides `vec` and nothing else;
//   * 100 000 random batches, walked on the host: every store of every launch lands inside its group's rect on the
//     plane the table names, at that plane's stride, and every sample of every rect is written.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../jxl_rs_amd/csrc/modular_local_plan.h"

using namespace jxlh;

static int fails = 0;
#define EXPECT(c)                                        \
  do {                                                   \
    if (!(c)) {                                          \
      fprintf(stderr, "line %d: %s\n", __LINE__, #c);    \
      fails++;                                           \
    }                                                    \
  } while (0)

static const jxlh_wp_header kWp = {16, 10, 7, 7, 7, 0, 0, 13, 12, 12, 12};
static const jxlh_status INV = JXLH_ERR_INVALID_ARGUMENT, BAD = JXLH_ERR_BAD_STATE, UNS = JXLH_ERR_UNSUPPORTED;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) {  // xorshift64*: [0, n)
  rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
  return (uint32_t)(((rng_state * 0x2545f4914f6cdd1dull) >> 33) % n);
}

static jxlh_local_dest dest_of(uint32_t n_colour, std::vector<uint32_t> ec, uint32_t bit_depth = 0) {
  jxlh_local_dest d;
  memset(&d, 0, sizeof d);
  d.n_colour = n_colour, d.n_ec = (uint32_t)ec.size(), d.bit_depth = bit_depth;
  for (size_t k = 0; k < ec.size() && k < 4; k++) d.ec[k] = ec[k];
  return d;
}
// a Modular frame of w x h (stride: its planes') whose extra channels 0..n_set-1 are set at the frame's size
static LocalDestState modular_state(uint32_t w, uint32_t h, uint32_t stride, uint32_t n_set) {
  LocalDestState s;
  s.in_frame = s.modular = true;
  s.w = w, s.h = h, s.plane_stride = stride;
  for (uint32_t i = 0; i < n_set; i++) s.ec[i].set = true, s.ec[i].w = w, s.ec[i].h = h;
  return s;
}

// one call in the squeeze form: groups, the call-wide tables, an arena handed out by a bump pointer
struct Call {
  std::vector<jxlh_local_squeeze_group> groups;
  std::vector<jxlh_local_coded_channel> coded;
  std::vector<jxlh_squeeze_params> params;
  std::vector<jxlh_wp_header> wp;
  uint64_t arena = 64;
  uint64_t take(uint64_t n) {
    const uint64_t at = arena;
    arena += (n + 3) / 4 * 4;
    return at;
  }
  LocalBatchIn in() const {
    LocalBatchIn v;
    v.form = LocalBatchIn::kSqueeze;
    v.sgroups = groups.data(), v.n = groups.size();
    v.coded = coded.data(), v.n_coded = coded.size(), v.params = params.data(), v.n_params = params.size();
    v.wp = wp.data(), v.arena_samples = arena;
    return v;
  }
};
static jxlh_local_step rct(uint32_t begin, uint32_t type) {
  jxlh_local_step s;
  memset(&s, 0, sizeof s);
  s.kind = JXLH_LOCAL_RCT, s.begin_c = begin, s.rct_type = type;
  return s;
}
static jxlh_local_step pal(Call& c, uint32_t begin, uint32_t num_c, uint32_t colors, uint32_t deltas, uint32_t predictor) {
  jxlh_local_step s;
  memset(&s, 0, sizeof s);
  s.kind = JXLH_LOCAL_PALETTE, s.begin_c = begin, s.num_c = num_c, s.num_colors = colors, s.num_deltas = deltas;
  s.predictor = predictor, s.palette_offset = c.take((uint64_t)num_c * (colors + deltas));
  return s;
}
// squeeze: 0 none, 1 the default list.  The coded channels are sized by the bookkeeping of meta_apply.rs.
static void add_group(Call& c, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t n_channels,
                      const std::vector<jxlh_local_step>& steps, int squeeze, uint32_t stride_pad = 0) {
  jxlh_local_squeeze_group g;
  memset(&g, 0, sizeof g);
  g.x0 = x0, g.y0 = y0, g.w = w, g.h = h, g.n_channels = n_channels, g.n_steps = (uint32_t)steps.size();
  for (size_t i = 0; i < steps.size(); i++) g.steps[i] = steps[i];
  jxlh_local_group gg;
  memset(&gg, 0, sizeof gg);
  gg.n_channels = n_channels, gg.n_steps = g.n_steps;
  for (size_t i = 0; i < steps.size(); i++) gg.steps[i] = steps[i];
  jxlh_local_general_program gp;
  const jxlh_status st = local_lower_core(gg, 8, ~0ull, true, &kWp, nullptr, &gp, nullptr, false);
  EXPECT(st == JXLH_OK);
  const uint32_t n_image = st == JXLH_OK ? gp.n_coded : 0;
  uint32_t n_meta = 0;
  for (const jxlh_local_step& s : steps) n_meta += s.kind == JXLH_LOCAL_PALETTE;
  struct E { uint32_t w, h; };
  std::vector<E> list(n_meta + n_image, E{w, h});
  if (squeeze) {
    g.has_squeeze = 1, g.squeeze_pos = g.n_steps;
    g.params_first = (uint32_t)c.params.size(), g.n_params = 0;
    jxlh_squeeze_params d[kLsMaxDefaultParams];
    uint32_t cw[4], ch[4];
    for (uint32_t k = 0; k < n_image; k++) cw[k] = w, ch[k] = h;
    const uint32_t np = default_squeeze_list(cw, ch, n_image, n_meta, d, kLsMaxDefaultParams);
    for (uint32_t i = 0; i < np; i++) {
      const jxlh_squeeze_params& p = d[i];
      const size_t end = p.begin_c + p.num_c, at0 = p.in_place ? end : list.size();
      for (uint32_t ic = 0; ic < p.num_c; ic++) {
        E& e = list[p.begin_c + ic];
        E r = e;
        if (p.horizontal) e.w = (e.w + 1) / 2, r.w -= e.w;
        else e.h = (e.h + 1) / 2, r.h -= e.h;
        list.insert(list.begin() + at0 + ic, r);
      }
    }
  }
  g.coded_first = (uint32_t)c.coded.size(), g.n_coded = (uint32_t)list.size() - n_meta;
  for (uint32_t k = 0; k < g.n_coded; k++) {
    const E& e = list[n_meta + k];
    const uint32_t stride = e.w + stride_pad;
    c.coded.push_back(jxlh_local_coded_channel{c.take((uint64_t)stride * e.h), stride, e.w, e.h});
  }
  c.groups.push_back(g);
  c.wp.push_back(kWp);
}

static LocalPlan plan_with(const Call& c, const LocalDestTable& t, bool arena_aligned = true, bool p0 = true, bool p1 = true,
                           bool p2 = true, bool p3 = true, bool fan = true) {
  LocalBatchIn in = c.in();
  in.dest = &t, in.bit_depth = t.bit_depth;
  in.plane_aligned[0] = p0, in.plane_aligned[1] = p1, in.plane_aligned[2] = p2, in.plane_aligned[3] = p3;
  in.fan_aligned = fan;
  return plan_local_batch(in, arena_aligned);
}
static std::vector<uint8_t> bytes_of(const LocalPlan& p) {
  std::vector<uint8_t> b(p.layout.total + 1);
  p.serialize(b.data());
  b.pop_back();
  return b;
}
static bool same_steps(const LocalPlan& a, const LocalPlan& b) {
  if (a.steps.size() != b.steps.size()) return false;
  for (size_t i = 0; i < a.steps.size(); i++) {
    const LocalStep &x = a.steps[i], &y = b.steps[i];
    if (x.kernel != y.kernel || x.n_items != y.n_items || x.step != y.step || x.weighted != y.weighted ||
        x.lds_palette != y.lds_palette || x.desc.off != y.desc.off || x.items.off != y.items.off)
      return false;
  }
  return true;
}

// ---------------------------------------------------------------- the tables
static void test_tables() {
  const LocalDestState s = modular_state(203, 137, 256, 4);
  {  // 3 + 1: RGBA
    const LocalDestTable t = plan_local_dest(dest_of(3, {2}), 8, s);
    EXPECT(t.status == JXLH_OK && t.n_slots == 4 && !t.fan && t.mixed() && t.w == 203 && t.h == 137 && t.bit_depth == 8);
    for (uint32_t c = 0; c < 3; c++) EXPECT(t.slot[c].plane == kLocalPlaneColour + c && t.slot[c].stride == 256);
    EXPECT(t.slot[3].plane == kLocalPlaneExtra + 2 && t.slot[3].stride == 203);
  }
  {  // 1 + 1: grey with alpha; the fan keeps colour planes 1 and 2, no slot names them
    const LocalDestTable t = plan_local_dest(dest_of(1, {0}), 16, s);
    EXPECT(t.status == JXLH_OK && t.n_slots == 2 && t.fan && t.mixed() && t.bit_depth == 16);
    EXPECT(t.slot[0].plane == kLocalPlaneColour && t.slot[0].stride == 256);
    EXPECT(t.slot[1].plane == kLocalPlaneExtra + 0 && t.slot[1].stride == 203);
  }
  {  // 1 + 3
    const LocalDestTable t = plan_local_dest(dest_of(1, {3, 0, 1}), 8, s);
    EXPECT(t.status == JXLH_OK && t.n_slots == 4 && t.fan);
    EXPECT(t.slot[0].plane == kLocalPlaneColour && t.slot[1].plane == kLocalPlaneExtra + 3 &&
           t.slot[2].plane == kLocalPlaneExtra + 0 && t.slot[3].plane == kLocalPlaneExtra + 1);
    for (uint32_t c = 1; c < 4; c++) EXPECT(t.slot[c].stride == 203);
  }
  for (uint32_t n = 1; n <= 4; n++) {  // 0 + n, on a VarDCT frame: the channels' own size, their own bit depth
    LocalDestState v;
    v.in_frame = true;
    for (uint32_t i = 0; i < 4; i++) v.ec[i].set = true, v.ec[i].w = 128, v.ec[i].h = 96;
    std::vector<uint32_t> ec;
    for (uint32_t k = 0; k < n; k++) ec.push_back(3 - k);
    const LocalDestTable t = plan_local_dest(dest_of(0, ec, 12), 0, v);
    EXPECT(t.status == JXLH_OK && t.n_slots == n && !t.fan && !t.mixed() && t.w == 128 && t.h == 96 && t.bit_depth == 12);
    for (uint32_t k = 0; k < n; k++) EXPECT(t.slot[k].plane == kLocalPlaneExtra + 3 - k && t.slot[k].stride == 128);
    // ... and on a Modular frame of another size alike
    LocalDestState m = modular_state(400, 300, 448, 0);
    for (uint32_t i = 0; i < 4; i++) m.ec[i] = v.ec[i];
    const LocalDestTable u = plan_local_dest(dest_of(0, ec, 0), 0, m);
    EXPECT(u.status == JXLH_OK && u.w == 128 && u.h == 96 && u.bit_depth == 0 && u.n_slots == n);
  }
  // XYB: depth 0 is a format of its own
  EXPECT(plan_local_dest(dest_of(3, {0}), JXLH_MODULAR_XYB, s).status == JXLH_OK);
  // 3 + 0 and 1 + 0: the frame form's plan, byte for byte
  for (uint32_t n_colour : {3u, 1u}) {
    Call c;
    add_group(c, 0, 0, 128, 128, n_colour, {}, 1);
    add_group(c, 128, 0, 75, 137, n_colour, n_colour == 3 ? std::vector<jxlh_local_step>{rct(0, 10)} : std::vector<jxlh_local_step>{}, 0);
    add_group(c, 0, 128, 64, 9, n_colour, {pal(c, 0, n_colour, 40, 6, 5)}, 0);
    add_group(c, 64, 128, 64, 9, n_colour, {pal(c, 0, 1, 17, 0, 0)}, 0, 3);
    const LocalDestTable t = plan_local_dest(dest_of(n_colour, {}), 8, s);
    EXPECT(t.status == JXLH_OK && t.n_slots == n_colour && !t.mixed() && t.fan == (n_colour == 1));
    for (bool aligned : {true, false}) {
      const LocalPlan a = plan_with(c, t, aligned);
      LocalBatchIn in = c.in();
      in.n_out = 3, in.w = 203, in.h = 137, in.frame = true, in.bit_depth = 8;
      const LocalPlan b = plan_local_batch(in, aligned);
      EXPECT(a.status == JXLH_OK && b.status == JXLH_OK && !a.steps.empty());
      EXPECT(same_steps(a, b) && a.scratch == b.scratch && a.layout.total == b.layout.total && bytes_of(a) == bytes_of(b));
    }
  }
}

// ---------------------------------------------------------------- the refusals
static void refuse_dest(const jxlh_local_dest& d, uint32_t fmt, const LocalDestState& s, jxlh_status st, const char* why, int line) {
  const LocalDestTable t = plan_local_dest(d, fmt, s);
  if (t.status != st || !t.why || strcmp(t.why, why) != 0 || t.n_slots != 0) {
    fprintf(stderr, "line %d: status %d, \"%s\"\n", line, (int)t.status, t.why ? t.why : "(null)");
    fails++;
  }
}
#define REFUSE(d, fmt, s, st, why) refuse_dest(d, fmt, s, st, why, __LINE__)

static void test_refusals() {
  const LocalDestState s = modular_state(256, 128, 256, 2);
  REFUSE(dest_of(2, {0}), 8, s, INV, "n_colour is 0, 1 or 3");
  REFUSE(dest_of(4, {}), 8, s, INV, "n_colour is 0, 1 or 3");
  REFUSE(dest_of(0, {}), 0, s, INV, "n_colour + n_ec is 1..4");
  REFUSE(dest_of(3, {0, 1}), 8, s, INV, "n_colour + n_ec is 1..4");
  {
    jxlh_local_dest d = dest_of(0, {0});
    d.n_ec = 0xffffffffu;  // (the sum wraps to 0xffffffff + 0: caught by the first clause)
    REFUSE(d, 0, s, INV, "n_colour + n_ec is 1..4");
    d.n_colour = 1;  // 1 + 0xffffffff wraps to 0
    REFUSE(d, 8, s, INV, "n_colour + n_ec is 1..4");
  }
  REFUSE(dest_of(3, {JXLH_MAX_EXTRA_CHANNELS}), 8, s, INV, "an extra channel index out of range");
  REFUSE(dest_of(0, {1, 0, 1}), 0, s, INV, "an extra channel named twice");
  REFUSE(dest_of(3, {0}, 8), 8, s, INV, "bit_depth with colour channels: the depth is sample_format's");
  REFUSE(dest_of(0, {0}, 32), 0, s, INV, "a bit depth above 31");
  REFUSE(dest_of(0, {0}), 8, s, INV, "a sample_format without colour channels");
  REFUSE(dest_of(3, {0}), 0, s, INV, "a sample_format that names no sample type");
  REFUSE(dest_of(3, {0}), 32, s, INV, "a sample_format that names no sample type");
  REFUSE(dest_of(3, {0}), JXLH_MODULAR_XYB | 32, s, INV, "a sample_format that names no sample type");
  {
    LocalDestState o = s;
    o.in_frame = o.modular = false;
    REFUSE(dest_of(3, {0}), 8, o, BAD, "outside a frame");
    REFUSE(dest_of(0, {0}), 0, o, BAD, "outside a frame");
    o.in_frame = true;  // a VarDCT frame
    REFUSE(dest_of(3, {0}), 8, o, BAD, "colour channels on a VarDCT frame");
    EXPECT(plan_local_dest(dest_of(0, {0}), 0, o).status == JXLH_OK);
  }
  {
    LocalDestState o = s;
    o.sharded = true;
    REFUSE(dest_of(3, {0}), 8, o, UNS, "group-local transforms on a sharded context");
    REFUSE(dest_of(0, {0}), 0, o, UNS, "group-local transforms on a sharded context");
    o.sharded = false, o.subsampled = true;
    REFUSE(dest_of(3, {0}), 8, o, UNS, "group-local transforms on a chroma-subsampled frame");
    EXPECT(plan_local_dest(dest_of(0, {0}), 0, o).status == JXLH_OK);  // the extra channels are not subsampled
  }
  REFUSE(dest_of(3, {2}), 8, s, BAD, "a named extra channel is not set");
  REFUSE(dest_of(0, {0, 3}), 0, s, BAD, "a named extra channel is not set");
  {
    LocalDestState o = s;
    o.ec[1].w = 128, o.ec[1].h = 64;  // ec_upsampling 2: its own resolution
    REFUSE(dest_of(3, {1}), 8, o, UNS, "a named extra channel of another size than the call's planes");
    REFUSE(dest_of(0, {0, 1}), 0, o, UNS, "a named extra channel of another size than the call's planes");
    EXPECT(plan_local_dest(dest_of(0, {1}), 0, o).status == JXLH_OK);
    // not set comes before the size
    o.ec[0].set = false;
    REFUSE(dest_of(0, {1, 0}), 0, o, BAD, "a named extra channel is not set");
  }
  {
    LocalDestState o = s;
    o.mod_format = 16;
    REFUSE(dest_of(3, {0}), 8, o, INV, "another sample_format than the frame's earlier groups");
    EXPECT(plan_local_dest(dest_of(3, {0}), 16, o).status == JXLH_OK);
    EXPECT(plan_local_dest(dest_of(0, {0}), 0, o).status == JXLH_OK);  // no colour: the frame's format is not this call's
  }
  // ---- per group, decided by plan_local_batch: a refused plan holds no launch
  const LocalDestTable t = plan_local_dest(dest_of(3, {0}), 8, s);
  EXPECT(t.status == JXLH_OK);
  auto refused = [&](const Call& c, jxlh_status st, size_t bad, const char* why, int line) {
    const LocalPlan p = plan_with(c, t);
    if (p.status != st || p.first_bad != bad || !p.why || strcmp(p.why, why) != 0 || !p.steps.empty() || p.layout.total != 0) {
      fprintf(stderr, "line %d: status %d first_bad %zu \"%s\"\n", line, (int)p.status, p.first_bad, p.why ? p.why : "(null)");
      fails++;
    }
  };
  {
    Call c;
    add_group(c, 0, 0, 128, 128, 4, {rct(0, 10)}, 0);
    add_group(c, 128, 0, 128, 128, 3, {rct(0, 10)}, 0);
    refused(c, INV, 1, "the group's channels are not the destination's n_colour + n_ec", __LINE__);
  }
  {
    Call c;
    add_group(c, 0, 0, 128, 128, 4, {}, 0);
    add_group(c, 128, 0, 128, 128, 4, {}, 0);
    add_group(c, 129, 0, 128, 128, 4, {}, 0);
    refused(c, INV, 2, "the rect leaves the planes", __LINE__);
    c.groups[2].x0 = 128, c.groups[2].y0 = 0xffffff00u;  // y0 + h wraps in 32 bits
    refused(c, INV, 2, "the rect leaves the planes", __LINE__);
  }
  {  // what the squeeze-form lowering rejects, with its status: an RCT that leaves the channels; a squeeze in front
    Call c;
    add_group(c, 0, 0, 64, 64, 4, {}, 0);
    c.groups[0].n_steps = 1, c.groups[0].steps[0] = rct(2, 10);
    const LocalPlan p = plan_with(c, t);
    EXPECT(p.status == INV && p.first_bad == 0 && p.why && p.steps.empty());
    Call q;
    add_group(q, 0, 0, 64, 64, 4, {rct(0, 3)}, 1);
    q.groups[0].squeeze_pos = 0;
    const LocalPlan r = plan_with(q, t);
    EXPECT(r.status == UNS && r.first_bad == 0 && r.why && r.steps.empty());
  }
  {  // an empty group is checked, never planned; a batch of them is accepted and launches nothing
    Call c;
    add_group(c, 0, 0, 0, 128, 4, {}, 0);
    add_group(c, 256, 128, 0, 0, 4, {}, 0);
    const LocalPlan p = plan_with(c, t);
    EXPECT(p.status == JXLH_OK && p.steps.empty());
    c.groups[1].x0 = 257;
    refused(c, INV, 1, "the rect leaves the planes", __LINE__);
  }
}

// ---------------------------------------------------------------- alignment: a per-plane fact
static void test_alignment() {
  Call c;
  add_group(c, 0, 0, 128, 64, 4, {rct(0, 10)}, 0);
  add_group(c, 128, 0, 128, 64, 4, {pal(c, 0, 4, 30, 0, 0)}, 0);
  add_group(c, 0, 64, 127, 64, 4, {}, 0, 1);   // (a ragged width keeps the vector path: rows still start aligned)
  add_group(c, 129, 64, 64, 64, 4, {}, 0);     // an odd x0 never takes it
  const LocalDestTable ok = plan_local_dest(dest_of(3, {0}), 8, modular_state(256, 128, 256, 1));
  const LocalPlan base = plan_with(c, ok);
  EXPECT(base.status == JXLH_OK && base.groups.size() == 4);
  EXPECT(base.groups[0].vec == 1 && base.groups[1].vec == 1 && base.groups[2].vec == 1 && base.groups[3].vec == 0);
  // any one plane's base, or the arena's, takes the whole batch to the 4-byte path; nothing else changes
  for (int which = 0; which < 5; which++) {
    const LocalPlan p = plan_with(c, ok, which != 4, which != 0, which != 1, which != 2, which != 3);
    EXPECT(p.status == JXLH_OK && same_steps(p, base) && p.layout.total == base.layout.total && p.scratch == base.scratch);
    for (size_t g = 0; g < 4; g++) {
      LocalGroupDev a = p.groups[g], b = base.groups[g];
      EXPECT(a.vec == 0);
      a.vec = b.vec = 0;
      EXPECT(memcmp(&a, &b, sizeof a) == 0);
    }
  }
  // the fan planes count only where there is a fan
  EXPECT(plan_with(c, ok, true, true, true, true, true, false).groups[0].vec == 1);
  // a ragged extra-channel stride (203) drops every group that writes it; the frame planes' stride alone does not help
  const LocalDestTable ragged = plan_local_dest(dest_of(3, {0}), 8, modular_state(203, 137, 256, 1));
  Call r;
  add_group(r, 0, 0, 64, 64, 4, {}, 0);
  const LocalPlan pr = plan_with(r, ragged);
  EXPECT(pr.status == JXLH_OK && pr.groups[0].vec == 0);
  const LocalDestTable colour_only = plan_local_dest(dest_of(3, {}), 8, modular_state(203, 137, 256, 1));
  Call r3;
  add_group(r3, 0, 0, 64, 64, 3, {}, 0);
  EXPECT(plan_with(r3, colour_only).groups[0].vec == 1);
  // grey + alpha: the two fan planes are planes the group writes
  const LocalDestTable grey = plan_local_dest(dest_of(1, {0}), 8, modular_state(256, 128, 256, 1));
  Call g;
  add_group(g, 0, 0, 64, 64, 2, {}, 0);
  EXPECT(plan_with(g, grey).groups[0].vec == 1);
  EXPECT(plan_with(g, grey, true, true, true, true, true, false).groups[0].vec == 0);
  EXPECT(plan_with(g, grey, true, true, false).groups[0].vec == 0);
  EXPECT(plan_with(g, grey, true, true, true, false, false, true).groups[0].vec == 1);  // planes no slot names
}

// ---------------------------------------------------------------- the walk
// Every store a plan's launches make to the destination, on per-slot bitmaps of the planes (a byte per sample: how often
// it was written as a final value), with the addressing the kernels use: row (y0 + y) * stride + x0 + x of the slot's plane.
struct Walk {
  const LocalDestTable& t;
  std::vector<std::vector<uint8_t>> hit;  // per slot, stride * h
  std::vector<uint8_t> fan_hit;
  bool ok = true;
  explicit Walk(const LocalDestTable& table) : t(table) {
    for (uint32_t c = 0; c < t.n_slots; c++) hit.emplace_back((size_t)t.slot[c].stride * t.h, 0);
    if (t.fan) fan_hit.assign((size_t)t.slot[0].stride * t.h, 0);
  }
  void store(uint32_t slot, uint64_t x, uint64_t y) {
    if (slot >= t.n_slots || x >= t.w || y >= t.h) {
      ok = false;
      return;
    }
    hit[slot][(size_t)(y * t.slot[slot].stride + x)] = 1;
  }
  void fan(uint64_t x, uint64_t y) {
    if (!t.fan || x >= t.w || y >= t.h) ok = false;
    else fan_hit[(size_t)(y * t.slot[0].stride + x)] = 1;
  }
};
static void walk_plan(const LocalPlan& p, const Call& c, Walk& wk) {
  for (const LocalStep& st : p.steps) {
    if (st.kernel == LocalKernel::kLocal) {
      EXPECT(st.fan_grey == (wk.t.fan ? 1u : 0u));
      for (const LocalItem& it : p.items) {
        const LocalGroupDev& g = p.groups[it.group];
        const jxlh_local_squeeze_group& sg = c.groups[it.group];
        if (g.x0 != sg.x0 || g.y0 != sg.y0 || g.w != sg.w || g.h != sg.h || it.row0 >= g.h || g.rows_per_item == 0) wk.ok = false;
        const uint32_t end = it.row0 + std::min(g.rows_per_item, g.h - it.row0);
        for (uint32_t y = it.row0; y < end; y++)
          for (uint32_t x = 0; x < g.w; x++) {
            for (uint32_t s = 0; s < g.n_channels; s++) wk.store(s, (uint64_t)g.x0 + x, (uint64_t)g.y0 + y);
            if (st.fan_grey) wk.fan((uint64_t)g.x0 + x, (uint64_t)g.y0 + y);
          }
      }
    } else if (st.kernel == LocalKernel::kPhase || st.kernel == LocalKernel::kPalette) {
      for (uint32_t ph = 0; ph < kLpMaxPhases; ph++) {
        if (p.layout.phase_items[ph].off != st.items.off || p.general.items[ph].empty()) continue;
        for (const LocalItem& it : p.general.items[ph]) {
          if (ph & 1) {
            const LpJobDev& j = p.general.jobs[ph][it.group];
            if (it.row0 >= j.n_slots) wk.ok = false;
            for (uint32_t y = 0; y < j.h; y++)
              for (uint32_t x = 0; x < j.w; x++) wk.store(j.out_slot[it.row0], (uint64_t)j.x0 + x, (uint64_t)j.y0 + y);
          } else {
            const LpPhaseDev& d = p.general.pointwise[ph][it.group];
            if (it.row0 >= d.h) wk.ok = false;
            const uint32_t end = it.row0 + std::min(d.rows_per_item, d.h - it.row0);
            for (uint32_t y = it.row0; y < end; y++)
              for (uint32_t x = 0; x < d.w; x++) {
                for (uint32_t s = 0; s < 4; s++)
                  if (d.dst[s].space == kLpOut) wk.store(s, (uint64_t)d.x0 + x, (uint64_t)d.y0 + y);
                if (d.fan) wk.fan((uint64_t)d.x0 + x, (uint64_t)d.y0 + y);
              }
          }
        }
      }
    } else {  // a chain writes the destination at its last level only
      const bool lds = st.kernel == LocalKernel::kSqueezeLds;
      const std::vector<LocalItem>& items = lds ? p.squeeze.lds_items : p.squeeze.level_items[st.step];
      for (const LocalItem& it : items) {
        const LsChainDev& ch = p.squeeze.chains[it.group];
        const uint32_t level = lds ? ch.n_lds - 1 : ch.n_lds + st.step;  // the last level this launch runs of the chain
        if (level >= ch.n_levels) wk.ok = false;
        if (level + 1 != ch.n_levels) continue;
        const LsLevelDev& L = ch.lv[level];
        if (lds) {
          for (uint32_t y = 0; y < L.out_h; y++)
            for (uint32_t x = 0; x < L.out_w; x++) wk.store(ch.slot, (uint64_t)ch.x0 + x, (uint64_t)ch.y0 + y);
        } else {  // kLsLines lines from it.row0: rows of a horizontal level, columns of a vertical one
          const uint32_t n_lines = L.horizontal ? L.out_h : L.out_w, n_out = L.horizontal ? L.out_w : L.out_h;
          for (uint32_t l = it.row0; l < std::min(n_lines, it.row0 + (uint32_t)kLsLines); l++)
            for (uint32_t i = 0; i < n_out; i++)
              wk.store(ch.slot, (uint64_t)ch.x0 + (L.horizontal ? i : l), (uint64_t)ch.y0 + (L.horizontal ? l : i));
        }
      }
    }
  }
}

static void test_walk(int n_batches) {
  const uint32_t layouts[][2] = {{3, 1}, {1, 1}, {1, 3}, {1, 2}, {0, 1}, {0, 2}, {0, 3}, {0, 4}, {3, 0}, {1, 0}};
  for (int b = 0; b < n_batches; b++) {
    const uint32_t* lay = layouts[rnd(10)];
    const uint32_t n_ch = lay[0] + lay[1];
    const uint32_t W = 1 + rnd(48), H = 1 + rnd(40), stride = (W + 3) / 4 * 4 + 4 * rnd(3);
    LocalDestState s = modular_state(W, H, stride, 4);
    std::vector<uint32_t> ec;
    for (uint32_t k = 0; k < lay[1]; k++) ec.push_back((k + b) % 4);
    const LocalDestTable t = plan_local_dest(dest_of(lay[0], ec, lay[0] ? 0 : 8), lay[0] ? 8 : 0, s);
    if (t.status != JXLH_OK) {
      EXPECT(t.status == JXLH_OK);
      return;
    }
    // a grid of cells over the planes, each a group; some empty
    Call c;
    const uint32_t cw = 1 + rnd(W), chh = 1 + rnd(H);
    std::vector<uint8_t> want((size_t)W * H, 0);
    for (uint32_t y0 = 0; y0 < H; y0 += chh)
      for (uint32_t x0 = 0; x0 < W; x0 += cw) {
        if (c.groups.size() >= 6) break;
        uint32_t w = std::min(cw, W - x0), h = std::min(chh, H - y0);
        const uint32_t kind = rnd(8);
        if (kind == 7) (rnd(2) ? w : h) = 0;
        std::vector<jxlh_local_step> steps;
        if ((kind & 1) && n_ch >= 3) steps.push_back(rct(rnd(n_ch - 2), rnd(42)));
        if (kind & 2) {
          const uint32_t num_c = 1 + rnd(n_ch), begin = rnd(n_ch - num_c + 1), pred = rnd(3) ? 0 : (rnd(2) ? 5 : 6);
          steps.push_back(pal(c, begin, num_c, 1 + rnd(20), pred ? rnd(4) : 0, pred));
        }
        add_group(c, x0, y0, w, h, n_ch, steps, (kind & 4) && w && h ? 1 : 0, rnd(3));
        for (uint32_t y = 0; y < h; y++)
          for (uint32_t x = 0; x < w; x++) want[(size_t)(y0 + y) * W + x0 + x] = 1;
      }
    const LocalPlan p = plan_with(c, t, rnd(2), rnd(2), rnd(2), rnd(2), rnd(2), rnd(2));
    if (p.status != JXLH_OK) {
      fprintf(stderr, "batch %d refused: %s\n", b, p.why ? p.why : "(null)");
      fails++;
      return;
    }
    Walk wk(t);
    walk_plan(p, c, wk);
    bool cover = true;
    for (uint32_t s2 = 0; s2 < t.n_slots; s2++)
      for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < t.slot[s2].stride; x++) {
          const uint8_t got = wk.hit[s2][(size_t)y * t.slot[s2].stride + x];
          cover = cover && got == (x < W ? want[(size_t)y * W + x] : 0);
        }
    if (t.fan)
      for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < stride; x++) cover = cover && wk.fan_hit[(size_t)y * stride + x] == (x < W ? want[(size_t)y * W + x] : 0);
    if (!wk.ok || !cover) {
      fprintf(stderr, "batch %d (%u + %u channels, %u x %u): %s\n", b, lay[0], lay[1], W, H, wk.ok ? "coverage" : "a store leaves its plane");
      fails++;
      return;
    }
  }
}

int main(int argc, char** argv) {
  test_tables();
  test_refusals();
  test_alignment();
  test_walk(argc > 1 ? atoi(argv[1]) : 100000);
  if (fails) {
    printf("modular local plan extra: %d failures\n", fails);
    return 1;
  }
  printf("modular local plan extra: ok\n");
  return 0;
}
