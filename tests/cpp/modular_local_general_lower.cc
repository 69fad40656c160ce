// The general lowering of group-local transform lists (jxl_rs_amd/csrc/modular_local_host.h, general mode) on its own:
// plain C++, no device, no library -- the program a sanitizer build runs (-fsanitize=address,undefined).
//   modular_local_general_lower            the documented refusals, the default mode's unchanged refusals, and a
//                                          deterministic sweep of random descriptors (any field may hold any value)
//   modular_local_general_lower LISTS      lowers the lists of the file LISTS, one per line
//                                            n_channels n_steps { kind begin_c rct_type num_c num_colors num_deltas predictor }
//                                          and prints per list
//                                            status n_coded coded_slot[4] n_phases n_ops { kind rct_op n_slots in_slot[3]
//                                            out_slot[4] num_colors num_deltas predictor phase }
//                                          for the test to compare with the restatement of the reference.
#include <cstdio>
#include <cstring>

#include "../../jxl_rs_amd/csrc/modular_local_host.h"

using namespace jxlh;

static int fails = 0;
#define EXPECT(c)                                        \
  do {                                                   \
    if (!(c)) {                                          \
      fprintf(stderr, "line %d: %s\n", __LINE__, #c);    \
      fails++;                                           \
    }                                                    \
  } while (0)

static const uint64_t kArena = 100000;

static jxlh_local_group group(uint32_t n_channels, uint32_t n_coded) {
  jxlh_local_group g;
  memset(&g, 0, sizeof g);
  g.w = 8, g.h = 4, g.coded_stride = 8;
  g.n_channels = n_channels;
  g.n_coded = n_coded;
  for (uint32_t i = 0; i < 4; i++) g.coded_offset[i] = 1000 + 32 * i;
  return g;
}
static jxlh_local_step rct(uint32_t begin, uint32_t type) {
  jxlh_local_step s;
  memset(&s, 0, sizeof s);
  s.kind = JXLH_LOCAL_RCT, s.begin_c = begin, s.rct_type = type;
  return s;
}
static jxlh_local_step pal(uint32_t begin, uint32_t num_c, uint32_t colors, uint32_t deltas, uint32_t predictor, uint64_t off) {
  jxlh_local_step s;
  memset(&s, 0, sizeof s);
  s.kind = JXLH_LOCAL_PALETTE, s.begin_c = begin, s.num_c = num_c, s.num_colors = colors, s.num_deltas = deltas;
  s.predictor = predictor, s.palette_offset = off;
  return s;
}
static const jxlh_wp_header kWp = {16, 10, 7, 7, 7, 0, 0, 13, 12, 12, 12};

static jxlh_status lower(const jxlh_local_group& g, const jxlh_wp_header* wp, jxlh_local_general_program* p) {
  const char* why = nullptr;
  return local_lower_core(g, 8, kArena, true, wp, nullptr, p, &why);
}

static int run_lists(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) return 2;
  unsigned n_channels, n_steps;
  while (fscanf(f, "%u %u", &n_channels, &n_steps) == 2) {
    if (n_steps > JXLH_LOCAL_MAX_STEPS) return 2;
    jxlh_local_group g = group(n_channels, 1);
    g.n_steps = n_steps;
    for (unsigned i = 0; i < n_steps; i++) {
      unsigned v[7];
      for (unsigned& x : v)
        if (fscanf(f, "%u", &x) != 1) return 2;
      g.steps[i] = v[0] == JXLH_LOCAL_RCT ? rct(v[1], v[2]) : pal(v[1], v[3], v[4], v[5], v[6], 2000 + 1000 * i);
      g.steps[i].kind = v[0];
    }
    // n_coded is what the steps leave: find it (the lowering refuses every other value)
    jxlh_local_general_program p;
    jxlh_status st = JXLH_ERR_INVALID_ARGUMENT;
    for (uint32_t nc = 1; nc <= 4 && st != JXLH_OK; nc++) {
      g.n_coded = nc;
      st = lower(g, &kWp, &p);
    }
    printf("%d", (int)st);
    if (st == JXLH_OK) {
      printf(" %u %u %u %u %u %u %u", p.n_coded, p.coded_slot[0], p.coded_slot[1], p.coded_slot[2], p.coded_slot[3], p.n_phases, p.n_ops);
      for (uint32_t i = 0; i < p.n_ops; i++) {
        const jxlh_local_general_op& o = p.ops[i];
        printf(" %u %u %u %u %u %u %u %u %u %u %u %u %u %u", o.kind, o.rct_op, o.n_slots, o.in_slot[0], o.in_slot[1], o.in_slot[2],
               o.out_slot[0], o.out_slot[1], o.out_slot[2], o.out_slot[3], o.num_colors, o.num_deltas, o.predictor, o.phase);
      }
    }
    printf("\n");
  }
  fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1) return run_lists(argv[1]);
  jxlh_local_general_program p;
  jxlh_local_program old;
  const char* why = nullptr;
  {  // predictor 0 with deltas: the look-up op over num_colors + num_deltas entries, one phase
    jxlh_local_group g = group(3, 1);
    g.n_steps = 1;
    g.steps[0] = pal(0, 3, 11, 5, 0, 0);
    EXPECT(lower(g, nullptr, &p) == JXLH_OK);
    EXPECT(p.n_phases == 1 && p.ops[0].kind == JXLH_LOCAL_PALETTE && p.ops[0].num_colors == 16 && p.ops[0].num_deltas == 0);
    // ... which the default mode still refuses, like every predictor
    EXPECT(local_lower_group(g, 8, kArena, &old, &why) == JXLH_ERR_UNSUPPORTED);
    g.steps[0] = pal(0, 3, 11, 0, 5, 0);
    EXPECT(local_lower_group(g, 8, kArena, &old, &why) == JXLH_ERR_UNSUPPORTED);
    EXPECT(lower(g, nullptr, &p) == JXLH_OK && p.n_phases == 3 && p.ops[0].kind == JXLH_LOCAL_GENERAL_PALETTE && p.ops[0].phase == 1);
  }
  {  // RCT, general palette, RCT: phases 0, 1, 2
    jxlh_local_group g = group(3, 3);
    g.n_steps = 3;
    g.steps[0] = rct(0, 9), g.steps[1] = pal(0, 1, 40, 5, 5, 0), g.steps[2] = rct(1, 4);
    EXPECT(lower(g, nullptr, &p) == JXLH_OK);
    EXPECT(p.n_phases == 3 && p.ops[0].phase == 0 && p.ops[1].phase == 1 && p.ops[2].phase == 2);
    EXPECT(p.ops[1].in_slot[0] == 0 && p.ops[1].out_slot[0] == 0 && p.ops[1].num_colors == 45 && p.ops[1].num_deltas == 5);
  }
  {  // four general palettes of one channel each: the deepest program, 9 phases
    jxlh_local_group g = group(4, 4);
    g.n_steps = 4;
    // the list grows by one meta channel in front per step: channel i sits at position 2 i when its palette comes
    for (uint32_t i = 0; i < 4; i++) g.steps[i] = pal(2 * i, 1, 3, 2, 1 + i, 100 * i);
    EXPECT(lower(g, nullptr, &p) == JXLH_OK);
    EXPECT(p.n_phases == 9 && p.ops[0].phase == 1 && p.ops[3].phase == 7);
  }
  {  // the new refusals
    jxlh_local_group g = group(3, 1);
    g.n_steps = 1;
    g.steps[0] = pal(0, 3, 11, 5, 14, 0);
    EXPECT(lower(g, &kWp, &p) == JXLH_ERR_INVALID_ARGUMENT);
    g.steps[0].predictor = 6;
    EXPECT(lower(g, nullptr, &p) == JXLH_ERR_INVALID_ARGUMENT);
    EXPECT(lower(g, &kWp, &p) == JXLH_OK);
    jxlh_wp_header bad = kWp;
    bad.p3ce = 32;
    EXPECT(lower(g, &bad, &p) == JXLH_ERR_INVALID_ARGUMENT);
    bad = kWp, bad.w3 = 16;
    EXPECT(lower(g, &bad, &p) == JXLH_ERR_INVALID_ARGUMENT);
    bad.w3 = 15;
    EXPECT(lower(g, &bad, &p) == JXLH_OK);
    g.steps[0].predictor = 5;
    EXPECT(lower(g, &bad, &p) == JXLH_OK);  // a header nobody reads is not checked
    g.steps[0].palette_offset = kArena - 3 * 16;  // the rows are num_colors + num_deltas wide
    EXPECT(lower(g, nullptr, &p) == JXLH_OK);
    g.steps[0].palette_offset = kArena - 3 * 16 + 1;
    EXPECT(lower(g, nullptr, &p) == JXLH_ERR_INVALID_ARGUMENT);
    g.steps[0].palette_offset = 0;
    g.steps[0].num_colors = 0x7fffffffu - 5;
    EXPECT(lower(g, nullptr, &p) == JXLH_ERR_INVALID_ARGUMENT);  // 3 * (2^31 - 1) values leave the arena
    g.steps[0].num_colors = 0x7fffffffu - 4;
    EXPECT(lower(g, nullptr, &p) == JXLH_ERR_INVALID_ARGUMENT);  // num_colors + num_deltas > 2^31 - 1
    g.steps[0].num_colors = 0xffffffffu, g.steps[0].num_deltas = 0xffffffffu;
    EXPECT(lower(g, nullptr, &p) == JXLH_ERR_INVALID_ARGUMENT);
    g.steps[0] = pal(0, 3, 11, 5, 5, 0);
    g.steps[0].kind = 2;  // local squeeze stays on the host
    EXPECT(lower(g, nullptr, &p) == JXLH_ERR_UNSUPPORTED);
    g = group(3, 3);
    g.n_steps = 2;
    g.steps[0] = pal(1, 1, 6, 2, 3, 0), g.steps[1] = rct(0, 0);  // [meta, c0, idx, c2]: touches the meta channel
    EXPECT(lower(g, nullptr, &p) == JXLH_ERR_UNSUPPORTED);
  }
  // random descriptors: refuse or accept, never read or write out of bounds; an accepted program is well formed
  uint64_t s = 0x9e3779b97f4a7c15ull;
  auto next = [&]() {
    s ^= s << 13, s ^= s >> 7, s ^= s << 17;
    return s;
  };
  int accepted = 0;
  for (int it = 0; it < 200000; it++) {
    jxlh_local_group g;
    jxlh_wp_header wp;
    uint32_t* raw = reinterpret_cast<uint32_t*>(&g);
    for (size_t i = 0; i < sizeof g / 4; i++) raw[i] = (next() & 7) ? (uint32_t)(next() % 7) : (uint32_t)next();
    uint32_t* rw = reinterpret_cast<uint32_t*>(&wp);
    for (size_t i = 0; i < sizeof wp / 4; i++) rw[i] = (uint32_t)(next() % 34);
    for (uint32_t i = 0; i < 4; i++) {
      g.coded_offset[i] = next() % 3000;
      g.steps[i].palette_offset = next() % 3000;
      g.steps[i].predictor = (uint32_t)(next() % 16);
    }
    g.w = 1 + next() % 8, g.h = 1 + next() % 4, g.coded_stride = g.w + next() % 3;
    jxlh_local_general_program q;
    memset(&q, 0x5a, sizeof q);
    const jxlh_status st = local_lower_core(g, 8, kArena, true, (next() & 3) ? &wp : nullptr, nullptr, &q, &why);
    if (st != JXLH_OK) continue;
    accepted++;
    EXPECT(q.n_ops <= 4 && q.n_coded >= 1 && q.n_coded <= 4 && q.n_phases <= 2 * JXLH_LOCAL_MAX_STEPS + 1);
    uint32_t last = 0;
    for (uint32_t i = 0; i < q.n_ops; i++) {
      const jxlh_local_general_op& o = q.ops[i];
      EXPECT(o.phase >= last && o.phase < q.n_phases && ((o.phase & 1) != 0) == (o.kind == JXLH_LOCAL_GENERAL_PALETTE));
      last = o.phase;
      EXPECT(o.n_slots >= 1 && o.n_slots <= 4);
      for (uint32_t k = 0; k < o.n_slots && k < 4; k++) EXPECT(o.out_slot[k] < g.n_channels);
      if (o.kind != JXLH_LOCAL_RCT) EXPECT(o.in_slot[0] == o.out_slot[0] && o.palette_offset + (uint64_t)o.n_slots * o.num_colors <= kArena);
    }
  }
  EXPECT(accepted > 1000);
  if (fails) return 1;
  printf("modular local general lowering: ok (%d random programs accepted)\n", accepted);
  return 0;
}
