// The host lowering of group-local transform lists (jxl_rs_amd/csrc/modular_local_host.h) on its own: plain C++, no
// device, no library -- the program a sanitizer build runs (-fsanitize=address,undefined).  Known lists, the documented
// refusals, and a deterministic sweep of random descriptors (any field may hold any value: the lowering must refuse
// or accept without reading or writing out of bounds).
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
static jxlh_local_step pal(uint32_t begin, uint32_t num_c, uint32_t colors, uint64_t off) {
  jxlh_local_step s;
  memset(&s, 0, sizeof s);
  s.kind = JXLH_LOCAL_PALETTE, s.begin_c = begin, s.num_c = num_c, s.num_colors = colors, s.palette_offset = off;
  return s;
}

int main() {
  const uint64_t arena = 2000;
  jxlh_local_program p;
  const char* why = nullptr;
  {  // [Palette(2, 1), RCT(begin_c = 1)]: the meta channel shifts the RCT onto channels 0, 1, 2
    jxlh_local_group g = group(3, 3);
    g.n_steps = 2;
    g.steps[0] = pal(2, 1, 6, 0);
    g.steps[1] = rct(1, 10);
    EXPECT(local_lower_group(g, 8, arena, &p, &why) == JXLH_OK);
    EXPECT(p.n_coded == 3 && p.n_ops == 2 && p.ops[0].kind == JXLH_LOCAL_RCT && p.ops[0].rct_op == 3);
    EXPECT(p.ops[0].in_slot[0] == 0 && p.ops[0].in_slot[1] == 1 && p.ops[0].in_slot[2] == 2);
    EXPECT(p.ops[0].out_slot[0] == 1 && p.ops[0].out_slot[1] == 2 && p.ops[0].out_slot[2] == 0);
    EXPECT(p.ops[1].kind == JXLH_LOCAL_PALETTE && p.ops[1].in_slot[0] == 2 && p.ops[1].out_slot[0] == 2 && p.ops[1].n_slots == 1);
  }
  {  // four palettes of one channel each: the list grows to its longest (4 image + 4 meta channels)
    jxlh_local_group g = group(4, 4);
    g.n_steps = 4;
    for (uint32_t i = 0; i < 4; i++) g.steps[i] = pal(2 * i, 1, 5, 10 * i);
    EXPECT(local_lower_group(g, 8, arena, &p, &why) == JXLH_OK);
    EXPECT(p.n_coded == 4 && p.ops[0].in_slot[0] == 3 && p.ops[3].in_slot[0] == 0);
  }
  {  // refusals
    jxlh_local_group g = group(3, 1);
    g.n_steps = 2;
    g.steps[0] = pal(0, 3, 6, 0);
    g.steps[1] = rct(0, 0);
    EXPECT(local_lower_group(g, 8, arena, &p, &why) == JXLH_ERR_INVALID_ARGUMENT && why);
    g.steps[1] = pal(0, 1, 6, 0);  // the meta channel itself
    EXPECT(local_lower_group(g, 8, arena, &p, &why) == JXLH_ERR_UNSUPPORTED);
    g.n_steps = 1;
    g.coded_offset[0] = ~0ull;
    EXPECT(local_lower_group(g, 8, arena, &p, &why) == JXLH_ERR_INVALID_ARGUMENT);
    g.coded_offset[0] = arena - (3 * 8 + 8);
    EXPECT(local_lower_group(g, 8, arena, &p, &why) == JXLH_OK);
    g.steps[0].palette_offset = arena - 17;
    EXPECT(local_lower_group(g, 8, arena, &p, &why) == JXLH_ERR_INVALID_ARGUMENT);
  }
  // random descriptors: xorshift-filled structs with the small fields folded into (a little beyond) their ranges
  uint64_t s = 0x9e3779b97f4a7c15ull;
  auto next = [&]() {
    s ^= s << 13, s ^= s >> 7, s ^= s << 17;
    return s;
  };
  int accepted = 0;
  for (int it = 0; it < 200000; it++) {
    jxlh_local_group g;
    uint64_t* raw = reinterpret_cast<uint64_t*>(&g);
    for (size_t i = 0; i < sizeof g / 8; i++) raw[i] = next();
    g.n_channels = next() % 6, g.n_steps = next() % 6, g.n_coded = next() % 6;
    g.w = next() % 64, g.h = next() % 64, g.coded_stride = g.w + next() % 3;
    for (int i = 0; i < 4; i++) {
      jxlh_local_step& t = g.steps[i];
      t.kind = next() % 3, t.begin_c = next() % 6, t.rct_type = next() % 44, t.num_c = next() % 5;
      t.num_colors = next() % 300, t.num_deltas = next() % 8 == 0, t.predictor = next() % 8 == 0;
      if (next() % 4) t.palette_offset %= 4096;
      if (next() % 4) g.coded_offset[i] %= 4096;
    }
    const jxlh_status st = local_lower_group(g, (uint32_t)(next() % 34), 1 << 16, &p, &why);
    EXPECT(st == JXLH_OK || st == JXLH_ERR_INVALID_ARGUMENT || st == JXLH_ERR_UNSUPPORTED);
    if (st == JXLH_OK) {
      accepted++;
      EXPECT(p.n_coded == g.n_coded && p.n_ops == g.n_steps);
      for (uint32_t k = 0; k < p.n_ops; k++)
        for (int i = 0; i < 4; i++) EXPECT(p.ops[k].out_slot[i] < 4 && (i == 3 || p.ops[k].in_slot[i] < 4));
    }
  }
  EXPECT(accepted > 100);
  if (fails) return 1;
  printf("modular local lowering: ok (%d random descriptors accepted)\n", accepted);
  return 0;
}
