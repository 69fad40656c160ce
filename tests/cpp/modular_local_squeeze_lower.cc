// The lowering of group-local squeezes (jxl_rs_amd/csrc/modular_local_squeeze_host.h) on its own: plain C++, no device,
// no library -- the program a sanitizer build runs (-fsanitize=address,undefined).
//   modular_local_squeeze_lower            known lists, the documented refusals, and a deterministic sweep of random
//                                          descriptors (any field may hold any value)
//   modular_local_squeeze_lower LISTS      lowers the groups of the file LISTS, one per line
//                                            w h n_channels n_steps { kind begin_c rct_type num_c num_colors num_deltas predictor }
//                                            has_squeeze n_params { horizontal in_place begin_c num_c } n_coded { w h }
//                                          and prints per group
//                                            status n_coded n_chains { slot base base_w base_h n_levels { horizontal out_w out_h res } }
//                                          for the test to compare with the restatement of the reference.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../jxl_rs_amd/csrc/modular_local_squeeze_host.h"

using namespace jxlh;

static int fails = 0;
#define EXPECT(c)                                        \
  do {                                                   \
    if (!(c)) {                                          \
      fprintf(stderr, "line %d: %s\n", __LINE__, #c);    \
      fails++;                                           \
    }                                                    \
  } while (0)

static const uint64_t kArena = 1u << 24;
static const jxlh_wp_header kWp = {16, 10, 7, 7, 7, 0, 0, 13, 12, 12, 12};

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

// a group with a squeeze behind n_steps steps, and the coded channels the list `sizes` (w, h pairs) names, packed tightly
struct Batch {
  jxlh_local_squeeze_group g;
  std::vector<jxlh_local_coded_channel> coded;
  std::vector<jxlh_squeeze_params> params;
  jxlh_status lower(jxlh_local_squeeze_program* p, const char** why = nullptr, uint64_t arena = kArena) const {
    return local_lower_squeeze_group(g, coded.data(), coded.size(), params.data(), params.size(), &kWp, 8, arena, p, why);
  }
  void set_coded(const std::vector<uint32_t>& sizes) {
    coded.clear();
    uint64_t at = 4096;
    for (size_t i = 0; i + 1 < sizes.size(); i += 2) {
      coded.push_back(jxlh_local_coded_channel{at, sizes[i], sizes[i], sizes[i + 1]});
      at += (uint64_t)sizes[i] * sizes[i + 1];
    }
    g.coded_first = 0, g.n_coded = (uint32_t)coded.size();
  }
};
static Batch batch(uint32_t w, uint32_t h, uint32_t n_channels, std::vector<jxlh_squeeze_params> params = {}) {
  Batch b;
  memset(&b.g, 0, sizeof b.g);
  b.g.w = w, b.g.h = h, b.g.n_channels = n_channels;
  b.g.has_squeeze = 1;
  b.params = params;
  b.g.n_params = (uint32_t)params.size();
  return b;
}

static int run_lists(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) return 2;
  unsigned w, h, n_channels, n_steps;
  while (fscanf(f, "%u %u %u %u", &w, &h, &n_channels, &n_steps) == 4) {
    if (n_steps > JXLH_LOCAL_MAX_STEPS) return 2;
    Batch b = batch(w, h, n_channels);
    b.g.n_steps = n_steps;
    for (unsigned i = 0; i < n_steps; i++) {
      unsigned v[7];
      for (unsigned& x : v)
        if (fscanf(f, "%u", &x) != 1) return 2;
      b.g.steps[i] = v[0] == JXLH_LOCAL_RCT ? rct(v[1], v[2]) : pal(v[1], v[3], v[4], v[5], v[6], 1000 * i);
      b.g.steps[i].kind = v[0];
    }
    unsigned has, n_params, n_coded;
    if (fscanf(f, "%u %u", &has, &n_params) != 2) return 2;
    b.g.has_squeeze = has, b.g.squeeze_pos = has ? n_steps : 0, b.g.n_params = n_params;
    for (unsigned i = 0; i < n_params; i++) {
      unsigned v[4];
      for (unsigned& x : v)
        if (fscanf(f, "%u", &x) != 1) return 2;
      b.params.push_back(jxlh_squeeze_params{v[0], v[1], v[2], v[3]});
    }
    if (fscanf(f, "%u", &n_coded) != 1) return 2;
    std::vector<uint32_t> sizes;
    for (unsigned i = 0; i < 2 * n_coded; i++) {
      unsigned x;
      if (fscanf(f, "%u", &x) != 1) return 2;
      sizes.push_back(x);
    }
    b.set_coded(sizes);
    jxlh_local_squeeze_program p;
    const jxlh_status st = b.lower(&p);
    printf("%d", (int)st);
    if (st == JXLH_OK) {
      printf(" %u %u", p.n_coded, p.general.n_coded);
      for (uint32_t k = 0; k < p.general.n_coded; k++) {
        const jxlh_local_squeeze_chain& c = p.chains[k];
        printf(" %u %u %u %u %u", p.general.coded_slot[k], c.base, c.base_w, c.base_h, c.n_levels);
        for (uint32_t i = 0; i < c.n_levels; i++)
          printf(" %u %u %u %u", c.levels[i].horizontal, c.levels[i].out_w, c.levels[i].out_h, c.levels[i].res);
      }
    }
    printf("\n");
  }
  fclose(f);
  return 0;
}

// an accepted program is well formed: every chain's levels double from the base to the group's size, every coded channel
// is used exactly once
static void check_program(const Batch& b, const jxlh_local_squeeze_program& p) {
  EXPECT(p.n_coded == b.g.n_coded && p.general.n_coded >= 1 && p.general.n_coded <= 4);
  std::vector<int> used(p.n_coded, 0);
  for (uint32_t k = 0; k < p.general.n_coded; k++) {
    const jxlh_local_squeeze_chain& c = p.chains[k];
    EXPECT(c.n_levels <= JXLH_LOCAL_SQUEEZE_MAX_LEVELS && c.base < p.n_coded);
    if (c.base < p.n_coded) used[c.base]++;
    uint32_t cw = c.base_w, ch = c.base_h;
    for (uint32_t i = 0; i < c.n_levels && i < JXLH_LOCAL_SQUEEZE_MAX_LEVELS; i++) {
      const jxlh_local_squeeze_level& l = c.levels[i];
      EXPECT(l.horizontal ? (cw == (l.out_w + 1) / 2 && ch == l.out_h) : (cw == l.out_w && ch == (l.out_h + 1) / 2));
      EXPECT(l.res < p.n_coded);
      if (l.res < p.n_coded) {
        used[l.res]++;
        const jxlh_local_coded_channel& r = b.coded[b.g.coded_first + l.res];
        EXPECT(l.horizontal ? (r.w == l.out_w / 2 && r.h == l.out_h) : (r.w == l.out_w && r.h == l.out_h / 2));
      }
      cw = l.out_w, ch = l.out_h;
    }
    EXPECT(cw == b.g.w && ch == b.g.h);
  }
  for (int u : used) EXPECT(u == 1);
}

int main(int argc, char** argv) {
  if (argc > 1) return run_lists(argv[1]);
  jxlh_local_squeeze_program p;
  const char* why = nullptr;
  {  // default squeeze of 9 x 9, one channel: v, then h.  The list after v: [a 9x5, r 9x4]; after h: [a 5x5, r 4x5, r 9x4];
     // the inverse runs h first
    Batch b = batch(9, 9, 1);
    b.set_coded({5, 5, 4, 5, 9, 4});
    EXPECT(b.lower(&p, &why) == JXLH_OK);
    EXPECT(p.n_coded == 3 && p.chains[0].n_levels == 2 && p.chains[0].base == 0 && p.chains[0].base_w == 5 && p.chains[0].base_h == 5);
    EXPECT(p.chains[0].levels[0].horizontal == 1 && p.chains[0].levels[0].out_w == 9 && p.chains[0].levels[0].out_h == 5 && p.chains[0].levels[0].res == 1);
    EXPECT(p.chains[0].levels[1].horizontal == 0 && p.chains[0].levels[1].out_w == 9 && p.chains[0].levels[1].out_h == 9 && p.chains[0].levels[1].res == 2);
    check_program(b, p);
    b.coded[1].w = 5;  // a size that is not what the transforms leave
    EXPECT(b.lower(&p, &why) == JXLH_ERR_INVALID_ARGUMENT);
    b.coded[1].w = 4, b.coded[2].stride = 8;
    EXPECT(b.lower(&p, &why) == JXLH_ERR_INVALID_ARGUMENT);  // stride < w
    b.coded[2].stride = 9, b.coded[2].offset = kArena - 9 * 4;
    EXPECT(b.lower(&p, &why) == JXLH_OK);
    b.coded[2].offset = kArena - 9 * 4 + 1;
    EXPECT(b.lower(&p, &why) == JXLH_ERR_INVALID_ARGUMENT);  // beyond the arena
    b.coded[2].offset = ~0ull - 3;
    EXPECT(b.lower(&p, &why) == JXLH_ERR_INVALID_ARGUMENT);  // ... without wrapping
    b.coded[2].offset = 0;
    b.g.n_coded = 2;
    EXPECT(b.lower(&p, &why) == JXLH_ERR_UNSUPPORTED);  // a coded channel is missing
    b.coded.push_back(b.coded[2]);
    b.g.n_coded = 4;
    EXPECT(b.lower(&p, &why) == JXLH_ERR_INVALID_ARGUMENT);
    b.g.n_coded = 3, b.g.coded_first = 2;
    EXPECT(b.lower(&p, &why) == JXLH_ERR_INVALID_ARGUMENT);  // the range leaves the array
    b.g.coded_first = 0xffffffffu;
    EXPECT(b.lower(&p, &why) == JXLH_ERR_INVALID_ARGUMENT);
  }
  {  // 1024 x 1024, three channels: 2 preview levels + 14 on channels 1 and 2, exactly the limit
    Batch b = batch(1024, 1024, 3);
    // the coded list: the same bookkeeping on sizes only
    std::vector<uint32_t> sizes;
    struct E { uint32_t w, h; };
    std::vector<E> list = {{1024, 1024}, {1024, 1024}, {1024, 1024}};
    jxlh_squeeze_params d[kLsMaxDefaultParams];
    const uint32_t cw[3] = {1024, 1024, 1024};
    const uint32_t n = default_squeeze_list(cw, cw, 3, 0, d, kLsMaxDefaultParams);
    EXPECT(n == 2 + 14);
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t end = d[i].begin_c + d[i].num_c, at0 = d[i].in_place ? end : (uint32_t)list.size();
      for (uint32_t ic = 0; ic < d[i].num_c; ic++) {
        E& e = list[d[i].begin_c + ic];
        E r = e;
        if (d[i].horizontal) e.w = (e.w + 1) / 2, r.w -= e.w;
        else e.h = (e.h + 1) / 2, r.h -= e.h;
        list.insert(list.begin() + at0 + ic, r);
      }
    }
    for (const E& e : list) sizes.push_back(e.w), sizes.push_back(e.h);
    b.set_coded(sizes);
    EXPECT(b.lower(&p, &why) == JXLH_OK);
    EXPECT(p.chains[0].n_levels == 14 && p.chains[1].n_levels == 16 && p.chains[2].n_levels == 16);
    check_program(b, p);
    // one more level on channel 1: refused
    Batch c = batch(1024, 1024, 3);
    c.params.assign(d, d + n);
    c.params.push_back(jxlh_squeeze_params{1, 1, 1, 1});
    c.g.n_params = (uint32_t)c.params.size();
    c.set_coded(sizes);
    EXPECT(c.lower(&p, &why) == JXLH_ERR_UNSUPPORTED);
  }
  {  // the refusals that need no coded channels
    Batch b = batch(16, 16, 3, {jxlh_squeeze_params{1, 1, 0, 4}});
    EXPECT(b.lower(&p, &why) == JXLH_ERR_INVALID_ARGUMENT);  // InvalidChannelRange
    b.params[0] = jxlh_squeeze_params{1, 1, 0xffffffffu, 2};
    EXPECT(b.lower(&p, &why) == JXLH_ERR_INVALID_ARGUMENT);
    b.params[0] = jxlh_squeeze_params{1, 1, 1, 0};
    EXPECT(b.lower(&p, &why) == JXLH_ERR_INVALID_ARGUMENT);
    b.params = {jxlh_squeeze_params{1, 1, 0, 1}, jxlh_squeeze_params{0, 1, 1, 1}};  // [a, r, c1, c2]: position 1 is a residual
    b.g.n_params = 2;
    EXPECT(b.lower(&p, &why) == JXLH_ERR_UNSUPPORTED);
    b = batch(16, 16, 3);
    b.g.n_steps = 1, b.g.squeeze_pos = 1;
    b.g.steps[0] = pal(0, 3, 6, 0, 0, 0);  // [meta, idx]
    b.params = {jxlh_squeeze_params{1, 1, 0, 2}};
    b.g.n_params = 1;
    EXPECT(b.lower(&p, &why) == JXLH_ERR_UNSUPPORTED);  // touches the meta channel
    b.params[0] = jxlh_squeeze_params{1, 1, 1, 1};
    b.set_coded({8, 16, 8, 16});
    EXPECT(b.lower(&p, &why) == JXLH_OK && p.general.n_coded == 1 && p.chains[0].n_levels == 1);
    b.g.squeeze_pos = 0;
    EXPECT(b.lower(&p, &why) == JXLH_ERR_UNSUPPORTED);  // a transform behind the squeeze
    b.g.squeeze_pos = 2;
    EXPECT(b.lower(&p, &why) == JXLH_ERR_INVALID_ARGUMENT);
    b.g.squeeze_pos = 1, b.g.has_squeeze = 2;
    EXPECT(b.lower(&p, &why) == JXLH_ERR_INVALID_ARGUMENT);
    b.g.has_squeeze = 0;
    EXPECT(b.lower(&p, &why) == JXLH_ERR_INVALID_ARGUMENT);  // parameters without a squeeze
    b.g.has_squeeze = 1, b.g.steps[0].kind = 2;
    EXPECT(b.lower(&p, &why) == JXLH_ERR_UNSUPPORTED);  // a second squeeze among the steps
    b.g.steps[0].kind = JXLH_LOCAL_PALETTE, b.g.params_first = 1;
    EXPECT(b.lower(&p, &why) == JXLH_ERR_INVALID_ARGUMENT);  // the parameter range leaves the array
    b.g.params_first = 0, b.g.w = (1u << 20) + 1;
    EXPECT(b.lower(&p, &why) == JXLH_ERR_UNSUPPORTED);
  }
  // random descriptors: refuse or accept, never read or write out of bounds; an accepted program is well formed
  uint64_t s = 0x9e3779b97f4a7c15ull;
  auto next = [&]() {
    s ^= s << 13, s ^= s >> 7, s ^= s << 17;
    return s;
  };
  int accepted = 0, squeezed = 0;
  for (int it = 0; it < 60000; it++) {
    Batch b;
    uint32_t* raw = reinterpret_cast<uint32_t*>(&b.g);
    for (size_t i = 0; i < sizeof b.g / 4; i++) raw[i] = (next() & 7) ? (uint32_t)(next() % 5) : (uint32_t)next();
    for (uint32_t i = 0; i < 4; i++) b.g.steps[i].palette_offset = next() % 3000;
    b.g.w = (uint32_t)(next() % 40), b.g.h = (uint32_t)(next() % 40);
    if (next() & 7) b.g.n_channels = 1 + (uint32_t)(next() % 4);
    if (next() & 3) b.g.n_steps = 0;
    if (next() & 3) b.g.has_squeeze = 1, b.g.squeeze_pos = b.g.n_steps;
    const uint32_t np = (uint32_t)(next() % 6);
    for (uint32_t i = 0; i < np; i++)
      b.params.push_back(jxlh_squeeze_params{(uint32_t)(next() & 1), (uint32_t)(next() & 1), (uint32_t)(next() % 4), (uint32_t)(next() % 4)});
    if (next() & 1) b.g.params_first = 0, b.g.n_params = np;
    // the coded channels: mostly the sizes a size-only run of the same parameters gives (groups without steps),
    // random ones otherwise
    std::vector<uint32_t> sizes;
    {
      struct E { uint32_t w, h; bool res; };
      std::vector<E> list(b.g.n_channels <= 4 ? b.g.n_channels : 0, E{b.g.w, b.g.h, false});
      bool ok = b.g.n_steps == 0 && !list.empty();
      jxlh_squeeze_params d[kLsMaxDefaultParams];
      std::vector<jxlh_squeeze_params> ps(b.params.begin(), b.params.begin() + (b.g.n_params <= np ? b.g.n_params : 0));
      if (ok && b.g.has_squeeze == 1 && ps.empty()) {
        uint32_t cw[4], ch[4];
        for (size_t k = 0; k < list.size(); k++) cw[k] = b.g.w, ch[k] = b.g.h;
        const uint32_t n = default_squeeze_list(cw, ch, (uint32_t)list.size(), 0, d, kLsMaxDefaultParams);
        ps.assign(d, d + n);
      }
      for (size_t i = 0; ok && b.g.has_squeeze == 1 && i < ps.size(); i++) {
        const uint64_t end = (uint64_t)ps[i].begin_c + ps[i].num_c;
        if (end > list.size() || ps[i].num_c == 0) { ok = false; break; }
        const size_t at0 = ps[i].in_place ? (size_t)end : list.size();
        for (uint32_t ic = 0; ic < ps[i].num_c; ic++) {
          E& e = list[ps[i].begin_c + ic];
          E r = e;
          r.res = true;
          if (ps[i].horizontal) e.w = (e.w + 1) / 2, r.w -= e.w;
          else e.h = (e.h + 1) / 2, r.h -= e.h;
          list.insert(list.begin() + at0 + ic, r);
        }
      }
      if (ok && (next() & 7)) for (const E& e : list) sizes.push_back(e.w), sizes.push_back(e.h);
      else for (uint32_t i = 0; i < 2 * (next() % 6); i++) sizes.push_back((uint32_t)(next() % 40));
    }
    const uint32_t first = b.g.coded_first, nc = b.g.n_coded;
    b.set_coded(sizes);
    if (!(next() & 7)) b.g.coded_first = first, b.g.n_coded = nc;
    jxlh_local_squeeze_program q;
    memset(&q, 0x5a, sizeof q);
    const jxlh_status st = b.lower(&q, &why, 1u << 20);
    if (st != JXLH_OK) continue;
    accepted++;
    check_program(b, q);
    for (uint32_t k = 0; k < q.general.n_coded; k++) squeezed += q.chains[k].n_levels > 0;
  }
  if (!(accepted > 1000 && squeezed > 1000)) fprintf(stderr, "accepted %d squeezed %d\n", accepted, squeezed);
  EXPECT(accepted > 1000 && squeezed > 1000);
  if (fails) return 1;
  printf("modular local squeeze lowering: ok (%d random programs accepted, %d squeezed chains)\n", accepted, squeezed);
  return 0;
}
