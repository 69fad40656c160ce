// Prints what every list of lowering_corpus.h lowers to, through lower() and through lower_modular_frame(): one line
//   <family> <index> <entry point> [<mutation>] -> <status> <what()>            for a rejected list
//   <family> <index> <entry point> [<mutation>] -> ok <every field of LoweredPipeline>   for an accepted one
// The C structs are printed word by word (all their fields are 32 bits wide), so floats appear as their bit patterns;
// weight tables as their index in lowering_corpus::kTables.  tools/record_pipeline_lowering.py digests the lines per
// family into tests/golden/pipeline_lowering.json, tests/test_pipeline_lowering_corpus_cpu.py compares against it.
// Exits 1 if a base list is not accepted by the entry point it belongs to.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "lowering_corpus.h"

using namespace jxlh;
using namespace lowering_corpus;

namespace {
void words(std::string& out, const char* name, const void* data, size_t bytes) {
  out += ' ';
  out += name;
  out += '=';
  char buf[16];
  for (size_t i = 0; i < bytes / 4; i++) {
    uint32_t w;
    memcpy(&w, (const char*)data + 4 * i, 4);
    snprintf(buf, sizeof buf, i ? ",%x" : "%x", w);
    out += buf;
  }
}
template <class T>
void words(std::string& out, const char* name, const T& v) {
  static_assert(sizeof(T) % 4 == 0 && std::is_trivially_copyable_v<T>);
  words(out, name, &v, sizeof(T));
}
template <class T>
void words(std::string& out, const char* name, const std::vector<T>& v) {
  static_assert(sizeof(T) % 4 == 0 && std::is_trivially_copyable_v<T>);
  out += ' ' + std::string(name) + ".size=" + std::to_string(v.size());
  words(out, name, v.data(), v.size() * sizeof(T));
}
void number(std::string& out, const char* name, long long v) { out += ' ' + std::string(name) + '=' + std::to_string(v); }

std::string serialise(const LoweredPipeline& lp) {
  std::string out;
  words(out, "frame", lp.frame);
  number(out, "has_output", lp.has_output);
  words(out, "output", lp.output);
  number(out, "upsampling_weights", table_index(lp.upsampling_weights));
  for (int i = 0; i < 3; i++) number(out, "weights_by_factor", table_index(lp.weights_by_factor[i]));
  number(out, "modular", (int)lp.modular);
  number(out, "modular_bits", lp.modular_bits);
  words(out, "modular_quant_factors", lp.modular_quant_factors);
  number(out, "i32_to_u8_multiplier", lp.i32_to_u8_multiplier);
  number(out, "i32_to_u8_max", lp.i32_to_u8_max);
  number(out, "modular_sample_format", lp.modular_sample_format);
  number(out, "input_border.x", lp.input_border.x);
  number(out, "input_border.y", lp.input_border.y);
  words(out, "extra", lp.extra);
  number(out, "has_patches", lp.has_patches);
  words(out, "patches", lp.patches.patches);
  words(out, "blendings", lp.patches.blendings);
  words(out, "ec_flags", lp.patches.ec_flags);
  number(out, "has_splines", lp.has_splines);
  words(out, "segments", lp.splines.segments);
  number(out, "has_blend", lp.has_blend);
  words(out, "blend", lp.blend);
  words(out, "blend_colour", lp.blend_colour);
  number(out, "saves.size", (long long)lp.saves.size());
  for (const jxlh_save_desc& d : lp.saves) words(out, "save", d);
  number(out, "out_w", lp.out_w);
  number(out, "out_h", lp.out_h);
  out += " stages=";
  for (const std::string& s : lp.stages) out += s + ';';
  return out;
}
}  // namespace

int main() {
  std::map<std::string, size_t> index;
  int bad_base = 0;
  for_each_list([&](const char* family, const List& l, const std::string& what) {
    const size_t i = index[family]++;
    for (const bool modular_frame : {false, true}) {
      std::string result;
      bool ok = false;
      try {
        const RenderPipelineBuilder b = build(l);
        result = "ok" + serialise(modular_frame ? b.lower_modular_frame() : b.lower());
        ok = true;
      } catch (const Error& e) {
        result = std::to_string((int)e.status) + " " + e.what();
      }
      printf("%s %zu %s [%s] -> %s\n", family, i, modular_frame ? "lower_modular_frame" : "lower", what.c_str(), result.c_str());
      if (!strcmp(family, "base") && modular_frame == l.modular_frame && !ok) bad_base++;
    }
  });
  if (bad_base) fprintf(stderr, "%d base lists are rejected by their own entry point\n", bad_base);
  return bad_base ? 1 : 0;
}
