// A deterministic corpus of stage lists for RenderPipelineBuilder::lower() / lower_modular_frame(): the lists the host
// programs of this directory assemble after Frame::build_render_pipeline (frame/render.rs:526-903), and every list a
// small mutation makes of one of them -- a stage deleted, doubled, swapped with its neighbour, moved, two stages
// deleted, a foreign stage inserted, one field of a stage out of its range (alone and with a deletion), the builder's
// own arguments off.  No random numbers, no clock: the same lists in the same order on every run.  Lists are built
// through the builder's public calls only, so the file compiles against any revision of the header;
// lowering_dump.cc prints what each list lowers to or fails with, and tests/golden/pipeline_lowering.json pins that.
#pragma once
#include <cmath>
#include <functional>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "lowering_helpers.h"

namespace lowering_corpus {
using namespace jxlh;
using namespace lowering_helpers;

// the weight tables Upsample stages draw from (only their addresses matter to the lowering)
inline const float kTables[3][4] = {{1.0f}, {2.0f}, {3.0f}};
inline int table_index(const float* w) {
  for (int i = 0; i < 3; i++)
    if (w == kTables[i]) return i;
  return -1;
}

// A list as the builder's constructor and add_* calls take it.  The argument-less add_extend_stage() is kept as the
// CpuOnlyStage it becomes.
struct List {
  std::string name;
  bool modular_frame;  // the entry point the list belongs to
  size_t num_channels;
  std::pair<size_t, size_t> size;
  size_t shift, log_group;
  jxlh_frame_params params;
  std::vector<Stage> stages;
};
inline const char* const kBareExtend = "extend to image dimensions";

template <class S, class... Ts>
constexpr bool is_one_of = (std::is_same_v<S, Ts> || ...);

template <class S>
RenderPipelineBuilder add(RenderPipelineBuilder b, const S& st) {
  if constexpr (is_one_of<S, AddNoiseStage, XybStage, YcbcrToRgbStage, FromLinearStage, PatchesStage, SplinesStage, BlendingStage,
                          SpotColorStage, PremultiplyAlphaStage>)
    return std::move(b).add_inplace_stage(st);
  else
    return std::move(b).add_inout_stage(st);
}
inline RenderPipelineBuilder add(RenderPipelineBuilder b, const CpuOnlyStage& st) {
  return st.name == kBareExtend ? std::move(b).add_extend_stage() : std::move(b).add_inplace_stage(st);
}
inline RenderPipelineBuilder add(RenderPipelineBuilder b, const ExtendToImageDimensionsStage& st) {
  return std::move(b).add_extend_stage(st);
}
inline RenderPipelineBuilder add(RenderPipelineBuilder b, const SaveStage& st) {
  return st.full ? std::move(b).add_save_stage(st.channels, st.orientation, st.output_buffer_index, st.color_type, st.data_format,
                                               st.fill_opaque_alpha)
                 : std::move(b).add_save_stage(st.channels, st.output_buffer_index, st.color_channels, st.bits);
}
inline RenderPipelineBuilder build(const List& l) {
  RenderPipelineBuilder b(l.num_channels, l.size, l.shift, l.log_group, l.params);
  for (const Stage& s : l.stages) b = std::visit([&](const auto& st) { return add(std::move(b), st); }, s);
  return b;
}

// ---------------------------------------------------------------------------------------------------------------
// Base lists
inline SaveStage save4(std::vector<int> channels, int buffer, uint32_t color_channels, uint32_t bits) {
  return SaveStage{std::move(channels), buffer, color_channels, bits};
}
inline SaveStage save6(std::vector<int> channels, uint32_t orientation, int buffer, ColorType ct, DataFormat df, bool fill) {
  SaveStage st{std::move(channels), buffer, 0, 0};
  st.full = true;
  st.orientation = orientation;
  st.color_type = ct;
  st.data_format = df;
  st.fill_opaque_alpha = fill;
  return st;
}
struct Stages : std::vector<Stage> {
  template <class S>
  Stages& operator<<(S s) {
    emplace_back(std::move(s));
    return *this;
  }
  Stages& filters(const jxlh_frame_params& p, bool gab, int epf_iters) {
    const Rf rf = rf_of(p);
    if (gab)
      for (int c = 0; c < 3; c++) *this << GaborishStage{c, rf.gab_w1[c], rf.gab_w2[c]};
    if (epf_iters >= 3) *this << Epf0Stage{rf.pass0, rf.border_sad_mul, rf.channel_scale};
    if (epf_iters >= 1) *this << Epf1Stage{1.0f, rf.border_sad_mul, rf.channel_scale};
    if (epf_iters >= 2) *this << Epf2Stage{rf.pass2, rf.border_sad_mul, rf.channel_scale};
    return *this;
  }
  template <int N>
  Stages& upsample(const float* w, std::initializer_list<int> channels) {
    for (int c : channels) *this << Upsample<N>{w, c};
    return *this;
  }
  Stages& noise(int first) {
    for (int c = 0; c < 3; c++) *this << ConvolveNoiseStage{first + c};
    return *this << AddNoiseStage{{0.1f, 0.2f, 0.3f, 0.4f, 0.5f, 0.6f, 0.7f, 0.8f}, 3, -2, first};
  }
  // add_conversion_stages (frame/render.rs:868-873)
  Stages& convert(std::initializer_list<int> channels, DataFormat df, bool clamp = false, float lo = 0.0f, float hi = 0.0f) {
    for (int c : channels) {
      if (df.format == JXLH_SAVE_U8) *this << ConvertF32ToU8Stage{c, (uint8_t)df.bit_depth};
      if (df.format == JXLH_SAVE_U16) *this << ConvertF32ToU16Stage{c, (uint8_t)df.bit_depth};
      if (df.format == JXLH_SAVE_F16) *this << ConvertF32ToF16Stage{c, clamp, lo, hi};
    }
    return *this;
  }
  Stages& modular(uint8_t bits) {
    for (int c = 0; c < 3; c++) *this << ConvertModularToF32Stage{c, bits};
    return *this;
  }
};
inline const std::array<float, 3> kLum{0.2627f, 0.678f, 0.0593f};
inline PatchesStage dict(size_t num_ec) {
  PatchesStage ps;
  ps.patches = {jxlh_patch{4, 5, 0, 0, 0, 16, 12}, jxlh_patch{40, 30, 1, 8, 2, 10, 20}};
  ps.blendings.assign(ps.patches.size() * (1 + num_ec), jxlh_patch_blending{JXLH_PATCH_BLEND_ABOVE, 0, 1});
  ps.ec_flags.assign(num_ec, JXLH_EC_ALPHA);
  return ps;
}
inline SplinesStage segs() {
  SplinesStage st;
  st.segments = {jxlh_spline_segment{10.0f, 20.0f, 3.5f, 1.25f, 0.1f, {0.5f, 0.6f, 0.7f}},
                 jxlh_spline_segment{11.0f, 21.0f, 4.5f, -1.0f, -0.2f, {-0.8f, -0.8f, -0.7f}}};
  return st;
}
inline BlendingStage blend(size_t num_ec) {
  return blending(-40, 100, 1280, 1024, jxlh_blending_info{JXLH_BLEND_BLEND, 0, 1, 2}, num_ec,
                  jxlh_blending_info{JXLH_BLEND_ALPHA_WEIGHTED_ADD, 0, 0, 1});
}

inline std::vector<List> base_lists() {
  std::vector<List> out;
  const jxlh_frame_params full = base(1000, 700), half = base(500, 350), quarter = base(250, 175), eighth = base(125, 88);
  // VarDCT: Gaborish, EPF0/1/2, frame upsampling, noise, XYB + sRGB, u8, the four-argument save -- at 2x, 4x and 8x
  auto vardct = [&](const char* name, const jxlh_frame_params& p, size_t shift, auto ups) {
    Stages s;
    s.filters(p, true, 3);
    ups(s);
    s.noise(3) << XybStage{0, some_xyb()} << FromLinearStage{0, JXLH_TF_SRGB, 0.0f, {0.f, 0.f, 0.f}};
    s.convert({0, 1, 2}, DataFormat::u8()) << save4({0, 1, 2}, 0, 4, 8);
    out.push_back(List{name, false, 6, {1000, 700}, shift, 8, p, s});
  };
  vardct("vardct_2x", half, 1, [](Stages& s) { s.upsample<2>(kTables[0], {0, 1, 2}); });
  vardct("vardct_4x", quarter, 2, [](Stages& s) { s.upsample<4>(nullptr, {0, 1, 2}); });
  vardct("vardct_8x", eighth, 3, [](Stages& s) { s.upsample<8>(kTables[2], {0, 1, 2}); });
  {  // a JPEG recompression: 4:2:0 chroma, YCbCr, u16 (with the filters, upsampling and noise of the list above)
    Stages s;
    s << HorizontalChromaUpsample{0} << VerticalChromaUpsample{0} << HorizontalChromaUpsample{2} << VerticalChromaUpsample{2};
    s.filters(half, true, 2).upsample<2>(nullptr, {0, 1, 2}).noise(3) << YcbcrToRgbStage{0};
    s.convert({0, 1, 2}, DataFormat::u16()) << save4({0, 1, 2}, 0, 3, 16);
    out.push_back(List{"ycbcr_u16", false, 6, {1000, 700}, 1, 8, half, s});
  }
  {  // the planar f32 save
    Stages s;
    s.filters(full, true, 3) << save4({0, 1, 2}, 0, 3, 32);
    out.push_back(List{"planar_f32", false, 3, {1000, 700}, 0, 8, full, s});
  }
  {  // blending + extend in front of the four-argument tail
    Stages s;
    s.filters(full, true, 0) << XybStage{0, xyb()} << FromLinearStage{0, JXLH_TF_PQ, 4000.0f, kLum} << blend(0) << extend_of(blend(0));
    s.convert({0, 1, 2}, DataFormat::u8()) << save4({0, 1, 2}, 0, 4, 8);
    out.push_back(List{"blend_u8", false, 3, {1000, 700}, 0, 8, full, s});
  }
  {  // two extra channels with everything the device path serves
    Stages s;
    s << ConvertModularToF32Stage{3, 16} << ConvertModularToF32Stage{4, 8};
    s.filters(half, true, 2).upsample<4>(kTables[1], {4}) << dict(2) << segs();
    s.upsample<2>(kTables[0], {0, 1, 2, 3}).noise(5) << XybStage{0, some_xyb()} << FromLinearStage{0, JXLH_TF_SRGB, 0.0f, kLum}
                                                      << blend(2) << extend_of(blend(2)) << SpotColorStage{0, {0.1f, 0.2f, 0.3f, 0.4f}}
                                                      << SpotColorStage{1, {1.0f, 0.0f, 0.0f, 0.5f}} << PremultiplyAlphaStage{0, 3, 3};
    s.convert({0, 1, 2, 3}, DataFormat::u8()) << save6({0, 1, 2, 3}, 6, 0, ColorType::kRgba, DataFormat::u8(), false);
    s.convert({3}, DataFormat::u8()) << save6({3}, 6, 1, ColorType::kGrayscale, DataFormat::u8(), false);
    s.convert({4}, DataFormat::u16(12)) << save6({4}, 6, 2, ColorType::kGrayscale, DataFormat::u16(12), false);
    out.push_back(List{"extra_full", false, 8, {1000, 700}, 1, 8, half, s});
  }
  // the six-argument save's forms: `num_ec` 16-bit extra channels, Gaborish, XYB + a transfer function, then `tail`
  auto six = [&](const char* name, int num_ec, uint32_t tf, auto tail) {
    Stages s;
    for (int i = 0; i < num_ec; i++) s << ConvertModularToF32Stage{3 + i, 16};
    s.filters(full, true, 0) << XybStage{0, xyb()} << FromLinearStage{0, tf, tf == JXLH_TF_PQ ? 10000.0f : 0.0f, kLum};
    tail(s);
    out.push_back(List{name, false, (size_t)(3 + num_ec), {1000, 700}, 0, 8, full, s});
  };
  six("bgra_premultiplied", 1, JXLH_TF_SRGB, [](Stages& s) {
    s << SpotColorStage{0, {0.1f, 0.2f, 0.3f, 0.4f}} << PremultiplyAlphaStage{0, 3, 3};
    s.convert({0, 1, 2, 3}, DataFormat::u8()) << save6({0, 1, 2, 3}, 1, 0, ColorType::kBgra, DataFormat::u8(), false);
  });
  six("gray_alpha", 2, JXLH_TF_SRGB, [](Stages& s) {
    s << PremultiplyAlphaStage{0, 1, 4};
    s.convert({0, 4}, DataFormat::u16(16, true)) << save6({0, 4}, 1, 0, ColorType::kGrayscaleAlpha, DataFormat::u16(16, true), false);
  });
  six("gray_spot", 1, JXLH_TF_SRGB, [](Stages& s) {
    s << SpotColorStage{0, {0.5f, 0.6f, 0.7f, 0.8f}};
    s.convert({0}, DataFormat::u8()) << save6({0}, 4, 0, ColorType::kGrayscale, DataFormat::u8(), false);
  });
  six("fill_opaque_alpha", 0, JXLH_TF_SRGB, [](Stages& s) {
    s.convert({0, 1, 2}, DataFormat::u8()) << save6({0, 1, 2}, 1, 0, ColorType::kRgba, DataFormat::u8(), true);
  });
  six("f16_clamp", 0, JXLH_TF_PQ, [](Stages& s) {
    s.convert({0, 1, 2}, DataFormat::f16(), true, 0.0f, 1.0f) << save6({0, 1, 2}, 1, 0, ColorType::kRgb, DataFormat::f16(), false);
  });
  six("u16_10bit", 0, JXLH_TF_SRGB, [](Stages& s) {
    s.convert({0, 1, 2}, DataFormat::u16(10)) << save6({0, 1, 2}, 8, 0, ColorType::kBgr, DataFormat::u16(10), false);
  });
  six("f32_big_endian", 3, JXLH_TF_SRGB, [](Stages& s) {
    s << SpotColorStage{0, {0.1f, 0.2f, 0.3f, 0.4f}} << SpotColorStage{2, {0.5f, 0.6f, 0.7f, 0.8f}}
      << save6({0, 1, 2}, 3, 0, ColorType::kRgb, DataFormat::f32(true), false);
  });
  six("eight_spots", 2, JXLH_TF_SRGB, [](Stages& s) {  // as many spot colour stages as a save descriptor holds
    for (int i = 0; i < JXLH_MAX_EXTRA_CHANNELS; i++) s << SpotColorStage{i & 1, {0.1f * (float)i, 0.2f, 0.3f, 0.4f}};
    s.convert({0, 1, 2}, DataFormat::u8()) << save6({0, 1, 2}, 1, 0, ColorType::kRgb, DataFormat::u8(), false);
  });
  // Modular lists on caller-held planes (build_modular): the I32 -> U8 special case, to-f32 with Gaborish + EPF1
  {
    Stages s;
    s.modular(4).convert({0, 1, 2}, DataFormat::u8()) << save4({0, 1, 2}, 0, 3, 8);
    out.push_back(List{"modular_i32_u8", false, 3, {1000, 700}, 0, 8, full, s});
  }
  jxlh_frame_params pm = full;
  pm.epf_sigma_for_modular = 1.5f;
  {
    Stages s;
    s.modular(12).filters(pm, true, 1) << save4({0, 1, 2}, 0, 3, 32);
    out.push_back(List{"modular_f32_filters", false, 3, {1000, 700}, 0, 8, pm, s});
  }
  {
    Stages s;
    s << ConvertModularXYBToF32Stage{0, {0.01f, 0.02f, 0.03f}};
    s.filters(pm, true, 1) << save4({0, 1, 2}, 0, 3, 32);
    out.push_back(List{"modular_xyb_filters", false, 3, {1000, 700}, 0, 8, pm, s});
  }
  // Modular frames of the context (build_modular_frame): the reference's full list, integer form (patches and splines,
  // the extra channels upsampled with the frame) and XYB form (splines only, one extra channel with its own factor)
  for (const bool xyb_form : {false, true}) {
    Stages s;
    if (xyb_form) s << ConvertModularXYBToF32Stage{0, {0.25f, 0.5f, 0.125f}};
    else s.modular(12);
    s << ConvertModularToF32Stage{3, 16} << ConvertModularToF32Stage{4, 8};
    if (!xyb_form)
      s << HorizontalChromaUpsample{0} << VerticalChromaUpsample{0} << HorizontalChromaUpsample{2} << VerticalChromaUpsample{2};
    s.filters(half, true, 1);
    if (xyb_form) s.upsample<2>(nullptr, {3});
    else s << dict(2);
    s << segs();
    s.upsample<2>(nullptr, {0, 1, 2});
    if (!xyb_form) s.upsample<2>(nullptr, {3});
    s.upsample<2>(nullptr, {4}).noise(5) << XybStage{0, jxlh_xyb_params{}} << FromLinearStage{0, JXLH_TF_SRGB, 0.0f, kLum} << blend(2)
                                          << extend_of(blend(2)) << SpotColorStage{1, {1.0f, 0.5f, 0.25f, 0.75f}}
                                          << PremultiplyAlphaStage{0, 3, 3};
    s.convert({0, 1, 2, 3}, DataFormat::u8()) << save6({0, 1, 2, 3}, 6, 0, ColorType::kRgba, DataFormat::u8(), false);
    out.push_back(List{xyb_form ? "modular_frame_xyb" : "modular_frame_int", true, 8, {1000, 700}, 1, 8, half, s});
  }
  {  // ... and a plain one: conversions, an alpha channel, filters, RGBA8
    Stages s;
    s.modular(8) << ConvertModularToF32Stage{3, 8};
    s.filters(full, true, 1).convert({0, 1, 2, 3}, DataFormat::u8()) << save6({0, 1, 2, 3}, 1, 0, ColorType::kRgba, DataFormat::u8(), false);
    out.push_back(List{"modular_frame_plain", true, 4, {1000, 700}, 0, 8, full, s});
  }
  return out;
}

// ---------------------------------------------------------------------------------------------------------------
// Per-field edits of one stage: each returned stage differs from `s` in one field
using Edits = std::vector<std::pair<std::string, Stage>>;

inline std::vector<int> channel_values(const List& l) {
  return {-1, 0, 3, (int)l.num_channels, 3 + JXLH_MAX_EXTRA_CHANNELS};
}
template <class S, class T, class V>
void edit(Edits& out, const S& s, T S::*field, V value, const char* what) {
  if (s.*field == (T)value) return;
  S e = s;
  e.*field = (T)value;
  out.emplace_back(std::string(what) + "=" + std::to_string((long long)value), Stage{e});
}
template <class S, class F>
void edit_with(Edits& out, const S& s, const char* what, F f) {
  S e = s;
  f(e);
  out.emplace_back(what, Stage{e});
}
template <class S>
void edit_channel(Edits& out, const S& s, int S::*field, const List& l, const char* what) {
  for (int c : channel_values(l)) edit(out, s, field, c, what);
}
template <class S>
void edit_depth(Edits& out, const S& s, std::initializer_list<int> depths) {
  for (int d : depths) edit(out, s, &S::bit_depth, d, "bit_depth");
}

template <class S>
void edits_of(Edits& out, const S& s, const List& l) {
  if constexpr (is_one_of<S, HorizontalChromaUpsample, VerticalChromaUpsample, GaborishStage, ConvolveNoiseStage, Upsample2x,
                          Upsample4x, Upsample8x, ConvertF32ToU8Stage, ConvertF32ToU16Stage, ConvertF32ToF16Stage,
                          ConvertModularToF32Stage>)
    edit_channel(out, s, &S::channel, l, "channel");
  if constexpr (is_one_of<S, AddNoiseStage, XybStage, YcbcrToRgbStage, FromLinearStage, ConvertModularXYBToF32Stage>)
    edit_channel(out, s, &S::first_channel, l, "first_channel");
  if constexpr (is_one_of<S, Upsample2x, Upsample4x, Upsample8x>)  // a second weight table for the factor
    edit_with(out, s, "weights", [&](S& e) { e.weights = s.weights == kTables[1] ? kTables[2] : kTables[1]; });
  if constexpr (std::is_same_v<S, Epf1Stage>) edit_with(out, s, "sigma_scale", [](S& e) { e.sigma_scale = 0.5f; });
  if constexpr (std::is_same_v<S, FromLinearStage>) edit(out, s, &S::transfer, JXLH_TF_GAMMA + 1, "transfer");
  if constexpr (std::is_same_v<S, ConvertF32ToU8Stage>) edit_depth(out, s, {0, 5, 9, 32});
  if constexpr (std::is_same_v<S, ConvertF32ToU16Stage>) edit_depth(out, s, {0, 5, 17, 32});
  if constexpr (std::is_same_v<S, ConvertModularToF32Stage>) edit_depth(out, s, {0, 5, 32});
  if constexpr (std::is_same_v<S, ConvertF32ToF16Stage>) {
    edit_with(out, s, "clamp min > max", [](S& e) { e.clamp = true, e.clamp_min = 1.0f, e.clamp_max = 0.0f; });
    edit_with(out, s, "clamp NaN", [](S& e) { e.clamp = true, e.clamp_min = std::nanf(""), e.clamp_max = 1.0f; });
    edit_with(out, s, "clamp other", [](S& e) { e.clamp = true, e.clamp_min = 0.0f, e.clamp_max = 0.5f; });
  }
  if constexpr (std::is_same_v<S, PatchesStage>) {
    edit_with(out, s, "ec_flags longer", [](S& e) { e.ec_flags.push_back(0); });
    edit_with(out, s, "blendings longer", [](S& e) { e.blendings.push_back(jxlh_patch_blending{JXLH_PATCH_ADD, 0, 0}); });
  }
  if constexpr (is_one_of<S, BlendingStage, ExtendToImageDimensionsStage>) {  // the pair built from different headers
    edit(out, s, &S::x0, s.x0 + 1, "x0");
    edit(out, s, &S::y0, s.y0 + 1, "y0");
    edit(out, s, &S::image_w, s.image_w + 1, "image_w");
    edit(out, s, &S::image_h, s.image_h + 1, "image_h");
    edit_with(out, s, "blending_info.mode", [](S& e) { e.blending_info.mode ^= 1; });
    edit_with(out, s, "blending_info.clamp", [](S& e) { e.blending_info.clamp ^= 1; });
    edit_with(out, s, "ec_blending_info longer", [](S& e) { e.ec_blending_info.push_back(jxlh_blending_info{}); });
    if (!s.ec_blending_info.empty()) {
      edit_with(out, s, "ec_blending_info shorter", [](S& e) { e.ec_blending_info.pop_back(); });
      edit_with(out, s, "ec_blending_info[0].source", [](S& e) { e.ec_blending_info[0].source ^= 1; });
    }
  }
  if constexpr (std::is_same_v<S, BlendingStage>) {
    edit_with(out, s, "ec_flags longer", [](S& e) { e.ec_flags.push_back(0); });
    if (!s.ec_flags.empty()) edit_with(out, s, "ec_flags shorter", [](S& e) { e.ec_flags.pop_back(); });
  }
  if constexpr (std::is_same_v<S, SpotColorStage>) edit_channel(out, s, &S::ec, l, "ec");
  if constexpr (std::is_same_v<S, PremultiplyAlphaStage>) {
    edit_channel(out, s, &S::alpha_channel, l, "alpha_channel");
    edit(out, s, &S::first_color_channel, 1, "first_color_channel");
    for (int n : {1, 2, 3}) edit(out, s, &S::num_color_channels, n, "num_color_channels");
  }
  if constexpr (std::is_same_v<S, SaveStage>) {
    for (size_t k = 0; k < s.channels.size(); k++)
      for (int c : channel_values(l))
        if (c != s.channels[k])
          edit_with(out, s, ("channels[" + std::to_string(k) + "]=" + std::to_string(c)).c_str(), [&](S& e) { e.channels[k] = c; });
    edit_with(out, s, "channels shorter", [](S& e) { e.channels.pop_back(); });
    for (int b : {-1, 1}) edit(out, s, &S::output_buffer_index, s.output_buffer_index + b, "output_buffer_index");
    if (!s.full) {
      for (int n : {2, 3, 4, 5}) edit(out, s, &S::color_channels, n, "color_channels");
      for (int n : {0, 8, 16, 32}) edit(out, s, &S::bits, n, "bits");
    } else {
      for (int o : {0, 9}) edit(out, s, &S::orientation, o, "orientation");
      for (uint32_t f = 0; f <= 4; f++)
        if (f != s.data_format.format) edit_with(out, s, ("format=" + std::to_string(f)).c_str(), [&](S& e) { e.data_format.format = f; });
      const uint32_t above = s.data_format.format == JXLH_SAVE_U8 ? 9 : 17;
      for (uint32_t d : {0u, 5u, above, 32u})
        if (d != s.data_format.bit_depth)
          edit_with(out, s, ("bit_depth=" + std::to_string(d)).c_str(), [&](S& e) { e.data_format.bit_depth = d; });
      edit_with(out, s, "big_endian", [](S& e) { e.data_format.big_endian = !e.data_format.big_endian; });
      for (int ct = 0; ct < 6; ct++)
        if ((ColorType)ct != s.color_type)
          edit_with(out, s, ("color_type=" + std::to_string(ct)).c_str(), [&](S& e) { e.color_type = (ColorType)ct; });
      edit_with(out, s, "fill_opaque_alpha", [](S& e) { e.fill_opaque_alpha = !e.fill_opaque_alpha; });
    }
  }
}
inline Edits edits_of(const Stage& s, const List& l) {
  Edits out;
  std::visit([&](const auto& st) { edits_of(out, st, l); }, s);
  return out;
}

// ---------------------------------------------------------------------------------------------------------------
// The enumeration.  emit(family, list, what): `what` names the mutation (base list, positions, field).
using Emit = std::function<void(const char* family, const List& list, const std::string& what)>;

inline List without(const List& l, size_t i) {
  List m = l;
  m.stages.erase(m.stages.begin() + (long)i);
  return m;
}
inline std::string at(size_t i) { return std::to_string(i); }

inline void mutations_of(const List& l, const Emit& emit) {
  const size_t n = l.stages.size();
  const std::string name = l.name + " ";
  emit("base", l, l.name);
  for (size_t i = 0; i < n; i++) emit("delete", without(l, i), name + at(i));
  for (size_t i = 0; i < n; i++) {
    List m = l;
    m.stages.insert(m.stages.begin() + (long)i, l.stages[i]);
    emit("duplicate", m, name + at(i) + " beside");
    m = l;
    m.stages.push_back(l.stages[i]);
    emit("duplicate", m, name + at(i) + " at the end");
  }
  for (size_t i = 0; i + 1 < n; i++) {
    List m = l;
    std::swap(m.stages[i], m.stages[i + 1]);
    emit("swap", m, name + at(i));
  }
  for (size_t i = 0; i < n; i++)
    for (size_t j = 0; j < n; j++) {
      if (i == j) continue;
      List m = without(l, i);
      m.stages.insert(m.stages.begin() + (long)j, l.stages[i]);
      emit("move", m, name + at(i) + " to " + at(j));
    }
  for (size_t i = 0; i < n; i++)
    for (size_t j = i + 1; j < n; j++) emit("pair", without(without(l, j), i), name + at(i) + " and " + at(j));
  // a stage that does not belong to the list, at every position
  const std::pair<const char*, Stage> foreign[] = {
      {"CpuOnlyStage", CpuOnlyStage{"patches"}},
      {"add_extend_stage()", CpuOnlyStage{kBareExtend}},
      {"four-argument save", save4({0, 1, 2}, 0, 3, 8)},
      {"six-argument save", save6({0, 1, 2}, 1, 0, ColorType::kRgb, DataFormat::f32(), false)},
      {"HorizontalChromaUpsample", HorizontalChromaUpsample{0}},
      {"ConvertModularXYBToF32Stage", ConvertModularXYBToF32Stage{0, {0.01f, 0.02f, 0.03f}}},
      {"XybStage", XybStage{0, some_xyb()}},
  };
  for (const auto& f : foreign)
    for (size_t i = 0; i <= n; i++) {
      List m = l;
      m.stages.insert(m.stages.begin() + (long)i, f.second);
      emit("insert", m, name + f.first + " at " + at(i));
    }
  for (size_t i = 0; i < n; i++)
    for (const auto& e : edits_of(l.stages[i], l)) {
      List m = l;
      m.stages[i] = e.second;
      emit("field", m, name + at(i) + " " + e.first);
      for (size_t k = 0; k < n; k++)
        if (k != i) emit("field+delete", without(m, k), name + at(i) + " " + e.first + ", without " + at(k));
    }
  // the builder's own arguments
  size_t num_ec = 0;
  for (const Stage& s : l.stages)
    if (const auto* m = std::get_if<ConvertModularToF32Stage>(&s)) num_ec += m->channel > 2;
  for (size_t nc : {(size_t)2, (size_t)3, 3 + num_ec}) {
    List m = l;
    m.num_channels = nc;
    emit("arguments", m, name + "num_channels=" + at(nc));
  }
  const std::pair<size_t, size_t> sizes[] = {{l.size.first + 1, l.size.second}, {l.size.first - 1, l.size.second},
                                             {l.size.first, l.size.second + 1}, {l.size.first, l.size.second - 1},
                                             {0, l.size.second},                {l.size.first, 0}};
  for (const auto& sz : sizes) {
    List m = l;
    m.size = sz;
    emit("arguments", m, name + "size=" + at(sz.first) + "x" + at(sz.second));
  }
  for (size_t shift = 0; shift <= 3; shift++)
    for (size_t lg : {(size_t)7, (size_t)8, (size_t)9, 8 + shift}) {
      List m = l;
      m.shift = shift;
      m.log_group = lg;
      emit("arguments", m, name + "downsampling_shift=" + at(shift) + " log_group_size=" + at(lg));
    }
}
inline void for_each_list(const Emit& emit) {
  for (const List& l : base_lists()) mutations_of(l, emit);
}
}  // namespace lowering_corpus
