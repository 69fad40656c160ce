// C++ mirror of the reference's stage traits and pipeline builder for the path this library replaces
// (jxl/src/render/mod.rs:52-114 RenderPipelineInOutStage / RenderPipelineInPlaceStage,
// jxl/src/render/builder.rs:19-120 RenderPipelineBuilder, and the stage list of
// Frame::build_render_pipeline, jxl/src/frame/render.rs:526-903), and the LOWERING of such a list.
//
// The builder takes the stages under the reference's names, with the reference's constructor arguments, in the
// reference's order, checks that the list is one the device path implements (anything else is JXLH_ERR_UNSUPPORTED
// naming the stage: that stage list stays on the CPU pipeline), and lowers it onto jxlh_frame_params, jxlh_output_desc,
// jxlh_blend_desc and one jxlh_save_desc per output buffer: a LoweredPipeline.  BORDER / SHIFT of every stage are the
// reference's constants, and the lowering reports the accumulated input border the way RenderPipelineShared does
// (render/internal.rs) -- 4 pixels for Gaborish + EPF1 + EPF2, jxl/src/render/mod.rs:28-36 -- which is the halo the
// fused kernel stages and the sharded path exchanges.
//
// Host-only: nothing here calls the library (Error formats a status).  detail::Lowering walks the list with one handler
// per stage type; jxl_hip_pipeline.hpp runs the result on a context.  tests/cpp/lowering_corpus.h enumerates stage lists
// and tests/golden/pipeline_lowering.json pins, for each, every lowered field or the status and message it fails with.
#pragma once
#include <array>
#include <cstdint>
#include <memory>
#include <string>
#include <utility>
#include <variant>
#include <vector>

#include "jxl_hip.hpp"

namespace jxlh {

// ---------------------------------------------------------------------------------------------------------------
// Stage descriptors.  Names, constructor argument order and the BORDER / SHIFT constants follow
// jxl/src/render/stages/*.rs; `Display` strings are the reference's (they end up in error messages).
struct Border {
  uint8_t x, y;
};

struct HorizontalChromaUpsample {  // chroma_upsample.rs:15, :67-68
  int channel;
  static constexpr Border BORDER{1, 0}, SHIFT{1, 0};
  std::string display() const { return "chroma upsample of channel " + std::to_string(channel) + ", horizontally"; }
  bool uses_channel(int c) const { return c == channel; }
};
struct VerticalChromaUpsample {  // chroma_upsample.rs:93, :154-155
  int channel;
  static constexpr Border BORDER{0, 1}, SHIFT{0, 1};
  std::string display() const { return "chroma upsample of channel " + std::to_string(channel) + ", vertically"; }
  bool uses_channel(int c) const { return c == channel; }
};
struct GaborishStage {  // gaborish.rs:20, :94-95
  int channel;
  float weight1, weight2;
  static constexpr Border BORDER{1, 1}, SHIFT{0, 0};
  std::string display() const { return "Gaborish filter for channel " + std::to_string(channel); }
  bool uses_channel(int c) const { return c == channel; }
};
template <int PASS>
struct EpfStage {  // epf/epf{0,1,2}.rs:35-48; the SigmaSource argument is the frame's own (jxlh_frame_run builds it)
  float sigma_scale, border_sad_mul;
  std::array<float, 3> channel_scale;
  static constexpr Border BORDER{PASS == 0 ? 3 : PASS == 1 ? 2 : 1, PASS == 0 ? 3 : PASS == 1 ? 2 : 1}, SHIFT{0, 0};
  std::string display() const {
    return "EPF stage " + std::to_string(PASS) + " with sigma scale: " + std::to_string(sigma_scale) +
           ", border_sad_mul: " + std::to_string(border_sad_mul);
  }
  bool uses_channel(int c) const { return c < 3; }
};
using Epf0Stage = EpfStage<0>;
using Epf1Stage = EpfStage<1>;
using Epf2Stage = EpfStage<2>;
template <int N>
struct Upsample {  // upsample.rs:22, :396-397.  weights: CustomTransformData::weights{2,4,8} or nullptr = defaults
  const float* weights;
  int channel;
  static constexpr Border BORDER{2, 2}, SHIFT{N == 2 ? 1 : N == 4 ? 2 : 3, N == 2 ? 1 : N == 4 ? 2 : 3};
  std::string display() const {
    return std::to_string(N) + "x" + std::to_string(N) + " upsampling of channel " + std::to_string(channel);
  }
  bool uses_channel(int c) const { return c == channel; }
};
using Upsample2x = Upsample<2>;
using Upsample4x = Upsample<4>;
using Upsample8x = Upsample<8>;
struct ConvolveNoiseStage {  // noise.rs:22, :87-88
  int channel;
  static constexpr Border BORDER{2, 2}, SHIFT{0, 0};
  std::string display() const { return "convolve noise for channel " + std::to_string(channel); }
  bool uses_channel(int c) const { return c == channel; }
};
struct AddNoiseStage {  // noise.rs:115-128 (in place).  lut = Noise::lut, ytox_lf / ytob_lf = ColorCorrelationParams
  std::array<float, 8> lut;
  int32_t ytox_lf, ytob_lf;
  int first_channel;
  std::string display() const {
    return "add noise for channels [" + std::to_string(first_channel) + "," + std::to_string(first_channel + 1) + "," +
           std::to_string(first_channel + 2) + "]";
  }
  bool uses_channel(int c) const { return c < 3 || (c >= first_channel && c < first_channel + 3); }
};
struct XybStage {  // xyb.rs:173 (in place); params = XybParams::new(opsin, intensity_target), xyb.rs:147-163
  int first_channel;
  jxlh_xyb_params params;
  std::string display() const { return "XYB to linear for channel [0,1,2]"; }
  bool uses_channel(int c) const { return c >= first_channel && c < first_channel + 3; }
};
struct YcbcrToRgbStage {  // ycbcr.rs:16 (in place)
  int first_channel;
  std::string display() const { return "YCbCr to RGB for channel [0,1,2]"; }
  bool uses_channel(int c) const { return c >= first_channel && c < first_channel + 3; }
};
struct FromLinearStage {  // from_linear.rs:20 (in place); transfer = JXLH_TF_*, param as jxlh_output_desc::tf_param
  int first_channel;
  uint32_t transfer;
  float param;
  std::array<float, 3> hlg_luminance_rgb;
  std::string display() const { return "Apply transfer function " + std::to_string(transfer) + " to channel [0,1,2]"; }
  bool uses_channel(int c) const { return c >= first_channel && c < first_channel + 3; }
};
struct ConvertF32ToU8Stage {  // convert.rs:555, :612-613
  int channel;
  uint8_t bit_depth;
  static constexpr Border BORDER{0, 0}, SHIFT{0, 0};
  std::string display() const {
    return "convert F32 to U8 in channel " + std::to_string(channel) + " with bit depth " + std::to_string(bit_depth);
  }
  bool uses_channel(int c) const { return c == channel; }
};
struct ConvertF32ToU16Stage {  // convert.rs:724, :767-768
  int channel;
  uint8_t bit_depth;
  static constexpr Border BORDER{0, 0}, SHIFT{0, 0};
  std::string display() const {
    return "convert F32 to U16 in channel " + std::to_string(channel) + " with bit depth " + std::to_string(bit_depth);
  }
  bool uses_channel(int c) const { return c == channel; }
};
struct ConvertModularToF32Stage {  // convert.rs:351, :512-513 (bit_depth: integer samples of that many bits)
  int channel;
  uint8_t bit_depth;
  static constexpr Border BORDER{0, 0}, SHIFT{0, 0};
  std::string display() const {
    return "convert modular data to F32 in channel " + std::to_string(channel) + " with bit depth " + std::to_string(bit_depth);
  }
  bool uses_channel(int c) const { return c == channel; }
};
struct ConvertModularXYBToF32Stage {  // convert.rs:284, :309-310; quant_factors = LfQuantFactors::quant_factors (X, Y, B)
  int first_channel;
  std::array<float, 3> quant_factors;
  static constexpr Border BORDER{0, 0}, SHIFT{0, 0};
  std::string display() const { return "convert modular xyb data to F32 in channels 0..3"; }
  bool uses_channel(int c) const { return c >= first_channel && c < first_channel + 3; }
};
// PatchesStage (render/stages/patches.rs, added at frame/render.rs:644-650): the frame's dictionary flattened as
// jxlh_frame_set_patches takes it -- blendings = patches.size() * (1 + ec_flags.size()) -- and the alpha flags of
// the extra channels.  In place on every channel; the reference frames it reads are the context's slots.
struct PatchesStage {
  std::vector<jxlh_patch> patches;
  std::vector<jxlh_patch_blending> blendings;
  std::vector<uint32_t> ec_flags;
  static constexpr Border BORDER{0, 0}, SHIFT{0, 0};
  std::string display() const { return "patches"; }
  bool uses_channel(int) const { return true; }
};
// SplinesStage (render/stages/splines.rs, added at frame/render.rs:652-653 when the frame has splines): the draw cache's
// segments (Splines::initialize_draw_cache; VarDctFrame::decode_splines builds them from the bitstream's form).  In
// place on the three colour channels.
struct SplinesStage {
  std::vector<jxlh_spline_segment> segments;
  static constexpr Border BORDER{0, 0}, SHIFT{0, 0};
  std::string display() const { return "splines"; }
  bool uses_channel(int c) const { return c < 3; }
};
// BlendingStage (render/stages/blending.rs:17-27, added at frame/render.rs:765-771 when needs_blending()): the fields
// BlendingStage::new takes from the frame and file headers that matter on the device -- the reference frames it reads
// are the context's slots.  In place on the colour and extra channels.
struct BlendingStage {
  int32_t x0, y0;                                    // frame_origin
  uint32_t image_w, image_h;                         // image_size
  jxlh_blending_info blending_info;
  std::vector<jxlh_blending_info> ec_blending_info;  // one per extra channel
  std::vector<uint32_t> ec_flags;                    // JXLH_EC_* of each extra channel (extra_channels)
  static constexpr Border BORDER{0, 0}, SHIFT{0, 0};
  std::string display() const { return "blending"; }
  bool uses_channel(int c) const { return c < 3 + (int)ec_blending_info.size(); }
};
// ExtendToImageDimensionsStage (render/stages/extend.rs:22-50, add_extend_stage at frame/render.rs:766-771): built from
// the same headers as the BlendingStage in front of it
struct ExtendToImageDimensionsStage {
  int32_t x0, y0;
  uint32_t image_w, image_h;
  jxlh_blending_info blending_info;
  std::vector<jxlh_blending_info> ec_blending_info;
  std::string display() const { return "extend-to-image-dims"; }
  bool uses_channel(int) const { return true; }
};
// SpotColorStage::new(spot_c_offset, spot_color) (spot.rs:24-29, added at frame/render.rs:793-806): in place on the
// colour channels, reading extra channel `ec`
struct SpotColorStage {
  int ec;
  std::array<float, 4> rgba;
  std::string display() const { return "spot color stage for channel " + std::to_string(3 + ec); }
  bool uses_channel(int c) const { return c < 3 || c == 3 + ec; }
};
// PremultiplyAlphaStage::new(first_color_channel, num_color_channels, alpha_channel) (premultiply_alpha.rs:33-45)
struct PremultiplyAlphaStage {
  int first_color_channel, num_color_channels, alpha_channel;
  std::string display() const {
    return "premultiply alpha stage for color channels " + std::to_string(first_color_channel) + "-" +
           std::to_string(first_color_channel + num_color_channels - 1) + " with alpha channel " + std::to_string(alpha_channel);
  }
  bool uses_channel(int c) const {
    return (c >= first_color_channel && c < first_color_channel + num_color_channels) || c == alpha_channel;
  }
};
// ConvertF32ToF16Stage::new_with_clamp_range(channel, clamp_range) (convert.rs:796-811)
struct ConvertF32ToF16Stage {
  int channel;
  bool clamp = false;
  float clamp_min = 0.0f, clamp_max = 0.0f;
  static constexpr Border BORDER{0, 0}, SHIFT{0, 0};
  std::string display() const { return "convert F32 to F16 in channel " + std::to_string(channel); }
  bool uses_channel(int c) const { return c == channel; }
};
// JxlColorType / JxlDataFormat / Endianness (api/data_types.rs) and Orientation (headers/image_metadata.rs:85-96, the
// values 1..8 of the codestream) as the richer add_save_stage takes them
enum class ColorType { kGrayscale, kGrayscaleAlpha, kRgb, kRgba, kBgr, kBgra };
struct DataFormat {
  uint32_t format;     // JXLH_SAVE_*
  uint32_t bit_depth;  // U8 / U16
  bool big_endian;
  static DataFormat u8(uint32_t depth = 8) { return {JXLH_SAVE_U8, depth, false}; }
  static DataFormat u16(uint32_t depth = 16, bool be = false) { return {JXLH_SAVE_U16, depth, be}; }
  static DataFormat f16(bool be = false) { return {JXLH_SAVE_F16, 0, be}; }
  static DataFormat f32(bool be = false) { return {JXLH_SAVE_F32, 0, be}; }
};
// A stage of the reference this path does not run on the device (patches or splines by name ...): adding one makes
// build() fail with JXLH_ERR_UNSUPPORTED.
struct CpuOnlyStage {
  std::string name;
  std::string display() const { return name; }
  bool uses_channel(int) const { return true; }
};
// add_save_stage (builder.rs:87-105): channels, output buffer index, interleaved colour type and sample format
struct SaveStage {
  std::vector<int> channels;
  int output_buffer_index;
  uint32_t color_channels;  // 3 = RGB, 4 = RGBA (fill_opaque_alpha)
  uint32_t bits;            // 8, 16, or 32 = the f32 planes themselves (JxlDataFormat::F32)
  // the six-argument form of builder.rs:87-105 (`full`): the stage lowers to a jxlh_save_desc; color_channels / bits unused
  bool full = false;
  uint32_t orientation = 1;
  ColorType color_type = ColorType::kRgb;
  DataFormat data_format{JXLH_SAVE_U8, 8, false};
  bool fill_opaque_alpha = false;
  std::string display() const { return "save stage for buffer " + std::to_string(output_buffer_index); }
  bool uses_channel(int c) const {
    for (int ch : channels)
      if (ch == c) return true;
    return false;
  }
};

using Stage = std::variant<ConvertModularToF32Stage, ConvertModularXYBToF32Stage, HorizontalChromaUpsample, VerticalChromaUpsample, GaborishStage, Epf0Stage, Epf1Stage, Epf2Stage,
                           Upsample2x, Upsample4x, Upsample8x, ConvolveNoiseStage, AddNoiseStage, XybStage, YcbcrToRgbStage,
                           FromLinearStage, ConvertF32ToU8Stage, ConvertF32ToU16Stage, CpuOnlyStage, SaveStage, PatchesStage,
                           BlendingStage, ExtendToImageDimensionsStage, SpotColorStage, PremultiplyAlphaStage,
                           ConvertF32ToF16Stage, SplinesStage>;

inline std::string stage_display(const Stage& s) {
  return std::visit([](const auto& st) { return st.display(); }, s);
}

// ---------------------------------------------------------------------------------------------------------------
// What a stage list lowers to.
struct LoweredPipeline {
  jxlh_frame_params frame;     // the caller's base parameters with the stage-derived fields overwritten
  bool has_output = false;     // a colour / conversion tail was given: read through jxlh_frame_read_output
  jxlh_output_desc output{};
  const float* upsampling_weights = nullptr;
  const float* weights_by_factor[3] = {nullptr, nullptr, nullptr};  // 2x, 4x, 8x: the frame's and the extra channels'
  // Modular frames (Encoding::Modular: the list opens with the Modular -> f32 conversions, frame/render.rs:553-567)
  enum class Modular { kNone, kToF32, kXybToF32, kI32ToU8 } modular = Modular::kNone;
  uint32_t modular_bits = 0;                       // kToF32: bits per integer sample
  std::array<float, 3> modular_quant_factors{};    // kXybToF32
  int32_t i32_to_u8_multiplier = 0, i32_to_u8_max = 0;  // kI32ToU8: ConvertI32ToU8Stage::new(c, mult, max), builder.rs:152-170
  // lower_modular_frame(): what jxlh_frame_set_modular_channels takes as sample_format (frame.flags then carries
  // JXLH_FRAME_MODULAR, and frame.lf_quant_factors the XYB conversion's factors)
  uint32_t modular_sample_format = 0;
  Border input_border{0, 0};   // accumulated BORDER of the in-out stages before any upsampling, in input pixels
  // Extra channels (pipeline channels 3..): ConvertModularToF32Stage::new(3 + ec, ec_bit_depth) (frame/render.rs:564-567)
  // and the channel's own Upsample{2,4,8}x::new(transform_data, 3 + ec) (frame/render.rs:624-637, or with the colour
  // channels when every ec_upsampling equals the frame's, :655-668).  bits == 0: the list does not name the channel.
  struct Extra {
    uint32_t bits = 0, upsampling = 1;
  };
  std::array<Extra, JXLH_MAX_EXTRA_CHANNELS> extra{};
  // PatchesStage: the dictionary build() hands to jxlh_frame_set_patches
  bool has_patches = false;
  PatchesStage patches;
  // SplinesStage: the segments build() hands to jxlh_frame_set_splines
  bool has_splines = false;
  SplinesStage splines;
  // BlendingStage + ExtendToImageDimensionsStage: do_render() ends in jxlh_frame_blend(blend, blend_colour).  The colour
  // stage of the list runs inside that call (blend_colour), so `output.color` is JXLH_COLOR_NONE
  bool has_blend = false;
  jxlh_blend_desc blend{};
  jxlh_output_desc blend_colour{};
  // The save tail (six-argument save stages): saves[i] is output buffer i, behind the colour stage `output` names
  // (color / transfer / xyb / tf_param; JXLH_COLOR_NONE after a blend).  SpotColorStage and PremultiplyAlphaStage fold
  // into the save that carries colour channels; extra-channel saves carry neither.  GpuRenderPipeline::save(i, ...) runs
  // jxlh_frame_save with it.
  std::vector<jxlh_save_desc> saves;
  uint32_t out_w = 0, out_h = 0;  // what the save stages see: the frame's (upsampled) size, or the image's when blending
  std::vector<std::string> stages;  // Display strings, in order (diagnostics; what `info!("adding stage")` logs)
};

// ---------------------------------------------------------------------------------------------------------------
// The lowering: one walk over the list with a handler per stage type, then the whole-list checks of finish().
namespace detail {

[[noreturn]] inline void fail(jxlh_status st, const std::string& what) { throw Error(st, "RenderPipelineBuilder::build", what); }
[[noreturn]] inline void unsupported(const std::string& what) { fail(JXLH_ERR_UNSUPPORTED, what); }
[[noreturn]] inline void invalid(const std::string& what) { fail(JXLH_ERR_INVALID_ARGUMENT, what); }

class Lowering {
 public:
  // modular_frame: the list is a Modular frame's and the frame runs through jxlh_frame_run; otherwise a Modular list is
  // the caller-held-planes form, with its narrower stage set
  Lowering(size_t num_channels, std::pair<size_t, size_t> size, size_t downsampling_shift, size_t log_group_size,
           const jxlh_frame_params& base, bool modular_frame)
      : num_channels_((int)num_channels), size_(size), downsampling_shift_(downsampling_shift), modular_frame_(modular_frame) {
    lp_.frame = base;
    if (log_group_size != 8 + downsampling_shift && log_group_size != 8)
      unsupported("group dimension other than 256 (FrameHeader::log_group_dim)");
    if (num_channels < 3) invalid("fewer than three channels");
    // stage-derived fields start from "no stage"
    p_.gab = p_.epf_iters = p_.noise = 0;
    p_.upsampling = 1;
    for (int c = 0; c < 3; c++) p_.hshift[c] = p_.vshift[c] = 0;
    lp_.output.color = JXLH_COLOR_NONE;
    lp_.output.transfer = JXLH_TF_LINEAR;
    lp_.output.bits = 0;
    lp_.output.channels = 3;
  }

  LoweredPipeline run(const std::vector<Stage>& stages) {
    // A list with a six-argument save stage is checked by the save tail's rules; a list without one goes through the
    // checks it always went through, with the statuses it always got.
    for (const Stage& s : stages)
      if (const auto* sv = std::get_if<SaveStage>(&s)) full_save_ |= sv->full;
    for (const Stage& s : stages) {
      name_ = stage_display(s);
      lp_.stages.push_back(name_);
      if (blend_.expect_extend && !std::holds_alternative<ExtendToImageDimensionsStage>(s))
        invalid(quoted() + " between the blending stage and the extend stage");
      if (blend_.seen && (std::holds_alternative<XybStage>(s) || std::holds_alternative<YcbcrToRgbStage>(s) ||
                          std::holds_alternative<FromLinearStage>(s)))
        invalid("blending / extend stage before the colour stage '" + name_ + "'");
      std::visit([this](const auto& st) { on(st); }, s);
    }
    finish();
    return std::move(lp_);
  }

 private:
  using Modular = LoweredPipeline::Modular;
  // The reference's order (frame/render.rs:568-790) as phases; a stage may only appear in a phase >= the current one.
  enum Phase { kModular, kChroma, kGab, kEpf0, kEpf1, kEpf2, kUpsample, kNoiseConvolve, kNoiseAdd, kColour, kTransfer, kConvert, kSave, kDone };

  // ---- the rules more than one handler applies
  std::string quoted() const { return "stage '" + name_ + "'"; }
  [[noreturn]] void out_of_order(jxlh_status st = JXLH_ERR_UNSUPPORTED) const {
    fail(st, quoted() + " out of the order of Frame::build_render_pipeline");
  }
  void enter(int ph) {
    if (ph < phase_) out_of_order();
    phase_ = ph;
  }
  // what the caller-held-planes form of a Modular list leaves to a stage hook
  void planes_use_hook(const std::string& what, const char* hook) const {
    if (!modular_frame_ && lp_.modular != Modular::kNone)
      unsupported(what + " on a Modular frame (jxlh_stage_" + hook + " on the planes instead)");
  }
  // the stages only a list with a six-argument save stage can express
  auto& full_tail() {
    if (!full_save_) unsupported(quoted() + " needs the save stage that carries colour type, data format and orientation");
    return tail_;
  }
  // frame/render.rs:765-806: spot colours, premultiplication and every conversion come behind blend / extend
  void in_front_of_save_tail() const {
    if (tail_.begun()) invalid(quoted() + " behind a spot colour, premultiply or conversion stage: they follow the blending and extend stages");
  }
  // weights_by_factor[n >> 2]: factor 2, 4, 8
  void one_table_per_factor(int n, const float* w) const {
    const float* seen = lp_.weights_by_factor[n >> 2];
    if (seen && seen != w) invalid("one weight table per upsampling factor (CustomTransformData)");
  }
  bool is_extra_channel(int ec) const { return ec >= 0 && ec < JXLH_MAX_EXTRA_CHANNELS && 3 + ec < num_channels_ && lp_.extra[ec].bits; }
  void add_border(Border b) {
    if (colour_.ups_seen != 0) return;  // in input pixels: the stages before any frame upsampling
    lp_.input_border.x = (uint8_t)(lp_.input_border.x + b.x);
    lp_.input_border.y = (uint8_t)(lp_.input_border.y + b.y);
  }

  // ---- one handler per stage type
  void on(const CpuOnlyStage&) { unsupported(quoted() + " is not part of the device path"); }

  void on(const BlendingStage& bl) {
    // the reference's position: behind the colour stage, in front of the conversions (frame/render.rs:754-779)
    if (blend_.seen) invalid("two blending stages");
    if (phase_ > kConvert || legacy_.convert_seen) invalid("blending stage behind the conversion / save stages");
    in_front_of_save_tail();
    planes_use_hook("blending", "blend");
    const size_t nec = bl.ec_blending_info.size();
    size_t named = 0;
    while (named < JXLH_MAX_EXTRA_CHANNELS && lp_.extra[named].bits) named++;
    if (nec > JXLH_MAX_EXTRA_CHANNELS || bl.ec_flags.size() != nec || nec != named)
      invalid("blending: one ec_blending_info and one flag word per extra channel of the list");
    blend_.seen = blend_.expect_extend = true;  // the extend stage follows at once (frame/render.rs:765-771)
    lp_.has_blend = true;
    lp_.blend = jxlh_blend_desc{};
    lp_.blend.x0 = bl.x0;
    lp_.blend.y0 = bl.y0;
    lp_.blend.image_w = bl.image_w;
    lp_.blend.image_h = bl.image_h;
    lp_.blend.color = bl.blending_info;
    lp_.blend.num_ec = (uint32_t)nec;
    for (size_t i = 0; i < nec; i++) {
      lp_.blend.ec[i] = bl.ec_blending_info[i];
      lp_.blend.ec_flags[i] = bl.ec_flags[i];
    }
    phase_ = kConvert;
  }
  void on(const ExtendToImageDimensionsStage& ex) {
    in_front_of_save_tail();
    if (!blend_.expect_extend) invalid(blend_.extend_seen ? "two extend stages" : "extend stage without a blending stage in front of it");
    auto same_info = [](const jxlh_blending_info& a, const jxlh_blending_info& b) {
      return a.mode == b.mode && a.alpha_channel == b.alpha_channel && a.clamp == b.clamp && a.source == b.source;
    };
    bool same = ex.x0 == lp_.blend.x0 && ex.y0 == lp_.blend.y0 && ex.image_w == lp_.blend.image_w &&
                ex.image_h == lp_.blend.image_h && same_info(ex.blending_info, lp_.blend.color) &&
                ex.ec_blending_info.size() == lp_.blend.num_ec;
    for (size_t i = 0; same && i < ex.ec_blending_info.size(); i++) same = same_info(ex.ec_blending_info[i], lp_.blend.ec[i]);
    if (!same) invalid("blending and extend stages built from different headers");
    blend_.expect_extend = false;
    blend_.extend_seen = true;
  }

  void on(const ConvertModularToF32Stage& m) {
    enter(kModular);
    if (m.bit_depth < 1 || m.bit_depth > 31) invalid("bit depth");
    if (m.channel > 2) {  // an extra channel: any frame encoding, after the colour conversions
      const int ec = m.channel - 3;
      if (ec >= JXLH_MAX_EXTRA_CHANNELS) unsupported("more extra channels than JXLH_MAX_EXTRA_CHANNELS");
      if (m.channel >= num_channels_ || lp_.extra[ec].bits || (ec > 0 && !lp_.extra[ec - 1].bits))
        invalid("Modular -> f32 conversion of extra channels: channels 3.. in order, once each");
      if (colour_.modular_seen != 0 && colour_.modular_seen != 3) invalid("extra channel conversion between the colour conversions");
      lp_.extra[ec].bits = m.bit_depth;
      return;
    }
    if (m.channel != colour_.modular_seen || lp_.modular == Modular::kXybToF32 || lp_.extra[0].bits)
      invalid("Modular -> f32 conversion: channels 0, 1, 2 in order, before the extra channels");
    if (colour_.modular_seen && m.bit_depth != lp_.modular_bits) unsupported("colour channels of different bit depths");
    lp_.modular = Modular::kToF32;
    lp_.modular_bits = m.bit_depth;
    colour_.modular_seen++;
  }
  void on(const ConvertModularXYBToF32Stage& mx) {
    enter(kModular);
    if (mx.first_channel != 0 || lp_.modular != Modular::kNone) invalid("one XYB conversion on channels 0..2");
    lp_.modular = Modular::kXybToF32;
    lp_.modular_quant_factors = mx.quant_factors;
    colour_.modular_seen = 3;
  }

  void chroma_upsample(int channel, uint32_t (&shift)[3]) {
    enter(kChroma);
    if (channel < 0 || channel > 2) invalid("chroma upsampling of a non-colour channel");
    shift[channel] = 1;
  }
  void on(const HorizontalChromaUpsample& h) { chroma_upsample(h.channel, p_.hshift); }
  void on(const VerticalChromaUpsample& v) { chroma_upsample(v.channel, p_.vshift); }

  void on(const GaborishStage& g) {
    enter(kGab);
    if (g.channel < 0 || g.channel > 2 || colour_.gab_seen[g.channel]) invalid("Gaborish: one stage per colour channel");
    colour_.gab_seen[g.channel] = true;
    p_.gab = 1;
    p_.gab_w1[g.channel] = g.weight1;
    p_.gab_w2[g.channel] = g.weight2;
    if (g.channel == 0) add_border(GaborishStage::BORDER);
  }
  void on(const Epf0Stage& e0) {
    enter(kEpf0);
    p_.epf_pass0_sigma_scale = e0.sigma_scale;
    p_.epf_border_sad_mul = e0.border_sad_mul;
    for (int c = 0; c < 3; c++) p_.epf_channel_scale[c] = e0.channel_scale[c];
    p_.epf_iters = 3;  // confirmed by finish(): EPF0 only ever runs together with EPF1 and EPF2 (epf_iters >= 3)
    add_border(Epf0Stage::BORDER);
    phase_ = kEpf1;
  }
  void on(const Epf1Stage& e1) {
    enter(kEpf1);
    if (e1.sigma_scale != 1.0f) unsupported("EPF1 with a sigma scale other than 1 (frame/render.rs:608-609)");
    p_.epf_border_sad_mul = e1.border_sad_mul;
    for (int c = 0; c < 3; c++) p_.epf_channel_scale[c] = e1.channel_scale[c];
    if (p_.epf_iters == 0) p_.epf_iters = 1;
    add_border(Epf1Stage::BORDER);
    phase_ = kEpf2;
    colour_.epf1_seen = true;
  }
  void on(const Epf2Stage& e2) {
    enter(kEpf2);
    if (!colour_.epf1_seen) unsupported("EPF2 without EPF1 (epf_iters >= 2 implies the first pass)");
    p_.epf_pass2_sigma_scale = e2.sigma_scale;
    if (p_.epf_iters < 2) p_.epf_iters = 2;
    add_border(Epf2Stage::BORDER);
    phase_ = kUpsample;
    colour_.epf2_seen = true;
  }

  template <int N>
  void on(const Upsample<N>& u) {
    enter(kUpsample);
    Colour& c = colour_;
    if (u.channel > 2) {  // an extra channel's own factor, or the frame's when it follows channel 2 (late_ec_upsample)
      const int ec = u.channel - 3;
      if (ec >= JXLH_MAX_EXTRA_CHANNELS || !lp_.extra[ec].bits) invalid("upsampling of an extra channel the list never converted to f32");
      if (lp_.extra[ec].upsampling != 1) invalid("an extra channel is upsampled once");
      // an extra channel's own upsampling comes before the patches (frame/render.rs:624-650); only the late form,
      // together with the colour channels, may follow them
      if (c.patches_seen && c.ups_seen == 0) unsupported(quoted() + " after the patches stage");
      if (c.splines_seen && c.ups_seen == 0) unsupported(quoted() + " after the splines stage");
      if (c.ups_seen != 0 && (c.ups_seen != 3 || N != c.ups_factor))
        invalid("extra channels upsampled with the colour channels use the frame's factor, after channel 2");
      one_table_per_factor(N, u.weights);
      lp_.weights_by_factor[N >> 2] = u.weights;
      lp_.extra[ec].upsampling = (uint32_t)N;
      return;
    }
    one_table_per_factor(N, u.weights);
    if ((c.ups_factor && c.ups_factor != N) || u.channel != c.ups_seen) invalid("frame upsampling: channels 0, 1, 2 with one factor");
    if (c.ups_seen && u.weights != lp_.upsampling_weights) invalid("frame upsampling: one weight table for the three channels");
    c.ups_factor = N;
    c.ups_seen++;
    lp_.upsampling_weights = u.weights;
    lp_.weights_by_factor[N >> 2] = u.weights;
    p_.upsampling = (uint32_t)N;
  }

  void on(const PatchesStage& ps) {
    // the reference's position: after the filters and the extra channels' own upsampling, before the colour
    // upsampling, noise and the colour stage (frame/render.rs:624-683)
    if (phase_ > kUpsample || colour_.ups_seen != 0 || colour_.patches_seen || colour_.splines_seen) out_of_order();
    planes_use_hook("patches", "patches");
    if (ps.blendings.size() != ps.patches.size() * (1 + ps.ec_flags.size())) invalid("patches: blendings != patches * (1 + num_ec)");
    phase_ = kUpsample;
    colour_.patches_seen = true;
    lp_.has_patches = true;
    lp_.patches = ps;
  }
  void on(const SplinesStage& sp) {
    // the reference's position: behind the patches stage (if any), before the colour upsampling, noise and the colour
    // stage (frame/render.rs:644-683)
    if (phase_ > kUpsample || colour_.ups_seen != 0 || colour_.splines_seen) out_of_order();
    planes_use_hook("splines", "splines");
    phase_ = kUpsample;
    colour_.splines_seen = true;
    lp_.has_splines = true;
    lp_.splines = sp;
  }

  void on(const ConvolveNoiseStage& cn) {
    enter(kNoiseConvolve);
    if (cn.channel != num_channels_ - 3 + colour_.conv_seen) invalid("noise convolution: the three temporaries behind the image channels");
    colour_.conv_seen++;
  }
  void on(const AddNoiseStage& an) {
    enter(kNoiseAdd);
    if (colour_.conv_seen != 3 || an.first_channel != num_channels_ - 3) invalid("AddNoise needs the three convolved noise channels");
    p_.noise = 1;
    for (int i = 0; i < 8; i++) p_.noise_lut[i] = an.lut[i];
    p_.ytox_lf = an.ytox_lf;
    p_.ytob_lf = an.ytob_lf;
    phase_ = kColour;
  }

  void colour_stage(int first_channel, uint32_t color, int next_phase) {
    enter(kColour);
    if (first_channel != 0 || colour_.have_colour) invalid("one colour stage on channels 0..2");
    colour_.have_colour = true;
    lp_.output.color = color;
    phase_ = next_phase;
  }
  void on(const XybStage& x) {
    colour_stage(x.first_channel, JXLH_COLOR_XYB, kTransfer);
    lp_.output.xyb = x.params;
  }
  // no transfer-function stage behind YCbCr (frame/render.rs:755-763)
  void on(const YcbcrToRgbStage& yc) { colour_stage(yc.first_channel, JXLH_COLOR_YCBCR, kConvert); }
  void on(const FromLinearStage& tf) {
    enter(kTransfer);
    if (lp_.output.color != JXLH_COLOR_XYB || colour_.have_tf || tf.first_channel != 0) unsupported("FromLinearStage without a preceding XybStage");
    if (tf.transfer > JXLH_TF_GAMMA) invalid("unknown transfer function");
    colour_.have_tf = true;
    lp_.output.transfer = tf.transfer;
    lp_.output.tf_param = tf.param;
    for (int i = 0; i < 3; i++) lp_.output.hlg_luminance_rgb[i] = tf.hlg_luminance_rgb[i];
    phase_ = kConvert;
  }

  // ---- the output side: each stage goes to the tail the list has
  void integer_conversion(int ch, uint32_t bits, uint32_t depth) {
    enter(kConvert);
    if (full_save_) tail_.integer_conversion(*this, ch, bits, depth);
    else legacy_.integer_conversion(ch, bits, depth);
  }
  void on(const ConvertF32ToU8Stage& c) { integer_conversion(c.channel, 8, c.bit_depth); }
  void on(const ConvertF32ToU16Stage& c) { integer_conversion(c.channel, 16, c.bit_depth); }
  void on(const ConvertF32ToF16Stage& f16) { full_tail().f16_conversion(*this, f16); }
  void on(const SpotColorStage& sp) { full_tail().spot_colour(*this, sp); }
  void on(const PremultiplyAlphaStage& pm) { full_tail().premultiply(*this, pm); }
  void on(const SaveStage& sv) {
    if (sv.full) return tail_.save(*this, sv);
    if (full_save_) unsupported(quoted() + ": the four-argument save stage in a list with a six-argument one");
    enter(kSave);
    legacy_.save(sv, lp_);
    phase_ = kDone;
  }

  // The legacy tail: the three integer conversions and the four-argument save stage, onto jxlh_output_desc
  struct LegacyTail {
    int convert_seen = 0;
    uint32_t convert_bits = 0;
    bool saved = false;
    void integer_conversion(int ch, uint32_t bits, uint32_t depth) {
      if (ch != convert_seen || ch > 2 || (convert_bits && convert_bits != bits)) invalid("integer conversion: channels 0, 1, 2 with one format");
      if (depth != bits) unsupported("integer output with a bit depth below the sample size");
      convert_bits = bits;
      convert_seen++;
    }
    void save(const SaveStage& sv, LoweredPipeline& lp) {
      if (saved) unsupported("more than one save stage (extra-channel outputs stay on the CPU pipeline)");
      if (sv.channels != std::vector<int>{0, 1, 2} || sv.output_buffer_index != 0) unsupported("save stage other than the colour channels into buffer 0");
      if (sv.bits == 32) {
        if (convert_seen) invalid("f32 save stage behind an integer conversion");
        if (sv.color_channels != 3) unsupported("planar f32 output has three channels");
      } else {
        if (convert_seen != 3 || convert_bits != sv.bits) invalid("save format and conversion stages disagree");
        if (sv.color_channels != 3 && sv.color_channels != 4) invalid("RGB or RGBA");
        lp.output.bits = sv.bits;
        lp.output.channels = sv.color_channels;
        lp.has_output = true;
      }
      saved = true;
    }
    void finish() const {
      if (convert_seen != 0 && convert_seen != 3) invalid("integer conversion on some channels only");
    }
  };

  // The save tail: spot colours, premultiplication and the conversions since the last save stage (one per channel),
  // which each six-argument save stage folds into a jxlh_save_desc (frame/render.rs:793-903)
  struct SaveTail {
    struct Conv {
      int channel;
      uint32_t format, depth;
      bool clamp;
      float clamp_min, clamp_max;
      std::string name;
    };
    std::vector<Conv> convs;
    std::vector<jxlh_spot_color> spots;
    bool premul_seen = false, colour_saved = false, seen = false;
    int premul_alpha = -1, premul_n = 0;

    bool begun() const { return !spots.empty() || premul_seen || !convs.empty() || seen; }
    void add_conv(const Lowering& lo, int ch, uint32_t format, uint32_t depth, bool clamp, float clamp_min, float clamp_max) {
      for (const Conv& c : convs)
        if (c.channel == ch) invalid(lo.quoted() + ": the channel is converted twice before a save stage");
      convs.push_back(Conv{ch, format, depth, clamp, clamp_min, clamp_max, lo.name_});
      seen = true;
    }
    void integer_conversion(const Lowering& lo, int ch, uint32_t bits, uint32_t depth) {  // checked by the save stage that follows
      if (ch < 0 || ch >= 3 + JXLH_MAX_EXTRA_CHANNELS || depth < 1 || depth > bits) invalid(lo.quoted() + ": channel or bit depth out of range");
      add_conv(lo, ch, bits == 8 ? JXLH_SAVE_U8 : JXLH_SAVE_U16, depth, false, 0.0f, 0.0f);
    }
    void f16_conversion(Lowering& lo, const ConvertF32ToF16Stage& f16) {
      if (lo.phase_ < kConvert) lo.enter(kConvert);
      if (f16.channel < 0 || f16.channel >= 3 + JXLH_MAX_EXTRA_CHANNELS) invalid(lo.quoted() + ": channel out of range");
      if (f16.clamp && !(f16.clamp_min <= f16.clamp_max)) invalid(lo.quoted() + ": clamp range with min > max or a NaN bound");
      add_conv(lo, f16.channel, JXLH_SAVE_F16, 0, f16.clamp, f16.clamp_min, f16.clamp_max);
    }
    // frame/render.rs:793-806 and :858-866: behind blend / extend, spot colours in front of premultiplication, both in
    // front of every conversion
    void in_front_of_conversions(const Lowering& lo) const {
      if (lo.phase_ > kConvert || !lo.lp_.saves.empty() || premul_seen || !convs.empty()) lo.out_of_order(JXLH_ERR_INVALID_ARGUMENT);
    }
    void spot_colour(Lowering& lo, const SpotColorStage& sp) {
      in_front_of_conversions(lo);
      if (!lo.is_extra_channel(sp.ec)) invalid(lo.quoted() + ": not an extra channel of the list");
      if (spots.size() == JXLH_MAX_EXTRA_CHANNELS) invalid("more spot colour stages than extra channels");
      jxlh_spot_color sc{};
      sc.ec = (uint32_t)sp.ec;
      for (int k = 0; k < 4; k++) sc.rgba[k] = sp.rgba[k];
      spots.push_back(sc);
      lo.phase_ = kConvert;
      seen = true;
    }
    void premultiply(Lowering& lo, const PremultiplyAlphaStage& pm) {
      in_front_of_conversions(lo);
      if (pm.first_color_channel != 0 || (pm.num_color_channels != 1 && pm.num_color_channels != 3))
        invalid(lo.quoted() + ": colour channels 0 or 0..2");
      if (!lo.is_extra_channel(pm.alpha_channel - 3)) invalid(lo.quoted() + ": the alpha is not an extra channel of the list");
      premul_seen = true;
      premul_alpha = pm.alpha_channel;
      premul_n = pm.num_color_channels;
      lo.phase_ = kConvert;
      seen = true;
    }
    // Saves come in buffer order, the colour one first (frame/render.rs:858-902)
    void save(Lowering& lo, const SaveStage& sv) {
      if (lo.phase_ < kConvert) lo.enter(kConvert);
      const std::string name = lo.quoted();
      std::vector<jxlh_save_desc>& saves = lo.lp_.saves;
      lo.planes_use_hook(name, "save");
      if (sv.output_buffer_index != (int)saves.size()) invalid(name + ": save stages come in output buffer order");
      const DataFormat& df = sv.data_format;
      if (df.format > JXLH_SAVE_F32 || sv.orientation < 1 || sv.orientation > 8) invalid(name + ": data format or orientation out of range");
      // the channel list against the colour type (frame/render.rs:851-857, :888-899)
      const bool gray = sv.color_type == ColorType::kGrayscale || sv.color_type == ColorType::kGrayscaleAlpha;
      const bool alpha = sv.color_type == ColorType::kGrayscaleAlpha || sv.color_type == ColorType::kRgba || sv.color_type == ColorType::kBgra;
      const bool bgr = sv.color_type == ColorType::kBgr || sv.color_type == ColorType::kBgra;
      const std::vector<int>& chs = sv.channels;
      const size_t ncol = gray ? 1 : 3;
      const bool ec_only = sv.color_type == ColorType::kGrayscale && chs.size() == 1 && chs[0] >= 3;
      if (!ec_only) {
        const size_t want = ncol + (alpha && !sv.fill_opaque_alpha ? 1 : 0);
        bool ok = chs.size() == want && (!sv.fill_opaque_alpha || alpha);
        for (size_t k = 0; ok && k < ncol; k++) ok = chs[k] == (int)k;
        if (ok && chs.size() > ncol) ok = chs[ncol] >= 3;
        if (!ok) invalid(name + ": channels, colour type and fill_opaque_alpha disagree");
      }
      for (int ch : chs)
        if (ch >= 3 && !lo.is_extra_channel(ch - 3)) invalid(name + ": an extra channel the list never converted to f32");
      if (!ec_only && colour_saved) unsupported(name + ": a second save of the colour channels");
      if (ec_only && !colour_saved && (premul_seen || !spots.empty()))
        invalid(name + ": spot colour / premultiply stages without a colour save behind them");
      // conversions: exactly the save's channels, in its format and depth; none for f32 (add_conversion_stages)
      jxlh_save_desc d{};
      d.format = df.format;
      d.bit_depth = df.format <= JXLH_SAVE_U16 ? df.bit_depth : 0;
      for (const Conv& c : convs) {
        bool mine = false;
        for (int ch : chs) mine |= ch == c.channel;
        if (!mine) invalid("stage '" + c.name + "' converts a channel the following save stage does not save");
      }
      if (df.format == JXLH_SAVE_F32) {
        if (!convs.empty()) invalid("stage '" + convs[0].name + "' in front of an f32 save stage");
      } else {
        if (df.format <= JXLH_SAVE_U16 && (df.bit_depth < 1 || df.bit_depth > (df.format == JXLH_SAVE_U8 ? 8u : 16u)))
          invalid(name + ": bit depth out of range");
        for (size_t k = 0; k < chs.size(); k++) {
          const Conv* c = nullptr;
          for (const Conv& cv : convs)
            if (cv.channel == chs[k]) c = &cv;
          if (!c) invalid(name + ": channel " + std::to_string(chs[k]) + " has no conversion to the save's format");
          if (c->format != df.format || c->depth != d.bit_depth) invalid("stage '" + c->name + "' and " + name + " disagree on format or bit depth");
          if (k == 0) {
            d.f16_clamp = c->clamp;
            d.f16_clamp_min = c->clamp_min;
            d.f16_clamp_max = c->clamp_max;
          } else if ((bool)d.f16_clamp != c->clamp || (c->clamp && (d.f16_clamp_min != c->clamp_min || d.f16_clamp_max != c->clamp_max))) {
            unsupported("stage '" + c->name + "': one f16 clamp range per save stage");
          }
        }
      }
      convs.clear();
      d.n_channels = (uint32_t)chs.size();
      for (size_t k = 0; k < chs.size(); k++) d.channels[k] = (uint32_t)chs[k];
      if (bgr) std::swap(d.channels[0], d.channels[2]);  // render/save.rs:33-40
      d.fill_opaque_alpha = sv.fill_opaque_alpha;
      d.big_endian = df.big_endian && df.format != JXLH_SAVE_U8;
      d.orientation = sv.orientation;
      if (!ec_only) {
        if (premul_seen && (premul_n != (int)ncol || chs.size() <= ncol || chs[ncol] != premul_alpha))
          invalid(name + ": the premultiply stage in front names other channels");
        d.premultiply = premul_seen;
        d.premultiply_alpha_channel = premul_seen ? (uint32_t)premul_alpha : 0;
        d.n_spot = (uint32_t)spots.size();
        for (size_t i = 0; i < spots.size(); i++) d.spot[i] = spots[i];
        colour_saved = true;
      }
      saves.push_back(d);
      seen = true;
      lo.phase_ = kConvert;  // further conversions and saves (the extra channels' buffers) may follow
    }
    void finish(const LoweredPipeline& lp) const {
      if (lp.saves.empty()) return;
      if (!convs.empty()) invalid("stage '" + convs[0].name + "' without a save stage behind it");
      if ((premul_seen || !spots.empty()) && !colour_saved) invalid("spot colour / premultiply stages without a save of the colour channels");
    }
  };

  // ---- consistency of the whole list, then the sizes
  void finish() {
    const Colour& c = colour_;
    finish_modular();
    if (p_.gab && !(c.gab_seen[0] && c.gab_seen[1] && c.gab_seen[2])) invalid("Gaborish on some channels only");
    if (p_.epf_iters == 3 && !(c.epf1_seen && c.epf2_seen)) unsupported("EPF0 without EPF1 and EPF2 (epf_iters >= 3 runs all three)");
    if (c.ups_seen != 0 && c.ups_seen != 3) invalid("frame upsampling on some channels only");
    if ((size_t)c.ups_factor != (c.ups_factor ? (size_t)1 << downsampling_shift_ : 0) && c.ups_factor != 0)
      invalid("upsampling factor and downsampling_shift disagree");
    if (!c.ups_factor && downsampling_shift_ != 0) invalid("downsampling_shift without upsampling stages");
    if (c.conv_seen != 0 && !p_.noise) invalid("noise convolution without AddNoise");
    tail_.finish(lp_);
    legacy_.finish();
    if (!legacy_.saved && lp_.saves.empty()) invalid("no save stage");
    if (lp_.has_output && lp_.output.color == JXLH_COLOR_NONE && c.have_tf) invalid("transfer function without colour stage");
    if (blend_.expect_extend) invalid("blending stage without the extend stage behind it");
    if (lp_.has_blend) {  // the colour stage runs inside jxlh_frame_blend; the conversion reads the composed image as it is
      lp_.blend_colour = lp_.output;
      lp_.output.color = JXLH_COLOR_NONE;
      lp_.output.transfer = JXLH_TF_LINEAR;
    }
    // size = FrameHeader::size_upsampled() (builder.rs:70-85): the frame itself is size >> downsampling_shift
    const uint32_t n = p_.upsampling;
    if (size_.first == 0 || size_.second == 0) invalid("empty frame");
    p_.xsize_upsampled = n > 1 ? (uint32_t)size_.first : 0;
    p_.ysize_upsampled = n > 1 ? (uint32_t)size_.second : 0;
    if (n > 1) {
      if ((size_.first + n - 1) / n != p_.xsize || (size_.second + n - 1) / n != p_.ysize)
        invalid("size_upsampled does not belong to the base frame size");
    } else if (size_.first != p_.xsize || size_.second != p_.ysize) {
      invalid("pipeline size and frame size disagree");
    }
    lp_.out_w = lp_.has_blend ? lp_.blend.image_w : (uint32_t)size_.first;
    lp_.out_h = lp_.has_blend ? lp_.blend.image_h : (uint32_t)size_.second;
  }
  // what a list that opens with Modular conversions may hold, by the entry point it came through
  void finish_modular() {
    const Colour& c = colour_;
    const bool chroma = p_.hshift[0] | p_.hshift[1] | p_.hshift[2] | p_.vshift[0] | p_.vshift[1] | p_.vshift[2];
    if (lp_.modular == Modular::kToF32 && c.modular_seen != 3) invalid("Modular -> f32 conversion on some channels only");
    if (modular_frame_) {
      // the frame runs through jxlh_frame_run: every stage the VarDCT list may hold is served; the I32 -> U8 special case
      // stays with build_modular
      if (lp_.modular == Modular::kNone) invalid("the stage list holds no Modular conversion");
      p_.flags |= JXLH_FRAME_MODULAR;
      if (lp_.modular == Modular::kXybToF32) {
        if (chroma) invalid("chroma subsampling on an XYB Modular frame");
        lp_.modular_sample_format = JXLH_MODULAR_XYB;
        for (int i = 0; i < 3; i++) p_.lf_quant_factors[i] = lp_.modular_quant_factors[i];
      } else {
        lp_.modular_sample_format = lp_.modular_bits;
      }
    } else if (lp_.modular != Modular::kNone) {
      // what this path runs for a Modular frame: the conversion, Gaborish / EPF with the constant sigma of
      // features/epf.rs:81-84 (jxlh_modular_frame_filters), then either the planes themselves or -- the builder's special
      // case -- straight to bytes
      if (p_.upsampling != 1 || p_.noise || chroma) unsupported("upsampling / noise / chroma subsampling on a Modular frame");
      const bool untouched = !p_.gab && p_.epf_iters == 0 && !c.have_colour && !c.have_tf;
      if (legacy_.convert_seen == 3) {
        // builder.rs:152-170: ConvertModularToF32(c, d) whose next use is ConvertF32ToU8(c, b) with b % d == 0 becomes
        // ConvertI32ToU8Stage(c, ((1 << b) - 1) / ((1 << d) - 1), (1 << b) - 1) and the second stage disappears
        if (lp_.modular == Modular::kToF32 && untouched && legacy_.convert_bits == 8 && 8 % lp_.modular_bits == 0) {
          lp_.modular = Modular::kI32ToU8;
          lp_.i32_to_u8_multiplier = 255 / ((1 << lp_.modular_bits) - 1);
          lp_.i32_to_u8_max = 255;
        } else {
          unsupported("integer output of a Modular frame other than the I32 -> U8 special case");
        }
      } else if (c.have_colour || c.have_tf) {
        unsupported("colour stages on a Modular frame");
      }
    }
  }

  // ---- what the builder was constructed with
  const int num_channels_;
  const std::pair<size_t, size_t> size_;
  const size_t downsampling_shift_;
  const bool modular_frame_;
  // ---- the result, and the stage at hand
  LoweredPipeline lp_;
  jxlh_frame_params& p_ = lp_.frame;
  std::string name_;  // its Display string
  // ---- state, by what it guards
  int phase_ = kModular;  // the order tracker: enter()
  struct Colour {         // the colour channels on their way through the frame's stages
    int modular_seen = 0;  // Modular -> f32 conversions
    bool gab_seen[3] = {false, false, false};
    bool epf1_seen = false, epf2_seen = false;
    bool patches_seen = false, splines_seen = false;
    int ups_seen = 0, ups_factor = 0;  // frame upsampling: channels done, their factor
    int conv_seen = 0;                 // noise convolutions
    bool have_colour = false, have_tf = false;
  } colour_;
  struct {  // BlendingStage must be followed at once by the extend stage (frame/render.rs:765-771)
    bool seen = false, extend_seen = false, expect_extend = false;
  } blend_;
  bool full_save_ = false;  // the list has a six-argument save stage: its output side is tail_'s, otherwise legacy_'s
  LegacyTail legacy_;
  SaveTail tail_;
};

}  // namespace detail

class GpuRenderPipeline;
class GpuModularFramePipeline;

// RenderPipelineBuilder (builder.rs:19-120).  `base` carries what is not a stage: frame size, quantiser and colour
// correlation fields, the EPF sharpness LUT / quant_mul of the sigma map, flags.
class RenderPipelineBuilder {
 public:
  // builder.rs:70-85: num_channels (3 colour + extra + noise temporaries), size = FrameHeader::size_upsampled(),
  // downsampling_shift = log2(upsampling), log_group_size = FrameHeader::log_group_dim() (8 on this path)
  RenderPipelineBuilder(size_t num_channels, std::pair<size_t, size_t> size, size_t downsampling_shift, size_t log_group_size,
                        const jxlh_frame_params& base)
      : num_channels_(num_channels), size_(size), downsampling_shift_(downsampling_shift), log_group_size_(log_group_size),
        base_(base) {}

  template <class S>
  RenderPipelineBuilder add_inout_stage(S stage) && {
    stages_.emplace_back(std::move(stage));
    return std::move(*this);
  }
  template <class S>
  RenderPipelineBuilder add_inplace_stage(S stage) && {
    stages_.emplace_back(std::move(stage));
    return std::move(*this);
  }
  RenderPipelineBuilder add_save_stage(std::vector<int> channels, int output_buffer_index, uint32_t color_channels,
                                       uint32_t bits) && {
    stages_.emplace_back(SaveStage{std::move(channels), output_buffer_index, color_channels, bits});
    return std::move(*this);
  }
  // builder.rs:87-105 in full: channels, orientation, output buffer index, colour type, data format, fill_opaque_alpha
  RenderPipelineBuilder add_save_stage(std::vector<int> channels, uint32_t orientation, int output_buffer_index,
                                       ColorType color_type, DataFormat data_format, bool fill_opaque_alpha) && {
    SaveStage st{std::move(channels), output_buffer_index, 0, 0};
    st.full = true;
    st.orientation = orientation;
    st.color_type = color_type;
    st.data_format = data_format;
    st.fill_opaque_alpha = fill_opaque_alpha;
    stages_.emplace_back(std::move(st));
    return std::move(*this);
  }
  RenderPipelineBuilder add_extend_stage() && {  // without the stage's arguments there is nothing to lower
    stages_.emplace_back(CpuOnlyStage{"extend to image dimensions"});
    return std::move(*this);
  }
  // builder.rs add_extend_stage(ExtendToImageDimensionsStage::new(frame_header, file_header, reference_frames))
  RenderPipelineBuilder add_extend_stage(ExtendToImageDimensionsStage stage) && {
    stages_.emplace_back(std::move(stage));
    return std::move(*this);
  }

  // The host-side half of build(): validation + lowering, no device needed.  Throws Error(JXLH_ERR_UNSUPPORTED)
  // for a stage list outside this path and Error(JXLH_ERR_INVALID_ARGUMENT) for an inconsistent one.
  LoweredPipeline lower() const { return lower_list(false); }
  // The same for a Modular frame that lives on the context (JXLH_FRAME_MODULAR): the reference's full Modular list --
  // conversions, chroma upsampling, Gaborish / EPF, extra channels, patches, splines, frame upsampling, noise, colour
  // stages, blending + extend, spot / premultiply / convert / save -- under the order and consistency checks lower()
  // applies to a VarDCT list, onto the same LoweredPipeline fields plus modular_sample_format.
  LoweredPipeline lower_modular_frame() const { return lower_list(true); }
  // builder.rs:120: returns the pipeline (here: begins the frame on the context with the lowered parameters)
  std::unique_ptr<GpuRenderPipeline> build(Context& ctx) &&;
  // the same for a Modular frame's list (it opens with ConvertModularToF32Stage x3 or ConvertModularXYBToF32Stage)
  std::unique_ptr<class GpuModularPipeline> build_modular(Context& ctx) &&;
  // ... as a frame of the context: begins it with JXLH_FRAME_MODULAR and the lowered parameters
  std::unique_ptr<GpuModularFramePipeline> build_modular_frame(Context& ctx) &&;

 private:
  // modular_frame: the list is a Modular frame's and the frame runs through jxlh_frame_run (lower_modular_frame);
  // otherwise a Modular list is the caller-held-planes form of build_modular, with its narrower stage set
  LoweredPipeline lower_list(bool modular_frame) const {
    return detail::Lowering(num_channels_, size_, downsampling_shift_, log_group_size_, base_, modular_frame).run(stages_);
  }
  size_t num_channels_;
  std::pair<size_t, size_t> size_;
  size_t downsampling_shift_, log_group_size_;
  jxlh_frame_params base_;
  std::vector<Stage> stages_;
};

}  // namespace jxlh
