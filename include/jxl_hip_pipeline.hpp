// C++ mirror of the reference's stage traits and pipeline builder for the path this library replaces
// (jxl/src/render/mod.rs:52-157 RenderPipelineInOutStage / RenderPipelineInPlaceStage / RenderPipeline,
// jxl/src/render/builder.rs:19-120 RenderPipelineBuilder, and the stage list of
// Frame::build_render_pipeline, jxl/src/frame/render.rs:526-790).
//
// The reference assembles a frame's post-processing as a list of stage objects and lets a RenderPipeline
// implementation run them row chunk by row chunk.  On the device the same list is ONE launch sequence behind
// jxlh_frame_run (K1, the fused Gaborish / EPF kernel, chroma / frame upsampling, noise) plus one output pass
// (jxlh_frame_read_output): so the builder here takes the stages under the reference's names, with the reference's
// constructor arguments, in the reference's order, checks that the list is one the device path implements (anything
// else is JXLH_ERR_UNSUPPORTED naming the stage: that stage list stays on the CPU pipeline), and LOWERS it onto
// jxlh_frame_params + jxlh_output_desc.  GpuRenderPipeline then carries the trait's methods for this path:
// set_buffer_for_group (with the `complete` flag of render/mod.rs:128-136), mark_group_to_rerender, do_render,
// check_buffer_sizes.  BORDER / SHIFT of every stage are the reference's constants, and the pipeline reports the
// accumulated input border the way RenderPipelineShared does (render/internal.rs) -- 4 pixels for Gaborish + EPF1 + EPF2,
// jxl/src/render/mod.rs:28-36 -- which is the halo the fused kernel stages and the sharded path exchanges.
//
// Header-only, C++17, no HIP types; tests/cpp/pipeline_builder.cc drives it (host-only checks without a GPU, a whole
// frame against the oracle with one).
#pragma once
#include <array>
#include <cstdint>
#include <cstring>
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
  [[noreturn]] static void fail(jxlh_status st, const std::string& what) { throw Error(st, "RenderPipelineBuilder::build", what); }
  // modular_frame: the list is a Modular frame's and the frame runs through jxlh_frame_run (lower_modular_frame);
  // otherwise a Modular list is the caller-held-planes form of build_modular, with its narrower stage set
  LoweredPipeline lower_list(bool modular_frame) const;
  size_t num_channels_;
  std::pair<size_t, size_t> size_;
  size_t downsampling_shift_, log_group_size_;
  jxlh_frame_params base_;
  std::vector<Stage> stages_;
};

inline LoweredPipeline RenderPipelineBuilder::lower_list(bool modular_frame) const {
  LoweredPipeline lp;
  lp.frame = base_;
  jxlh_frame_params& p = lp.frame;
  if (log_group_size_ != 8 + downsampling_shift_ && log_group_size_ != 8)
    fail(JXLH_ERR_UNSUPPORTED, "group dimension other than 256 (FrameHeader::log_group_dim)");
  if (num_channels_ < 3) fail(JXLH_ERR_INVALID_ARGUMENT, "fewer than three channels");
  // stage-derived fields start from "no stage"
  p.gab = 0;
  p.epf_iters = 0;
  p.upsampling = 1;
  p.noise = 0;
  for (int c = 0; c < 3; c++) p.hshift[c] = p.vshift[c] = 0;
  // The reference's order (frame/render.rs:568-790) as phases; a stage may only appear in a phase >= the current one.
  enum Phase { kModular, kChroma, kGab, kEpf0, kEpf1, kEpf2, kUpsample, kNoiseConvolve, kNoiseAdd, kColour, kTransfer, kConvert, kSave, kDone };
  int phase = kModular;
  auto enter = [&](int ph, const Stage& s) {
    if (ph < phase) fail(JXLH_ERR_UNSUPPORTED, "stage '" + stage_display(s) + "' out of the order of Frame::build_render_pipeline");
    phase = ph;
  };
  bool gab_seen[3] = {false, false, false};
  int ups_seen = 0, ups_factor = 0, conv_seen = 0, convert_seen = 0, modular_seen = 0;
  const float*(&ec_weights)[3] = lp.weights_by_factor;  // index n >> 2: factor 2, 4, 8
  uint32_t convert_bits = 0;
  bool have_colour = false, have_tf = false, have_save = false, pre_upsample = true, epf1_seen = false, epf2_seen = false;
  bool patches_seen = false, splines_seen = false;
  // BlendingStage must be followed at once by the extend stage (frame/render.rs:765-771)
  bool blend_seen = false, extend_seen = false, expect_extend = false;
  auto same_info = [](const jxlh_blending_info& a, const jxlh_blending_info& b) {
    return a.mode == b.mode && a.alpha_channel == b.alpha_channel && a.clamp == b.clamp && a.source == b.source;
  };
  // the save tail: conversions since the last save stage (one per channel), spot colours, premultiplication
  struct Conv {
    int channel;
    uint32_t format, depth;
    bool clamp;
    float clamp_min, clamp_max;
    std::string name;
  };
  std::vector<Conv> convs;
  std::vector<jxlh_spot_color> spots;
  bool premul_seen = false, colour_saved = false, tail_seen = false;
  // A list with a six-argument save stage is checked by the save tail's rules; a list without one goes through the
  // checks it always went through, with the statuses it always got.
  bool has_full_save = false;
  for (const Stage& s : stages_)
    if (const auto* sv = std::get_if<SaveStage>(&s)) has_full_save |= sv->full;
  int premul_alpha = -1, premul_n = 0;
  auto add_conv = [&](const Stage& s, int ch, uint32_t format, uint32_t depth, bool clamp, float lo, float hi) {
    for (const Conv& c : convs)
      if (c.channel == ch) fail(JXLH_ERR_INVALID_ARGUMENT, "stage '" + stage_display(s) + "': the channel is converted twice before a save stage");
    convs.push_back(Conv{ch, format, depth, clamp, lo, hi, stage_display(s)});
  };
  Border border{0, 0};
  auto add_border = [&](Border b) {
    if (pre_upsample) {
      border.x = (uint8_t)(border.x + b.x);
      border.y = (uint8_t)(border.y + b.y);
    }
  };
  lp.output.color = JXLH_COLOR_NONE;
  lp.output.transfer = JXLH_TF_LINEAR;
  lp.output.bits = 0;
  lp.output.channels = 3;
  for (const Stage& s : stages_) {
    lp.stages.push_back(stage_display(s));
    if (expect_extend && !std::holds_alternative<ExtendToImageDimensionsStage>(s))
      fail(JXLH_ERR_INVALID_ARGUMENT, "stage '" + stage_display(s) + "' between the blending stage and the extend stage");
    if (blend_seen && (std::holds_alternative<XybStage>(s) || std::holds_alternative<YcbcrToRgbStage>(s) ||
                       std::holds_alternative<FromLinearStage>(s)))
      fail(JXLH_ERR_INVALID_ARGUMENT, "blending / extend stage before the colour stage '" + stage_display(s) + "'");
    if (const auto* st = std::get_if<CpuOnlyStage>(&s)) {
      fail(JXLH_ERR_UNSUPPORTED, "stage '" + st->name + "' is not part of the device path");
    } else if (const auto* bl = std::get_if<BlendingStage>(&s)) {
      // the reference's position: behind the colour stage, in front of the conversions (frame/render.rs:754-779)
      if (blend_seen) fail(JXLH_ERR_INVALID_ARGUMENT, "two blending stages");
      if (phase > kConvert || convert_seen) fail(JXLH_ERR_INVALID_ARGUMENT, "blending stage behind the conversion / save stages");
      // frame/render.rs:765-806: spot colours, premultiplication and every conversion come behind blend / extend
      if (!spots.empty() || premul_seen || !convs.empty() || tail_seen)
        fail(JXLH_ERR_INVALID_ARGUMENT, "stage '" + stage_display(s) + "' behind a spot colour, premultiply or conversion stage: they follow the blending and extend stages");
      if (!modular_frame && lp.modular != LoweredPipeline::Modular::kNone)
        fail(JXLH_ERR_UNSUPPORTED, "blending on a Modular frame (jxlh_stage_blend on the planes instead)");
      const size_t nec = bl->ec_blending_info.size();
      size_t named = 0;
      while (named < JXLH_MAX_EXTRA_CHANNELS && lp.extra[named].bits) named++;
      if (nec > JXLH_MAX_EXTRA_CHANNELS || bl->ec_flags.size() != nec || nec != named)
        fail(JXLH_ERR_INVALID_ARGUMENT, "blending: one ec_blending_info and one flag word per extra channel of the list");
      blend_seen = expect_extend = true;
      lp.has_blend = true;
      lp.blend = jxlh_blend_desc{};
      lp.blend.x0 = bl->x0;
      lp.blend.y0 = bl->y0;
      lp.blend.image_w = bl->image_w;
      lp.blend.image_h = bl->image_h;
      lp.blend.color = bl->blending_info;
      lp.blend.num_ec = (uint32_t)nec;
      for (size_t i = 0; i < nec; i++) {
        lp.blend.ec[i] = bl->ec_blending_info[i];
        lp.blend.ec_flags[i] = bl->ec_flags[i];
      }
      phase = kConvert;
    } else if (const auto* ex = std::get_if<ExtendToImageDimensionsStage>(&s)) {
      if (!spots.empty() || premul_seen || !convs.empty() || tail_seen)
        fail(JXLH_ERR_INVALID_ARGUMENT, "stage '" + stage_display(s) + "' behind a spot colour, premultiply or conversion stage: they follow the blending and extend stages");
      if (!expect_extend) fail(JXLH_ERR_INVALID_ARGUMENT, extend_seen ? "two extend stages" : "extend stage without a blending stage in front of it");
      bool same = ex->x0 == lp.blend.x0 && ex->y0 == lp.blend.y0 && ex->image_w == lp.blend.image_w &&
                  ex->image_h == lp.blend.image_h && same_info(ex->blending_info, lp.blend.color) &&
                  ex->ec_blending_info.size() == lp.blend.num_ec;
      for (size_t i = 0; same && i < ex->ec_blending_info.size(); i++) same = same_info(ex->ec_blending_info[i], lp.blend.ec[i]);
      if (!same) fail(JXLH_ERR_INVALID_ARGUMENT, "blending and extend stages built from different headers");
      expect_extend = false;
      extend_seen = true;
    } else if (const auto* m = std::get_if<ConvertModularToF32Stage>(&s)) {
      enter(kModular, s);
      if (m->bit_depth < 1 || m->bit_depth > 31) fail(JXLH_ERR_INVALID_ARGUMENT, "bit depth");
      if (m->channel > 2) {  // an extra channel: any frame encoding, after the colour conversions
        const int ec = m->channel - 3;
        if (ec >= JXLH_MAX_EXTRA_CHANNELS) fail(JXLH_ERR_UNSUPPORTED, "more extra channels than JXLH_MAX_EXTRA_CHANNELS");
        if (m->channel >= (int)num_channels_ || lp.extra[ec].bits || (ec > 0 && !lp.extra[ec - 1].bits))
          fail(JXLH_ERR_INVALID_ARGUMENT, "Modular -> f32 conversion of extra channels: channels 3.. in order, once each");
        if (modular_seen != 0 && modular_seen != 3) fail(JXLH_ERR_INVALID_ARGUMENT, "extra channel conversion between the colour conversions");
        lp.extra[ec].bits = m->bit_depth;
        continue;
      }
      if (m->channel != modular_seen || lp.modular == LoweredPipeline::Modular::kXybToF32 || lp.extra[0].bits)
        fail(JXLH_ERR_INVALID_ARGUMENT, "Modular -> f32 conversion: channels 0, 1, 2 in order, before the extra channels");
      if (modular_seen && m->bit_depth != lp.modular_bits) fail(JXLH_ERR_UNSUPPORTED, "colour channels of different bit depths");
      lp.modular = LoweredPipeline::Modular::kToF32;
      lp.modular_bits = m->bit_depth;
      modular_seen++;
    } else if (const auto* mx = std::get_if<ConvertModularXYBToF32Stage>(&s)) {
      enter(kModular, s);
      if (mx->first_channel != 0 || lp.modular != LoweredPipeline::Modular::kNone) fail(JXLH_ERR_INVALID_ARGUMENT, "one XYB conversion on channels 0..2");
      lp.modular = LoweredPipeline::Modular::kXybToF32;
      lp.modular_quant_factors = mx->quant_factors;
      modular_seen = 3;
    } else if (const auto* h = std::get_if<HorizontalChromaUpsample>(&s)) {
      enter(kChroma, s);
      if (h->channel < 0 || h->channel > 2) fail(JXLH_ERR_INVALID_ARGUMENT, "chroma upsampling of a non-colour channel");
      p.hshift[h->channel] = 1;
    } else if (const auto* v = std::get_if<VerticalChromaUpsample>(&s)) {
      enter(kChroma, s);
      if (v->channel < 0 || v->channel > 2) fail(JXLH_ERR_INVALID_ARGUMENT, "chroma upsampling of a non-colour channel");
      p.vshift[v->channel] = 1;
    } else if (const auto* g = std::get_if<GaborishStage>(&s)) {
      enter(kGab, s);
      if (g->channel < 0 || g->channel > 2 || gab_seen[g->channel]) fail(JXLH_ERR_INVALID_ARGUMENT, "Gaborish: one stage per colour channel");
      gab_seen[g->channel] = true;
      p.gab = 1;
      p.gab_w1[g->channel] = g->weight1;
      p.gab_w2[g->channel] = g->weight2;
      if (g->channel == 0) add_border(GaborishStage::BORDER);
    } else if (const auto* e0 = std::get_if<Epf0Stage>(&s)) {
      enter(kEpf0, s);
      p.epf_pass0_sigma_scale = e0->sigma_scale;
      p.epf_border_sad_mul = e0->border_sad_mul;
      for (int c = 0; c < 3; c++) p.epf_channel_scale[c] = e0->channel_scale[c];
      p.epf_iters = 3;  // confirmed below: EPF0 only ever runs together with EPF1 and EPF2 (epf_iters >= 3)
      add_border(Epf0Stage::BORDER);
      phase = kEpf1;
    } else if (const auto* e1 = std::get_if<Epf1Stage>(&s)) {
      enter(kEpf1, s);
      if (e1->sigma_scale != 1.0f) fail(JXLH_ERR_UNSUPPORTED, "EPF1 with a sigma scale other than 1 (frame/render.rs:608-609)");
      p.epf_border_sad_mul = e1->border_sad_mul;
      for (int c = 0; c < 3; c++) p.epf_channel_scale[c] = e1->channel_scale[c];
      if (p.epf_iters == 0) p.epf_iters = 1;
      add_border(Epf1Stage::BORDER);
      phase = kEpf2;
      epf1_seen = true;
    } else if (const auto* e2 = std::get_if<Epf2Stage>(&s)) {
      enter(kEpf2, s);
      if (!epf1_seen) fail(JXLH_ERR_UNSUPPORTED, "EPF2 without EPF1 (epf_iters >= 2 implies the first pass)");
      p.epf_pass2_sigma_scale = e2->sigma_scale;
      if (p.epf_iters < 2) p.epf_iters = 2;
      add_border(Epf2Stage::BORDER);
      phase = kUpsample;
      epf2_seen = true;
    } else if (std::holds_alternative<Upsample2x>(s) || std::holds_alternative<Upsample4x>(s) || std::holds_alternative<Upsample8x>(s)) {
      enter(kUpsample, s);
      int n = 0, ch = 0;
      const float* w = nullptr;
      if (const auto* u = std::get_if<Upsample2x>(&s)) n = 2, ch = u->channel, w = u->weights;
      if (const auto* u = std::get_if<Upsample4x>(&s)) n = 4, ch = u->channel, w = u->weights;
      if (const auto* u = std::get_if<Upsample8x>(&s)) n = 8, ch = u->channel, w = u->weights;
      if (ch > 2) {  // an extra channel's own factor, or the frame's when it follows channel 2 (late_ec_upsample)
        const int ec = ch - 3;
        if (ec >= JXLH_MAX_EXTRA_CHANNELS || !lp.extra[ec].bits) fail(JXLH_ERR_INVALID_ARGUMENT, "upsampling of an extra channel the list never converted to f32");
        if (lp.extra[ec].upsampling != 1) fail(JXLH_ERR_INVALID_ARGUMENT, "an extra channel is upsampled once");
        // an extra channel's own upsampling comes before the patches (frame/render.rs:624-650); only the late form,
        // together with the colour channels, may follow them
        if (patches_seen && ups_seen == 0) fail(JXLH_ERR_UNSUPPORTED, "stage '" + stage_display(s) + "' after the patches stage");
        if (splines_seen && ups_seen == 0) fail(JXLH_ERR_UNSUPPORTED, "stage '" + stage_display(s) + "' after the splines stage");
        if (ups_seen != 0 && (ups_seen != 3 || n != ups_factor)) fail(JXLH_ERR_INVALID_ARGUMENT, "extra channels upsampled with the colour channels use the frame's factor, after channel 2");
        if (ec_weights[n >> 2] && ec_weights[n >> 2] != w) fail(JXLH_ERR_INVALID_ARGUMENT, "one weight table per upsampling factor (CustomTransformData)");
        ec_weights[n >> 2] = w;
        lp.extra[ec].upsampling = (uint32_t)n;
        continue;
      }
      if (ec_weights[n >> 2] && ec_weights[n >> 2] != w) fail(JXLH_ERR_INVALID_ARGUMENT, "one weight table per upsampling factor (CustomTransformData)");
      if ((ups_factor && ups_factor != n) || ch != ups_seen) fail(JXLH_ERR_INVALID_ARGUMENT, "frame upsampling: channels 0, 1, 2 with one factor");
      if (ups_seen && w != lp.upsampling_weights) fail(JXLH_ERR_INVALID_ARGUMENT, "frame upsampling: one weight table for the three channels");
      ups_factor = n;
      ups_seen++;
      lp.upsampling_weights = w;
      ec_weights[n >> 2] = w;
      p.upsampling = (uint32_t)n;
      pre_upsample = false;
    } else if (const auto* ps = std::get_if<PatchesStage>(&s)) {
      // the reference's position: after the filters and the extra channels' own upsampling, before the colour
      // upsampling, noise and the colour stage (frame/render.rs:624-683)
      if (phase > kUpsample || ups_seen != 0 || patches_seen || splines_seen)
        fail(JXLH_ERR_UNSUPPORTED, "stage 'patches' out of the order of Frame::build_render_pipeline");
      if (!modular_frame && lp.modular != LoweredPipeline::Modular::kNone)
        fail(JXLH_ERR_UNSUPPORTED, "patches on a Modular frame (jxlh_stage_patches on the planes instead)");
      if (ps->blendings.size() != ps->patches.size() * (1 + ps->ec_flags.size()))
        fail(JXLH_ERR_INVALID_ARGUMENT, "patches: blendings != patches * (1 + num_ec)");
      phase = kUpsample;
      patches_seen = true;
      lp.has_patches = true;
      lp.patches = *ps;
    } else if (const auto* sp = std::get_if<SplinesStage>(&s)) {
      // the reference's position: behind the patches stage (if any), before the colour upsampling, noise and the colour
      // stage (frame/render.rs:644-683)
      if (phase > kUpsample || ups_seen != 0 || splines_seen)
        fail(JXLH_ERR_UNSUPPORTED, "stage 'splines' out of the order of Frame::build_render_pipeline");
      if (!modular_frame && lp.modular != LoweredPipeline::Modular::kNone)
        fail(JXLH_ERR_UNSUPPORTED, "splines on a Modular frame (jxlh_stage_splines on the planes instead)");
      phase = kUpsample;
      splines_seen = true;
      lp.has_splines = true;
      lp.splines = *sp;
    } else if (const auto* cn = std::get_if<ConvolveNoiseStage>(&s)) {
      enter(kNoiseConvolve, s);
      if (cn->channel != (int)num_channels_ - 3 + conv_seen) fail(JXLH_ERR_INVALID_ARGUMENT, "noise convolution: the three temporaries behind the image channels");
      conv_seen++;
    } else if (const auto* an = std::get_if<AddNoiseStage>(&s)) {
      enter(kNoiseAdd, s);
      if (conv_seen != 3 || an->first_channel != (int)num_channels_ - 3) fail(JXLH_ERR_INVALID_ARGUMENT, "AddNoise needs the three convolved noise channels");
      p.noise = 1;
      for (int i = 0; i < 8; i++) p.noise_lut[i] = an->lut[i];
      p.ytox_lf = an->ytox_lf;
      p.ytob_lf = an->ytob_lf;
      phase = kColour;
    } else if (const auto* x = std::get_if<XybStage>(&s)) {
      enter(kColour, s);
      if (x->first_channel != 0 || have_colour) fail(JXLH_ERR_INVALID_ARGUMENT, "one colour stage on channels 0..2");
      have_colour = true;
      lp.output.color = JXLH_COLOR_XYB;
      lp.output.xyb = x->params;
      phase = kTransfer;
    } else if (const auto* yc = std::get_if<YcbcrToRgbStage>(&s)) {
      enter(kColour, s);
      if (yc->first_channel != 0 || have_colour) fail(JXLH_ERR_INVALID_ARGUMENT, "one colour stage on channels 0..2");
      have_colour = true;
      lp.output.color = JXLH_COLOR_YCBCR;
      phase = kConvert;  // no transfer-function stage behind YCbCr (frame/render.rs:755-763)
    } else if (const auto* tf = std::get_if<FromLinearStage>(&s)) {
      enter(kTransfer, s);
      if (lp.output.color != JXLH_COLOR_XYB || have_tf || tf->first_channel != 0) fail(JXLH_ERR_UNSUPPORTED, "FromLinearStage without a preceding XybStage");
      if (tf->transfer > JXLH_TF_GAMMA) fail(JXLH_ERR_INVALID_ARGUMENT, "unknown transfer function");
      have_tf = true;
      lp.output.transfer = tf->transfer;
      lp.output.tf_param = tf->param;
      for (int i = 0; i < 3; i++) lp.output.hlg_luminance_rgb[i] = tf->hlg_luminance_rgb[i];
      phase = kConvert;
    } else if (std::holds_alternative<ConvertF32ToU8Stage>(s) || std::holds_alternative<ConvertF32ToU16Stage>(s)) {
      enter(kConvert, s);
      int ch;
      uint32_t bits, depth;
      if (const auto* c8 = std::get_if<ConvertF32ToU8Stage>(&s)) ch = c8->channel, bits = 8, depth = c8->bit_depth;
      else ch = std::get<ConvertF32ToU16Stage>(s).channel, bits = 16, depth = std::get<ConvertF32ToU16Stage>(s).bit_depth;
      if (has_full_save) {  // the save tail: checked by the six-argument save stage that follows
        if (ch < 0 || ch >= 3 + JXLH_MAX_EXTRA_CHANNELS || depth < 1 || depth > bits)
          fail(JXLH_ERR_INVALID_ARGUMENT, "stage '" + stage_display(s) + "': channel or bit depth out of range");
        add_conv(s, ch, bits == 8 ? JXLH_SAVE_U8 : JXLH_SAVE_U16, depth, false, 0.0f, 0.0f);
        tail_seen = true;
        continue;
      }
      if (ch != convert_seen || ch > 2 || (convert_bits && convert_bits != bits)) fail(JXLH_ERR_INVALID_ARGUMENT, "integer conversion: channels 0, 1, 2 with one format");
      if (depth != bits) fail(JXLH_ERR_UNSUPPORTED, "integer output with a bit depth below the sample size");
      convert_bits = bits;
      convert_seen++;
    } else if (const auto* f16 = std::get_if<ConvertF32ToF16Stage>(&s)) {
      if (!has_full_save)
        fail(JXLH_ERR_UNSUPPORTED, "stage '" + stage_display(s) + "' needs the save stage that carries colour type, data format and orientation");
      if (phase < kConvert) enter(kConvert, s);
      if (f16->channel < 0 || f16->channel >= 3 + JXLH_MAX_EXTRA_CHANNELS)
        fail(JXLH_ERR_INVALID_ARGUMENT, "stage '" + stage_display(s) + "': channel out of range");
      if (f16->clamp && !(f16->clamp_min <= f16->clamp_max))
        fail(JXLH_ERR_INVALID_ARGUMENT, "stage '" + stage_display(s) + "': clamp range with min > max or a NaN bound");
      add_conv(s, f16->channel, JXLH_SAVE_F16, 0, f16->clamp, f16->clamp_min, f16->clamp_max);
      tail_seen = true;
    } else if (const auto* sp = std::get_if<SpotColorStage>(&s)) {
      if (!has_full_save)
        fail(JXLH_ERR_UNSUPPORTED, "stage '" + stage_display(s) + "' needs the save stage that carries colour type, data format and orientation");
      // frame/render.rs:793-806: behind blend / extend, in front of premultiplication and every conversion
      if (phase > kConvert || have_save || premul_seen || !convs.empty())
        fail(JXLH_ERR_INVALID_ARGUMENT, "stage '" + stage_display(s) + "' out of the order of Frame::build_render_pipeline");
      if (sp->ec < 0 || sp->ec >= JXLH_MAX_EXTRA_CHANNELS || 3 + sp->ec >= (int)num_channels_ || !lp.extra[sp->ec].bits)
        fail(JXLH_ERR_INVALID_ARGUMENT, "stage '" + stage_display(s) + "': not an extra channel of the list");
      if (spots.size() == JXLH_MAX_EXTRA_CHANNELS) fail(JXLH_ERR_INVALID_ARGUMENT, "more spot colour stages than extra channels");
      jxlh_spot_color sc{};
      sc.ec = (uint32_t)sp->ec;
      for (int k = 0; k < 4; k++) sc.rgba[k] = sp->rgba[k];
      spots.push_back(sc);
      phase = kConvert;
      tail_seen = true;
    } else if (const auto* pm = std::get_if<PremultiplyAlphaStage>(&s)) {
      if (!has_full_save)
        fail(JXLH_ERR_UNSUPPORTED, "stage '" + stage_display(s) + "' needs the save stage that carries colour type, data format and orientation");
      // frame/render.rs:858-866: directly in front of the colour conversions
      if (phase > kConvert || have_save || premul_seen || !convs.empty())
        fail(JXLH_ERR_INVALID_ARGUMENT, "stage '" + stage_display(s) + "' out of the order of Frame::build_render_pipeline");
      if (pm->first_color_channel != 0 || (pm->num_color_channels != 1 && pm->num_color_channels != 3))
        fail(JXLH_ERR_INVALID_ARGUMENT, "stage '" + stage_display(s) + "': colour channels 0 or 0..2");
      const int ec = pm->alpha_channel - 3;
      if (ec < 0 || ec >= JXLH_MAX_EXTRA_CHANNELS || pm->alpha_channel >= (int)num_channels_ || !lp.extra[ec].bits)
        fail(JXLH_ERR_INVALID_ARGUMENT, "stage '" + stage_display(s) + "': the alpha is not an extra channel of the list");
      premul_seen = true;
      premul_alpha = pm->alpha_channel;
      premul_n = pm->num_color_channels;
      phase = kConvert;
      tail_seen = true;
    } else if (const auto* sv = std::get_if<SaveStage>(&s); sv && sv->full) {
      // the save tail: lowers to a jxlh_save_desc.  Saves come in buffer order, the colour one first
      // (frame/render.rs:858-902)
      if (phase < kConvert) enter(kConvert, s);
      const std::string name = "stage '" + stage_display(s) + "'";
      if (!modular_frame && lp.modular != LoweredPipeline::Modular::kNone)
        fail(JXLH_ERR_UNSUPPORTED, name + " on a Modular frame (jxlh_stage_save on the planes instead)");
      if (sv->output_buffer_index != (int)lp.saves.size())
        fail(JXLH_ERR_INVALID_ARGUMENT, name + ": save stages come in output buffer order");
      const DataFormat& df = sv->data_format;
      if (df.format > JXLH_SAVE_F32 || sv->orientation < 1 || sv->orientation > 8)
        fail(JXLH_ERR_INVALID_ARGUMENT, name + ": data format or orientation out of range");
      // the channel list against the colour type (frame/render.rs:851-857, :888-899)
      const bool gray = sv->color_type == ColorType::kGrayscale || sv->color_type == ColorType::kGrayscaleAlpha;
      const bool alpha = sv->color_type == ColorType::kGrayscaleAlpha || sv->color_type == ColorType::kRgba ||
                         sv->color_type == ColorType::kBgra;
      const bool bgr = sv->color_type == ColorType::kBgr || sv->color_type == ColorType::kBgra;
      const std::vector<int>& chs = sv->channels;
      const size_t ncol = gray ? 1 : 3;
      const bool ec_only = sv->color_type == ColorType::kGrayscale && chs.size() == 1 && chs[0] >= 3;
      if (!ec_only) {
        const size_t want = ncol + (alpha && !sv->fill_opaque_alpha ? 1 : 0);
        bool ok = chs.size() == want && (!sv->fill_opaque_alpha || alpha);
        for (size_t k = 0; ok && k < ncol; k++) ok = chs[k] == (int)k;
        if (ok && chs.size() > ncol) ok = chs[ncol] >= 3;
        if (!ok) fail(JXLH_ERR_INVALID_ARGUMENT, name + ": channels, colour type and fill_opaque_alpha disagree");
      }
      for (int ch : chs)
        if (ch >= 3 && (ch >= (int)num_channels_ || ch - 3 >= JXLH_MAX_EXTRA_CHANNELS || !lp.extra[ch - 3].bits))
          fail(JXLH_ERR_INVALID_ARGUMENT, name + ": an extra channel the list never converted to f32");
      if (!ec_only && colour_saved) fail(JXLH_ERR_UNSUPPORTED, name + ": a second save of the colour channels");
      if (ec_only && !colour_saved && (premul_seen || !spots.empty()))
        fail(JXLH_ERR_INVALID_ARGUMENT, name + ": spot colour / premultiply stages without a colour save behind them");
      // conversions: exactly the save's channels, in its format and depth; none for f32 (add_conversion_stages)
      jxlh_save_desc d{};
      d.format = df.format;
      d.bit_depth = df.format <= JXLH_SAVE_U16 ? df.bit_depth : 0;
      for (const Conv& c : convs) {
        bool mine = false;
        for (int ch : chs) mine |= ch == c.channel;
        if (!mine) fail(JXLH_ERR_INVALID_ARGUMENT, "stage '" + c.name + "' converts a channel the following save stage does not save");
      }
      if (df.format == JXLH_SAVE_F32) {
        if (!convs.empty()) fail(JXLH_ERR_INVALID_ARGUMENT, "stage '" + convs[0].name + "' in front of an f32 save stage");
      } else {
        if (df.format <= JXLH_SAVE_U16 && (df.bit_depth < 1 || df.bit_depth > (df.format == JXLH_SAVE_U8 ? 8u : 16u)))
          fail(JXLH_ERR_INVALID_ARGUMENT, name + ": bit depth out of range");
        for (size_t k = 0; k < chs.size(); k++) {
          const Conv* c = nullptr;
          for (const Conv& cv : convs)
            if (cv.channel == chs[k]) c = &cv;
          if (!c) fail(JXLH_ERR_INVALID_ARGUMENT, name + ": channel " + std::to_string(chs[k]) + " has no conversion to the save's format");
          if (c->format != df.format || c->depth != d.bit_depth)
            fail(JXLH_ERR_INVALID_ARGUMENT, "stage '" + c->name + "' and " + name + " disagree on format or bit depth");
          if (k == 0) {
            d.f16_clamp = c->clamp;
            d.f16_clamp_min = c->clamp_min;
            d.f16_clamp_max = c->clamp_max;
          } else if ((bool)d.f16_clamp != c->clamp || (c->clamp && (d.f16_clamp_min != c->clamp_min || d.f16_clamp_max != c->clamp_max))) {
            fail(JXLH_ERR_UNSUPPORTED, "stage '" + c->name + "': one f16 clamp range per save stage");
          }
        }
      }
      convs.clear();
      d.n_channels = (uint32_t)chs.size();
      for (size_t k = 0; k < chs.size(); k++) d.channels[k] = (uint32_t)chs[k];
      if (bgr) std::swap(d.channels[0], d.channels[2]);  // render/save.rs:33-40
      d.fill_opaque_alpha = sv->fill_opaque_alpha;
      d.big_endian = df.big_endian && df.format != JXLH_SAVE_U8;
      d.orientation = sv->orientation;
      if (!ec_only) {
        if (premul_seen && (premul_n != (int)ncol || chs.size() <= ncol || chs[ncol] != premul_alpha))
          fail(JXLH_ERR_INVALID_ARGUMENT, name + ": the premultiply stage in front names other channels");
        d.premultiply = premul_seen;
        d.premultiply_alpha_channel = premul_seen ? (uint32_t)premul_alpha : 0;
        d.n_spot = (uint32_t)spots.size();
        for (size_t i = 0; i < spots.size(); i++) d.spot[i] = spots[i];
        colour_saved = true;
      }
      lp.saves.push_back(d);
      have_save = true;
      tail_seen = true;
      phase = kConvert;  // further conversions and saves (the extra channels' buffers) may follow
    } else if (const auto* sv = std::get_if<SaveStage>(&s)) {
      if (has_full_save) fail(JXLH_ERR_UNSUPPORTED, "stage '" + stage_display(s) + "': the four-argument save stage in a list with a six-argument one");
      enter(kSave, s);
      if (have_save) fail(JXLH_ERR_UNSUPPORTED, "more than one save stage (extra-channel outputs stay on the CPU pipeline)");
      if (sv->channels != std::vector<int>{0, 1, 2} || sv->output_buffer_index != 0) fail(JXLH_ERR_UNSUPPORTED, "save stage other than the colour channels into buffer 0");
      if (sv->bits == 32) {
        if (convert_seen) fail(JXLH_ERR_INVALID_ARGUMENT, "f32 save stage behind an integer conversion");
        if (sv->color_channels != 3) fail(JXLH_ERR_UNSUPPORTED, "planar f32 output has three channels");
      } else {
        if (convert_seen != 3 || convert_bits != sv->bits) fail(JXLH_ERR_INVALID_ARGUMENT, "save format and conversion stages disagree");
        if (sv->color_channels != 3 && sv->color_channels != 4) fail(JXLH_ERR_INVALID_ARGUMENT, "RGB or RGBA");
        lp.output.bits = sv->bits;
        lp.output.channels = sv->color_channels;
        lp.has_output = true;
      }
      have_save = true;
      phase = kDone;
    }
  }
  // consistency of the whole list
  if (lp.modular == LoweredPipeline::Modular::kToF32 && modular_seen != 3) fail(JXLH_ERR_INVALID_ARGUMENT, "Modular -> f32 conversion on some channels only");
  if (modular_frame) {
    // the frame runs through jxlh_frame_run: every stage the VarDCT list may hold is served; the I32 -> U8 special case
    // stays with build_modular
    if (lp.modular == LoweredPipeline::Modular::kNone) fail(JXLH_ERR_INVALID_ARGUMENT, "the stage list holds no Modular conversion");
    p.flags |= JXLH_FRAME_MODULAR;
    if (lp.modular == LoweredPipeline::Modular::kXybToF32) {
      if (p.hshift[0] | p.hshift[1] | p.hshift[2] | p.vshift[0] | p.vshift[1] | p.vshift[2])
        fail(JXLH_ERR_INVALID_ARGUMENT, "chroma subsampling on an XYB Modular frame");
      lp.modular_sample_format = JXLH_MODULAR_XYB;
      for (int c = 0; c < 3; c++) p.lf_quant_factors[c] = lp.modular_quant_factors[c];
    } else {
      lp.modular_sample_format = lp.modular_bits;
    }
  } else if (lp.modular != LoweredPipeline::Modular::kNone) {
    // what this path runs for a Modular frame: the conversion, Gaborish / EPF with the constant sigma of
    // features/epf.rs:81-84 (jxlh_modular_frame_filters), then either the planes themselves or -- the builder's special
    // case -- straight to bytes
    if (p.upsampling != 1 || p.noise || p.hshift[0] | p.hshift[1] | p.hshift[2] | p.vshift[0] | p.vshift[1] | p.vshift[2])
      fail(JXLH_ERR_UNSUPPORTED, "upsampling / noise / chroma subsampling on a Modular frame");
    const bool untouched = !p.gab && p.epf_iters == 0 && !have_colour && !have_tf;
    if (convert_seen == 3) {
      // builder.rs:152-170: ConvertModularToF32(c, d) whose next use is ConvertF32ToU8(c, b) with b % d == 0 becomes
      // ConvertI32ToU8Stage(c, ((1 << b) - 1) / ((1 << d) - 1), (1 << b) - 1) and the second stage disappears
      if (lp.modular == LoweredPipeline::Modular::kToF32 && untouched && convert_bits == 8 && 8 % lp.modular_bits == 0) {
        lp.modular = LoweredPipeline::Modular::kI32ToU8;
        lp.i32_to_u8_multiplier = 255 / ((1 << lp.modular_bits) - 1);
        lp.i32_to_u8_max = 255;
      } else {
        fail(JXLH_ERR_UNSUPPORTED, "integer output of a Modular frame other than the I32 -> U8 special case");
      }
    } else if (have_colour || have_tf) {
      fail(JXLH_ERR_UNSUPPORTED, "colour stages on a Modular frame");
    }
  }
  if (p.gab && !(gab_seen[0] && gab_seen[1] && gab_seen[2])) fail(JXLH_ERR_INVALID_ARGUMENT, "Gaborish on some channels only");
  if (p.epf_iters == 3 && !(epf1_seen && epf2_seen)) fail(JXLH_ERR_UNSUPPORTED, "EPF0 without EPF1 and EPF2 (epf_iters >= 3 runs all three)");
  if (ups_seen != 0 && ups_seen != 3) fail(JXLH_ERR_INVALID_ARGUMENT, "frame upsampling on some channels only");
  if ((size_t)ups_factor != (ups_factor ? (size_t)1 << downsampling_shift_ : 0) && ups_factor != 0) fail(JXLH_ERR_INVALID_ARGUMENT, "upsampling factor and downsampling_shift disagree");
  if (!ups_factor && downsampling_shift_ != 0) fail(JXLH_ERR_INVALID_ARGUMENT, "downsampling_shift without upsampling stages");
  if (conv_seen != 0 && !p.noise) fail(JXLH_ERR_INVALID_ARGUMENT, "noise convolution without AddNoise");
  if (!lp.saves.empty()) {
    if (!convs.empty()) fail(JXLH_ERR_INVALID_ARGUMENT, "stage '" + convs[0].name + "' without a save stage behind it");
    if ((premul_seen || !spots.empty()) && !colour_saved)
      fail(JXLH_ERR_INVALID_ARGUMENT, "spot colour / premultiply stages without a save of the colour channels");
    convert_seen = 0;  // the tail's conversions were checked by their save stages
  }
  if (convert_seen != 0 && convert_seen != 3) fail(JXLH_ERR_INVALID_ARGUMENT, "integer conversion on some channels only");
  if (!have_save) fail(JXLH_ERR_INVALID_ARGUMENT, "no save stage");
  if (lp.has_output && lp.output.color == JXLH_COLOR_NONE && have_tf) fail(JXLH_ERR_INVALID_ARGUMENT, "transfer function without colour stage");
  if (expect_extend) fail(JXLH_ERR_INVALID_ARGUMENT, "blending stage without the extend stage behind it");
  if (lp.has_blend) {  // the colour stage runs inside jxlh_frame_blend; the conversion reads the composed image as it is
    lp.blend_colour = lp.output;
    lp.output.color = JXLH_COLOR_NONE;
    lp.output.transfer = JXLH_TF_LINEAR;
  }
  // size = FrameHeader::size_upsampled() (builder.rs:70-85): the frame itself is size >> downsampling_shift
  const uint32_t n = p.upsampling;
  if (size_.first == 0 || size_.second == 0) fail(JXLH_ERR_INVALID_ARGUMENT, "empty frame");
  p.xsize_upsampled = n > 1 ? (uint32_t)size_.first : 0;
  p.ysize_upsampled = n > 1 ? (uint32_t)size_.second : 0;
  if (n > 1) {
    if ((size_.first + n - 1) / n != p.xsize || (size_.second + n - 1) / n != p.ysize)
      fail(JXLH_ERR_INVALID_ARGUMENT, "size_upsampled does not belong to the base frame size");
  } else if (size_.first != p.xsize || size_.second != p.ysize) {
    fail(JXLH_ERR_INVALID_ARGUMENT, "pipeline size and frame size disagree");
  }
  lp.input_border = border;
  lp.out_w = lp.has_blend ? lp.blend.image_w : (uint32_t)size_.first;
  lp.out_h = lp.has_blend ? lp.blend.image_h : (uint32_t)size_.second;
  return lp;
}

// What GpuRenderPipeline and GpuModularFramePipeline share: the frame begun on the context with the lowered parameters,
// its dictionary and splines, the extra channels, and the output side -- blend, save, read.
class GpuFramePipeline {
 public:
  GpuFramePipeline(Context& ctx, LoweredPipeline lp) : ctx_(ctx), lp_(std::move(lp)), frame_(ctx, lp_.frame) {
    const float* const* w = lp_.weights_by_factor;
    if (w[0] || w[1] || w[2])  // CustomTransformData::weights{2,4,8} of the factors in use; the others keep their state
      ctx_.check(jxlh_set_upsampling_weights(ctx_.raw(), w[0], w[1], w[2]), "jxlh_set_upsampling_weights");
    if (lp_.has_patches) frame_.decode_patches(lp_.patches.patches, lp_.patches.blendings, lp_.patches.ec_flags);
    if (lp_.has_splines) frame_.set_spline_segments(lp_.splines.segments);
  }
  VarDctFrame& frame() { return frame_; }  // decode_hf_global / decode_lf_group / decode_hf_metadata go here
  const LoweredPipeline& lowered() const { return lp_; }
  // render/mod.rs:141-144: nothing of the frame lies outside what the groups cover on this path
  void render_outside_frame() {}
  // render/mod.rs:138: the caller's buffer must hold out_height rows of out_width * channels samples
  void check_buffer_sizes(size_t bytes_per_row, size_t rows) const {
    const size_t need = lp_.has_output ? (size_t)lp_.out_w * lp_.output.channels * (lp_.output.bits / 8)
                                       : (size_t)lp_.out_w * sizeof(float);
    if (bytes_per_row < need || rows < lp_.out_h)
      throw Error(JXLH_ERR_INVALID_ARGUMENT, "GpuRenderPipeline::check_buffer_sizes", "output buffer too small");
  }
  // ... of output buffer `buffer_index` of a list with six-argument save stages: the ORIENTED image
  void check_buffer_sizes(size_t buffer_index, size_t bytes_per_row, size_t rows) const {
    const jxlh_save_desc& d = save_desc(buffer_index);
    const bool t = d.orientation >= 5;
    const size_t bps = d.format == JXLH_SAVE_U8 ? 1 : d.format == JXLH_SAVE_F32 ? 4 : 2;
    const size_t need = (size_t)(t ? lp_.out_h : lp_.out_w) * (d.n_channels + (d.fill_opaque_alpha ? 1 : 0)) * bps;
    if (bytes_per_row < need || rows < (t ? lp_.out_w : lp_.out_h))
      throw Error(JXLH_ERR_INVALID_ARGUMENT, "GpuRenderPipeline::check_buffer_sizes", "output buffer too small");
  }
  // the save stage: interleaved integers through the colour tail, or the three f32 planes
  void save(void* out) {
    if (lp_.has_output) frame_.read_output(lp_.output, out);
    else throw Error(JXLH_ERR_INVALID_ARGUMENT, "GpuRenderPipeline::save", "planar f32 pipeline: use save_planes");
  }
  // a six-argument save stage: output buffer `buffer_index` (host or device memory, the origin of the whole oriented
  // image), source rows [y0, y1)
  void save(size_t buffer_index, void* out, size_t bytes_per_row, uint32_t y0 = 0, uint32_t y1 = 0xFFFFFFFFu) {
    frame_.save(&lp_.output, save_desc(buffer_index), out, bytes_per_row, y0, y1);
  }
  // ... only the pixels of `rects` (source rectangles of the result), e.g. what changed_rects() names after a pass
  void save_rects(size_t buffer_index, const std::vector<jxlh_rect>& rects, void* out, size_t bytes_per_row) {
    frame_.save_rects(&lp_.output, save_desc(buffer_index), rects, out, bytes_per_row);
  }
  void save_planes(float* c0, float* c1, float* c2) { frame_.read_planes(c0, c1, c2); }
  // an LF frame's result (lf_level = L) into LF slot L - 1, where the reference's list has its three Grayscale f32 save
  // stages (frame/render.rs:699-710); those stages are not lowered
  void save_lf(uint32_t slot) { frame_.save_lf(slot); }
  // An extra channel's integer samples as the Modular decoder leaves them (w x h at the channel's own resolution, host
  // or device memory).  The stage list decides what happens to them: ConvertModularToF32Stage with the channel's bit
  // depth, then its Upsample stage if it has one; both run inside do_render() behind the colour channels' stages.
  void set_extra_channel_buffer(uint32_t ec, const int32_t* samples, size_t stride, uint32_t w, uint32_t h) {
    if (ec >= JXLH_MAX_EXTRA_CHANNELS || !lp_.extra[ec].bits)
      throw Error(JXLH_ERR_INVALID_ARGUMENT, "GpuRenderPipeline::set_extra_channel_buffer", "the stage list does not name this extra channel");
    ctx_.check(jxlh_frame_set_extra_channel(ctx_.raw(), ec, samples, stride, w, h, lp_.extra[ec].bits, lp_.extra[ec].upsampling),
               "jxlh_frame_set_extra_channel");
  }
  // the save stage of an extra channel: one f32 plane of the frame's output size (out_width() x out_height())
  void save_extra_channel(uint32_t ec, float* out, size_t stride) {
    jxlh_plane pl{out, (size_t)frame_.out_width() * sizeof(float), frame_.out_height(), stride * sizeof(float)};
    ctx_.check(jxlh_frame_read_extra_channel(ctx_.raw(), ec, &pl), "jxlh_frame_read_extra_channel");
  }

 protected:
  // BlendingStage + extend (with the list's colour stage in front): the image becomes what the save stages read
  void blend_if_listed() {
    if (lp_.has_blend) frame_.blend(lp_.blend, &lp_.blend_colour);
  }
  const jxlh_save_desc& save_desc(size_t buffer_index) const {
    if (buffer_index >= lp_.saves.size())
      throw Error(JXLH_ERR_INVALID_ARGUMENT, "GpuRenderPipeline::save", "the stage list has no save stage for this buffer");
    return lp_.saves[buffer_index];
  }
  Context& ctx_;
  LoweredPipeline lp_;
  VarDctFrame frame_;
};

// RenderPipeline (render/mod.rs:116-157) for this path: inputs are a group's coefficient slabs instead of its pixel
// buffers (the transforms run on the device too), everything else keeps the trait's meaning.
class GpuRenderPipeline : public GpuFramePipeline {
 public:
  using GpuFramePipeline::GpuFramePipeline;
  // render/mod.rs:128-136.  complete = false: a progressive pass that leaves the group open
  void set_buffer_for_group(uint32_t group_id, bool complete, const int32_t* coeffs, int slot = 0) {
    ctx_.check(jxlh_submit_group(ctx_.raw(), slot, group_id, coeffs, complete ? JXLH_GROUP_COMPLETE : 0u), "jxlh_submit_group");
    // the reference renders every group it is handed (render/mod.rs:128-136): once the frame has been rendered, a group
    // that receives new coefficients is re-rendered whether or not the caller also marks it (duplicates are merged by
    // jxlh_frame_rerender_groups)
    if (!dirty_first_) rerender_.push_back(group_id);
  }
  // render/mod.rs:146
  void mark_group_to_rerender(uint32_t g) { rerender_.push_back(g); }
  // The rectangles of the frame's result that re-rendering `groups` can change (jxlh_changed_rects): what save_rects
  // repaints after the do_render() of a pass that touched them.  Frame coordinates: with a BlendingStage in the list,
  // shift them by the frame's origin and clip them to the image.
  std::vector<jxlh_rect> changed_rects(const std::vector<uint32_t>& groups) const { return frame_.changed_rects(groups); }
  // A group that must be rendered while its HF has not arrived (force_render with DataStatus::Zero, frame/decode.rs:
  // 744-752): the reference hands the pipeline the LF image upsampled 8x as the group's buffers; here the group is marked
  // and the next do_render() fills it on the device.  set_buffer_for_group on the group later clears the mark.
  void set_lf_only_group(uint32_t group_id) {
    frame_.upsample_lf_groups(&group_id, 1);
    if (!dirty_first_) rerender_.push_back(group_id);
  }
  // what the reference does when the last group of a pass has been handed over (frame/decode.rs:547-558, :703-711)
  void do_render() {
    for (int s = 0; s < ctx_.n_slots(); s++) ctx_.check(jxlh_slot_wait(ctx_.raw(), s), "jxlh_slot_wait");
    if (!rerender_.empty() && !dirty_first_) {
      ctx_.check(jxlh_frame_rerender_groups(ctx_.raw(), rerender_.data(), (uint32_t)rerender_.size()), "jxlh_frame_rerender_groups");
    } else {
      frame_.finalize_and_render();
    }
    blend_if_listed();
    dirty_first_ = false;
    rerender_.clear();
  }

 private:
  std::vector<uint32_t> rerender_;
  bool dirty_first_ = true;
};

// A Modular frame as a frame of the context (lower_modular_frame): the samples come out of the Modular inverse
// transforms (jxlh_rct, jxlh_palette*, jxlh_unsqueeze_chain) as three i32 planes, host or device memory, and go in rect
// by rect; render() is the whole stage list behind jxlh_frame_run, and the output side is GpuRenderPipeline's.
class GpuModularFramePipeline : public GpuFramePipeline {
 public:
  GpuModularFramePipeline(Context& ctx, LoweredPipeline lp) : GpuFramePipeline(ctx, std::move(lp)) {
    if (!(lp_.frame.flags & JXLH_FRAME_MODULAR))
      throw Error(JXLH_ERR_INVALID_ARGUMENT, "GpuModularFramePipeline", "the list was not lowered by lower_modular_frame");
  }
  // one rect of the three colour channels (coded order Y, X, B for an XYB list; one pointer three times for a grey
  // frame), full-resolution coordinates, row stride in samples
  void set_channels(uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const int32_t* const planes[3], size_t stride) {
    frame_.set_modular_channels(x0, y0, w, h, planes, stride, lp_.modular_sample_format);
  }
  // the batched intake: many groups as decoded, each with its local transform list (jxlh_frame_set_modular_groups);
  // what a group's list holds that the device does not take comes back as JXLH_ERR_UNSUPPORTED before anything ran, and
  // that group goes through set_channels after the host's local_apply
  void set_groups(const int32_t* arena, uint64_t arena_samples, const std::vector<jxlh_local_group>& groups, bool async = false) {
    frame_.set_modular_groups(arena, arena_samples, groups.data(), groups.size(), lp_.modular_sample_format, async);
  }
  // the whole frame, then the list's blending
  void render() {
    frame_.finalize_and_render();
    blend_if_listed();
  }
  // 256-row bands [band0, band1) (a list with blending or frame upsampling renders whole)
  void render_band(uint32_t band0, uint32_t band1) {
    if (lp_.has_blend) throw Error(JXLH_ERR_UNSUPPORTED, "GpuModularFramePipeline::render_band", "a blended frame is rendered whole");
    frame_.finalize_and_render(band0, band1);
  }
};

// A Modular frame's stage list on the device: the samples come out of the Modular inverse transforms (jxlh_rct,
// jxlh_palette*, jxlh_unsqueeze_chain) as three i32 planes, host or device memory.
class GpuModularPipeline {
 public:
  GpuModularPipeline(Context& ctx, LoweredPipeline lp) : ctx_(ctx), lp_(std::move(lp)) {
    if (lp_.modular == LoweredPipeline::Modular::kNone)
      throw Error(JXLH_ERR_INVALID_ARGUMENT, "GpuModularPipeline", "the stage list holds no Modular conversion");
  }
  const LoweredPipeline& lowered() const { return lp_; }
  // the batched intake of the caller-held-planes form (jxlh_modular_local_transforms): every group's local transforms,
  // finished channels into `planes` (n_planes DEVICE planes of the frame's size) at the group's rect, one launch
  void local_transforms(const int32_t* arena, uint64_t arena_samples, const std::vector<jxlh_local_group>& groups,
                        uint32_t bit_depth, int32_t* const planes[], uint32_t n_planes, size_t stride) {
    size_t bad = 0;
    ctx_.check(jxlh_modular_local_transforms(ctx_.raw(), arena, arena_samples, groups.data(), groups.size(), bit_depth, planes,
                                             n_planes, lp_.frame.xsize, lp_.frame.ysize, stride, &bad),
               "jxlh_modular_local_transforms");
  }
  // ConvertI32ToU8Stage: interleaved bytes (3 or 4 per pixel) in one pass
  void render_u8(const int32_t* const planes[3], size_t stride, void* out, size_t bytes_per_row) {
    if (lp_.modular != LoweredPipeline::Modular::kI32ToU8)
      throw Error(JXLH_ERR_INVALID_ARGUMENT, "GpuModularPipeline::render_u8", "not the I32 -> U8 special case");
    ctx_.check(jxlh_modular_to_rgb8(ctx_.raw(), planes, stride, lp_.frame.xsize, lp_.frame.ysize, lp_.i32_to_u8_multiplier,
                                    lp_.i32_to_u8_max, lp_.output.channels, out, bytes_per_row),
               "jxlh_modular_to_rgb8");
  }
  // conversion to f32 and, if the list holds them, Gaborish / EPF with the frame's constant sigma
  // (jxlh_modular_frame_filters: device planes, 16-byte aligned, row stride a multiple of 4 floats, tmp != out).
  // in[] in coded order for an XYB frame (Y, X, B); the result (X, Y, B) lands in out[]; tmp[] is only used when the
  // list holds filters.  Planes are tight: stride = xsize, which must then be a multiple of 4.
  void render_f32(const int32_t* const in[3], float* const tmp[3], float* const out[3]) {
    const size_t w = lp_.frame.xsize, h = lp_.frame.ysize, n = w * h;
    const bool filters = lp_.frame.gab || lp_.frame.epf_iters;
    float* const* dst = filters ? tmp : out;
    if (lp_.modular == LoweredPipeline::Modular::kXybToF32) {
      ctx_.check(jxlh_modular_xyb_to_f32(ctx_.raw(), in[0], in[1], in[2], n, lp_.modular_quant_factors.data(), dst[0], dst[1], dst[2]),
                 "jxlh_modular_xyb_to_f32");
    } else if (lp_.modular == LoweredPipeline::Modular::kToF32) {
      for (int c = 0; c < 3; c++)
        ctx_.check(jxlh_modular_to_f32(ctx_.raw(), in[c], n, lp_.modular_bits, dst[c]), "jxlh_modular_to_f32");
    } else {
      throw Error(JXLH_ERR_INVALID_ARGUMENT, "GpuModularPipeline::render_f32", "the list lowers to the I32 -> U8 special case");
    }
    if (filters) {
      if (w % 4) throw Error(JXLH_ERR_UNSUPPORTED, "GpuModularPipeline::render_f32", "filters need a row length that is a multiple of 4 samples");
      ctx_.check(jxlh_modular_frame_filters(ctx_.raw(), &lp_.frame, tmp, out, (uint32_t)w, (uint32_t)h, w), "jxlh_modular_frame_filters");
    }
  }

 private:
  Context& ctx_;
  LoweredPipeline lp_;
};

inline std::unique_ptr<GpuRenderPipeline> RenderPipelineBuilder::build(Context& ctx) && {
  return std::make_unique<GpuRenderPipeline>(ctx, lower());
}

inline std::unique_ptr<GpuModularPipeline> RenderPipelineBuilder::build_modular(Context& ctx) && {
  return std::make_unique<GpuModularPipeline>(ctx, lower());
}

inline std::unique_ptr<GpuModularFramePipeline> RenderPipelineBuilder::build_modular_frame(Context& ctx) && {
  return std::make_unique<GpuModularFramePipeline>(ctx, lower_modular_frame());
}

}  // namespace jxlh
