// fsr_formats.h -- what an ovrfsr_image::format value means to the host code, in one place: the launch manager (postprocessor.cpp), the
// capture writers (config_json.cpp) and the host half of the resolve launcher (fsr_kernels.hip).  Host only; the kernels take their
// formats as template parameters (fsr_params.h, whose FMT_* values are the header's).  A new input format is a row in each function here.
#pragma once
#include <stdint.h>
#include "../../include/openvr_fsr_amd.h"
#include "fsr_params.h"

namespace ovrfsr {

static_assert(FMT_RGBA8 == OVRFSR_FORMAT_RGBA8_UNORM && FMT_RGBA16F == OVRFSR_FORMAT_RGBA16F && FMT_RGBA32F == OVRFSR_FORMAT_RGBA32F &&
              FMT_RGB10A2 == OVRFSR_FORMAT_RGB10A2_UNORM && FMT_BGRA8 == OVRFSR_FORMAT_BGRA8_UNORM && FMT_R11G11B10F == OVRFSR_FORMAT_R11G11B10F &&
              FMT_RGBA8_MS4 == OVRFSR_FORMAT_MS(OVRFSR_FORMAT_RGBA8_UNORM, 4), "the launchers take ovrfsr_format values as they are");

// ovrfsr_image::format = base format | samples << OVRFSR_FORMAT_SAMPLES_SHIFT (header: multisampled input); samples 0 and 1 both mean one
constexpr uint32_t base_format(uint32_t fmt) { return fmt & ((1u << OVRFSR_FORMAT_SAMPLES_SHIFT) - 1u); }
constexpr uint32_t format_samples(uint32_t fmt) { return (fmt >> OVRFSR_FORMAT_SAMPLES_SHIFT) > 1u ? fmt >> OVRFSR_FORMAT_SAMPLES_SHIFT : 1u; }

// bytes of one texel (one SAMPLE of a multisampled image).  For a format the caller has validated (CheckImage, the capture writers' own
// test): an unassigned base value (5, 7, ...) has no texel size, and the 4 it gets here means nothing.
constexpr uint32_t texel_bytes(uint32_t fmt)
{
    return base_format(fmt) == OVRFSR_FORMAT_RGBA16F ? 8u : base_format(fmt) == OVRFSR_FORMAT_RGBA32F ? 16u : 4u;
}

// What the kernels see in a submission's place once the resolve pass or the BGRA8 re-order has run (PostProcessor::ApplyPostProcess): a
// multisampled image resolved to one sample, BGRA8 re-ordered to RGBA8 (the reference reads it through a typed view and writes R8G8B8A8,
// PostProcessor.cpp:30-61,63-74), R11G11B10F unpacked to RGBA16F.  With cfg.reference_formats = 0 (the default: this library's own rule,
// BASELINE C5's packed-half I/O -- NOT the reference's) it is also the format of the quantised intermediate and of the ctx-owned output.
constexpr uint32_t pipeline_format(uint32_t fmt)
{
    return base_format(fmt) == OVRFSR_FORMAT_BGRA8_UNORM ? (uint32_t)OVRFSR_FORMAT_RGBA8_UNORM
         : base_format(fmt) == OVRFSR_FORMAT_R11G11B10F ? (uint32_t)OVRFSR_FORMAT_RGBA16F : base_format(fmt);
}

// The reference's DetermineOutputFormat (PostProcessor.cpp:63-74), the format of BOTH textures it creates (upscaledTexture :340-352,
// sharpenedTexture :462-475): R10G10B10A2_UNORM for a 10-bit submission, R8G8B8A8_UNORM for everything else -- RGBA16F, RGBA32F and
// R11G11B10F included.  `fmt`: a pipeline_format value.  cfg.reference_formats = 1 selects it (header).
constexpr uint32_t reference_output_format(uint32_t fmt)
{
    return fmt == OVRFSR_FORMAT_RGB10A2_UNORM ? (uint32_t)OVRFSR_FORMAT_RGB10A2_UNORM : (uint32_t)OVRFSR_FORMAT_RGBA8_UNORM;
}

// nullptr, or why an image of this format cannot be a destination
constexpr const char *input_only(uint32_t fmt)
{
    return base_format(fmt) == OVRFSR_FORMAT_R11G11B10F ? "R11G11B10F is an input-only format"
         : format_samples(fmt) > 1u ? "multisampled images are input-only"
         : base_format(fmt) == OVRFSR_FORMAT_BGRA8_UNORM ? "BGRA8 is an input-only format" : nullptr;
}

} // namespace ovrfsr
