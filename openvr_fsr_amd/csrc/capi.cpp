// capi.cpp -- the C ABI declared in include/openvr_fsr_amd.h over ovrfsr::PostProcessor.
// No exception crosses this boundary (the reference swallows failures the same way,
// PostProcessor.cpp:145-152).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include "postprocessor.hpp"
#include "fsr_launch.h"
#include "fsr_bounds.h"
#include "hdr_map.h"
#include "mask_feather.h"
#include "nis_tables.h"

struct ovrfsr_ctx {
    ovrfsr::PostProcessor *pp;
};

namespace {
bool config_ok(const ovrfsr_config *cfg) { return cfg && cfg->struct_size == sizeof(ovrfsr_config); }
// what create / set_config accept: a ctx is never built around a configuration no kernel exists for (and so never
// disables itself over one at the first apply)
// The float fields feed float -> uint32 conversions (mask centre and radius, PostProcessor.cpp:298-305) and clamps: a ctx is only ever built
// around values for which every one of them is defined (header, "Configuration values").  The reference validates none of this -- its only
// rule is `if (sharpness < 0) sharpness = 0` (Config.h:40) -- and is undefined for the values refused here.
bool floats_valid(const ovrfsr_config *cfg)
{
    if (!std::isfinite(cfg->radius) || cfg->radius < 0.0f) return false;
    if (!std::isfinite(cfg->sharpness) || !std::isfinite(cfg->render_scale)) return false;
    for (int i = 0; i < 4; ++i)
        if (!(cfg->proj_centre[i] >= -1.0f && cfg->proj_centre[i] <= 2.0f)) return false; // NaN fails the comparison
    return true;
}
bool config_valid(const ovrfsr_config *cfg)
{
    return config_ok(cfg) && (cfg->precision == OVRFSR_PRECISION_FP32 || cfg->precision == OVRFSR_PRECISION_FP32_STRICT || cfg->precision == OVRFSR_PRECISION_FP32_EXACT) &&
           cfg->stage_mask >= 0 && cfg->stage_mask <= 2 && cfg->fused >= -1 && cfg->fused <= 1 && (cfg->pair_submit == 0 || cfg->pair_submit == 1) &&
           (cfg->reference_formats == 0 || cfg->reference_formats == 1) && floats_valid(cfg);
}

// Nothing may unwind through the extern "C" boundary (header: "nothing here throws"): host-side containers of the launch
// manager can throw std::bad_alloc, which becomes a status like every other failure.
template <typename F>
int guarded(F &&f) noexcept
{
    try {
        return f();
    } catch (const std::bad_alloc &) {
        return OVRFSR_ERR_OUT_OF_MEMORY;
    } catch (...) {
        return OVRFSR_ERR_INVALID_ARGUMENT;
    }
}
} // namespace

extern "C" {

OVRFSR_API uint32_t ovrfsr_abi_version(void) { return OVRFSR_ABI_VERSION; }

#ifdef OVRFSR_TIE_AUDIT
// AUDIT BUILDS ONLY (-DOVRFSR_TIE_AUDIT; not part of the ABI, not declared in include/openvr_fsr_amd.h, absent from the shipped library):
// the current device's near-tie audit counters {audited, listed, flips, small-channel half differences, max distance bytes (fp32 bits),
// max distance half spacings (fp32 bits)} -- see g_ovrfsr_tie_audit in fsr_kernels.hip.  tools/debug/tie_audit.py drives it.
OVRFSR_API int ovrfsr_debug_tie_audit(unsigned long long counts[6], int reset)
{
    return ovrfsr::tie_audit_read(counts, reset != 0) == hipSuccess ? OVRFSR_OK : OVRFSR_ERR_HIP;
}
// the exact-stores RCAS instances (OVRFSR_PRECISION_FP32_EXACT): {audited, listed, flips, max |product - reference-order| in bytes (fp32 bits),
// K of the band 2^-K byte the kernels were built with} -- g_ovrfsr_tie_audit_rcas in fsr_kernels.hip.  tools/debug/tie_audit.py --rcas drives it.
OVRFSR_API int ovrfsr_debug_tie_audit_rcas(unsigned long long counts[5], int reset)
{
    return ovrfsr::tie_audit_read_rcas(counts, reset != 0) == hipSuccess ? OVRFSR_OK : OVRFSR_ERR_HIP;
}
#endif

#ifdef OVRFSR_BOUNDS
// CHECKED BUILDS ONLY (-DOVRFSR_BOUNDS, fsr_bounds.h; not part of the ABI, not declared in include/openvr_fsr_amd.h, absent from the shipped
// library): the current device's checked-accessor counters, summed over the three kernel translation units, n = ovrfsr_chk::kSlots values
// (layout: fsr_bounds.h); and the self-test launch.  tests/test_gpu_bounds.py drives them.
OVRFSR_API int ovrfsr_debug_bounds_slots(void) { return ovrfsr_chk::kSlots; }
OVRFSR_API int ovrfsr_debug_bounds(unsigned long long *counts, int n, int reset)
{
    if (!counts || n != ovrfsr_chk::kSlots) return OVRFSR_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < n; ++i) counts[i] = 0;
    if (ovrfsr::bounds_read_fsr(counts, reset != 0) != hipSuccess) return OVRFSR_ERR_HIP;
    if (ovrfsr::bounds_read_packed(counts, reset != 0) != hipSuccess) return OVRFSR_ERR_HIP;
    return ovrfsr::bounds_read_nis(counts, reset != 0) == hipSuccess ? OVRFSR_OK : OVRFSR_ERR_HIP;
}
OVRFSR_API int ovrfsr_debug_bounds_selftest(void) { return ovrfsr::bounds_selftest() == hipSuccess ? OVRFSR_OK : OVRFSR_ERR_HIP; }
// fault injection (checked builds only): the nth device allocation / stream / event creation of the launch manager from now on fails, once; 0 disarms
OVRFSR_API void ovrfsr_debug_fail_resource(int nth) { ovrfsr::debug_fail_resource(nth); }
// dynamic resolution (checked builds only): the route a re-scale refills the tap tables by from now on -- 1: host-built taps through a staging
// slot, 0: tap_tables_kernel --, and the device tap tables read back (bytes: 8 x (outW rounded up to 32 + outH + 64))
OVRFSR_API void ovrfsr_debug_tap_route(int upload) { ovrfsr::debug_tap_route(upload); }
OVRFSR_API int ovrfsr_debug_read_taps(ovrfsr_ctx *ctx, void *dst, size_t bytes)
{
    if (!ctx || !dst) return OVRFSR_ERR_INVALID_ARGUMENT;
    return guarded([&] { return ctx->pp->DebugReadTaps(dst, bytes); });
}
#endif

OVRFSR_API int ovrfsr_pair_pending(const ovrfsr_ctx *ctx) { return ctx && ctx->pp && ctx->pp->PairPending() ? 1 : 0; }

// ---- hidden-area mesh (header).  The argument checks live here: the planner's refusal table knows nothing of meshes.
namespace {
constexpr uint32_t kMaxHiddenTriangles = 4096;
bool mesh_ok(const float *uv, uint32_t triangle_count)
{
    if (triangle_count > kMaxHiddenTriangles || (!uv && triangle_count)) return false;
    for (size_t i = 0; i < 6 * (size_t)triangle_count; ++i)
        if (!std::isfinite(uv[i])) return false;
    return true;
}
} // namespace

OVRFSR_API int ovrfsr_set_hidden_area(ovrfsr_ctx *ctx, int eye, const float *uv, uint32_t triangle_count)
{
    if (!ctx || (eye != OVRFSR_EYE_LEFT && eye != OVRFSR_EYE_RIGHT) || !mesh_ok(uv, triangle_count)) return OVRFSR_ERR_INVALID_ARGUMENT; // the stored mesh stays
    return guarded([&] { return ctx->pp->SetHiddenArea(eye, uv, triangle_count); });
}

OVRFSR_API int ovrfsr_hidden_area_stats(const ovrfsr_ctx *ctx, int eye, uint32_t *tiles_total, uint32_t *tiles_skipped)
{
    if (!ctx || (eye != OVRFSR_EYE_LEFT && eye != OVRFSR_EYE_RIGHT) || !tiles_total || !tiles_skipped) return OVRFSR_ERR_INVALID_ARGUMENT;
    return guarded([&] { return ctx->pp->HiddenAreaStats(eye, tiles_total, tiles_skipped); });
}

OVRFSR_API int ovrfsr_hidden_tiles(const float *uv, uint32_t triangle_count, uint32_t out_w, uint32_t out_h, uint32_t tile_w, uint32_t tile_h,
                                   uint8_t *hidden, size_t hidden_len)
{
    if (!mesh_ok(uv, triangle_count) || !hidden || out_w == 0 || out_h == 0 || out_w > 16384 || out_h > 16384 || tile_w == 0 || tile_h == 0 ||
        tile_w > 16384 || tile_h > 16384)
        return OVRFSR_ERR_INVALID_ARGUMENT;
    const size_t tiles = (size_t)((out_w + tile_w - 1) / tile_w) * ((out_h + tile_h - 1) / tile_h);
    if (hidden_len < tiles) return OVRFSR_ERR_INVALID_ARGUMENT; // (nothing written)
    return guarded([&] {
        ovrfsr::hidden_tiles(uv, triangle_count, nullptr, 0, false, out_w, out_h, tile_w, tile_h, hidden);
        return (int)OVRFSR_OK;
    });
}

// ---- HDR domain (header).  The argument checks live here, like the mesh's.
OVRFSR_API int ovrfsr_set_hdr_domain(ovrfsr_ctx *ctx, int domain)
{
    if (!ctx || (domain != OVRFSR_HDR_DOMAIN_LINEAR && domain != OVRFSR_HDR_DOMAIN_SRTM)) return OVRFSR_ERR_INVALID_ARGUMENT; // the stored value stays
    return guarded([&] { return ctx->pp->SetHdrDomain(domain); });
}

OVRFSR_API int ovrfsr_get_hdr_domain(const ovrfsr_ctx *ctx, int *domain)
{
    if (!ctx || !domain) return OVRFSR_ERR_INVALID_ARGUMENT;
    *domain = ctx->pp->HdrDomain();
    return OVRFSR_OK;
}

// ---- eye-tracked foveation (header).  The argument checks live here; the setters store, the next apply acts (PostProcessor::AimGaze).
namespace {
bool eye_ok(int eye) { return eye == OVRFSR_EYE_LEFT || eye == OVRFSR_EYE_RIGHT; }
bool centre_ok(float c) { return c >= -1.0f && c <= 2.0f; } // proj_centre's range (floats_valid); NaN and the infinities fail the comparison
} // namespace

OVRFSR_API int ovrfsr_set_gaze(ovrfsr_ctx *ctx, int eye, float x, float y)
{
    if (!ctx || !eye_ok(eye) || !centre_ok(x) || !centre_ok(y)) return OVRFSR_ERR_INVALID_ARGUMENT; // the stored value stays
    ctx->pp->SetGaze(eye, x, y);
    return OVRFSR_OK;
}

OVRFSR_API int ovrfsr_clear_gaze(ovrfsr_ctx *ctx, int eye)
{
    if (!ctx || !eye_ok(eye)) return OVRFSR_ERR_INVALID_ARGUMENT;
    ctx->pp->ClearGaze(eye);
    return OVRFSR_OK;
}

OVRFSR_API int ovrfsr_get_gaze(const ovrfsr_ctx *ctx, int eye, float xy[2], int *is_set)
{
    if (!ctx || !eye_ok(eye) || !xy || !is_set) return OVRFSR_ERR_INVALID_ARGUMENT;
    ctx->pp->GetGaze(eye, xy, is_set);
    return OVRFSR_OK;
}

OVRFSR_API int ovrfsr_gaze_stats(const ovrfsr_ctx *ctx, uint32_t *reaims, uint32_t *rebuilds)
{
    if (!ctx || !reaims || !rebuilds) return OVRFSR_ERR_INVALID_ARGUMENT;
    ctx->pp->GazeStats(reaims, rebuilds);
    return OVRFSR_OK;
}

// ---- dynamic resolution (header).  The argument checks live here; the setter stores, the next apply plans afresh (PostProcessor::SetMaxInputSize).
OVRFSR_API int ovrfsr_set_max_input_size(ovrfsr_ctx *ctx, uint32_t max_width, uint32_t max_height)
{
    if (!ctx || (max_width == 0) != (max_height == 0) || max_width > 16384 || max_height > 16384) return OVRFSR_ERR_INVALID_ARGUMENT; // the stored value stays
    return guarded([&] { return ctx->pp->SetMaxInputSize(max_width, max_height); });
}

OVRFSR_API int ovrfsr_get_max_input_size(const ovrfsr_ctx *ctx, uint32_t *max_width, uint32_t *max_height)
{
    if (!ctx || !max_width || !max_height) return OVRFSR_ERR_INVALID_ARGUMENT;
    ctx->pp->MaxInputSize(max_width, max_height);
    return OVRFSR_OK;
}

OVRFSR_API int ovrfsr_rescale_stats(const ovrfsr_ctx *ctx, uint32_t *rescales, uint32_t *rebuilds)
{
    if (!ctx || !rescales || !rebuilds) return OVRFSR_ERR_INVALID_ARGUMENT;
    ctx->pp->RescaleStats(rescales, rebuilds);
    return OVRFSR_OK;
}

// ---- mask feather (header).  The argument checks live here; the setter stores and nothing else (PostProcessor::SetMaskFeather), so it needs
// no guard: nothing in it allocates or throws.
OVRFSR_API int ovrfsr_set_mask_feather(ovrfsr_ctx *ctx, float width)
{
    if (!ctx || !(width >= 0.0f && width <= 2.0f)) return OVRFSR_ERR_INVALID_ARGUMENT; // (NaN fails both comparisons; the stored value stays)
    ctx->pp->SetMaskFeather(width);
    return OVRFSR_OK;
}

OVRFSR_API int ovrfsr_get_mask_feather(const ovrfsr_ctx *ctx, float *width)
{
    if (!ctx || !width) return OVRFSR_ERR_INVALID_ARGUMENT;
    *width = ctx->pp->MaskFeather();
    return OVRFSR_OK;
}

OVRFSR_API int ovrfsr_mask_feather_stats(const ovrfsr_ctx *ctx, uint32_t *launches)
{
    if (!ctx || !launches) return OVRFSR_ERR_INVALID_ARGUMENT;
    *launches = ctx->pp->MaskFeatherLaunches();
    return OVRFSR_OK;
}

OVRFSR_API int ovrfsr_mask_feather_weights(const uint32_t centre[4], uint32_t radius_px, uint32_t feather_px, uint32_t out_w, uint32_t out_h,
                                           uint16_t *w8, uint8_t *inside, size_t len)
{
    if (!centre || !w8 || !inside || out_w == 0 || out_h == 0 || out_w > 16384 || out_h > 16384 || len < (size_t)out_w * out_h)
        return OVRFSR_ERR_INVALID_ARGUMENT; // (nothing written)
    ovrfsr::FeatherCon fc;
    const bool ramp = ovrfsr::feather_constants(radius_px, feather_px, &fc);
    const uint32_t r2 = radius_px * radius_px; // radius[1], with its wrap-around
    for (uint32_t y = 0; y < out_h; ++y)
        for (uint32_t x = 0; x < out_w; ++x) {
            const size_t i = (size_t)y * out_w + x;
            // (no ramp -- F = 0 or Ro = 0 --: the feather is not active, every pixel keeps its value)
            w8[i] = (uint16_t)(ramp ? ovrfsr::feather_w8(fc, ovrfsr::feather_d2(centre, x, y)) : 256u);
            inside[i] = ovrfsr::feather_group_inside(centre, r2, x, y) ? 1 : 0;
        }
    return OVRFSR_OK;
}

OVRFSR_API int ovrfsr_hdr_map(const float *rgb_in, float *rgb_out, size_t n, int inverse)
{
    if ((n && (!rgb_in || !rgb_out)) || (inverse != 0 && inverse != 1)) return OVRFSR_ERR_INVALID_ARGUMENT; // (nothing written)
    for (size_t i = 0; i < n; ++i) {
        float r = rgb_in[3 * i], g = rgb_in[3 * i + 1], b = rgb_in[3 * i + 2];
        ovrfsr::hdr_map(r, g, b, inverse != 0);
        rgb_out[3 * i] = r; rgb_out[3 * i + 1] = g; rgb_out[3 * i + 2] = b;
    }
    return OVRFSR_OK;
}

OVRFSR_API void ovrfsr_config_default(ovrfsr_config *cfg)
{
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = sizeof(*cfg);
    cfg->fsr_enabled = 0;      // Config.h:11
    cfg->use_nis = 0;          // :17
    cfg->debug_mode = 0;       // :16
    cfg->render_scale = 1.f;   // :13
    cfg->sharpness = 0.75f;    // :14
    cfg->radius = 0.5f;        // :15
    cfg->proj_centre[0] = cfg->proj_centre[1] = cfg->proj_centre[2] = cfg->proj_centre[3] = 0.5f;
    cfg->precision = OVRFSR_PRECISION_FP32;
    cfg->quantize_intermediate = 1;
    cfg->fused = -1;
}

OVRFSR_API int ovrfsr_output_size(const ovrfsr_config *cfg, uint32_t in_w, uint32_t in_h, uint32_t *out_w, uint32_t *out_h)
{
    if (!config_ok(cfg) || !out_w || !out_h) return OVRFSR_ERR_INVALID_ARGUMENT;
    return ovrfsr::plan_output_size(*cfg, in_w, in_h, out_w, out_h);
}

OVRFSR_API int ovrfsr_create(int device, const ovrfsr_config *cfg, ovrfsr_ctx **out_ctx)
{
    if (!out_ctx || !config_valid(cfg)) return OVRFSR_ERR_INVALID_ARGUMENT;
    *out_ctx = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return OVRFSR_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return OVRFSR_ERR_NO_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return OVRFSR_ERR_NO_DEVICE; // kernels are gfx950-only
    return guarded([&] {
        // owned until success: a throwing PostProcessor constructor (its std::string / std::vector members) must not leak the ctx
        std::unique_ptr<ovrfsr_ctx> c(new (std::nothrow) ovrfsr_ctx);
        if (!c) return (int)OVRFSR_ERR_OUT_OF_MEMORY;
        c->pp = nullptr;
        std::unique_ptr<ovrfsr::PostProcessor> pp(new (std::nothrow) ovrfsr::PostProcessor(device, *cfg));
        if (!pp) return (int)OVRFSR_ERR_OUT_OF_MEMORY;
        c->pp = pp.release();
        *out_ctx = c.release();
        return (int)OVRFSR_OK;
    });
}

OVRFSR_API void ovrfsr_destroy(ovrfsr_ctx *ctx)
{
    if (!ctx) return;
    delete ctx->pp;
    delete ctx;
}

OVRFSR_API int ovrfsr_set_config(ovrfsr_ctx *ctx, const ovrfsr_config *cfg)
{
    if (!ctx || !config_valid(cfg)) return OVRFSR_ERR_INVALID_ARGUMENT; // the ctx keeps its previous configuration
    return guarded([&] { return ctx->pp->SetConfig(*cfg); });
}

OVRFSR_API int ovrfsr_get_config(const ovrfsr_ctx *ctx, ovrfsr_config *cfg)
{
    if (!ctx || !cfg) return OVRFSR_ERR_INVALID_ARGUMENT;
    *cfg = ctx->pp->GetConfig();
    return OVRFSR_OK;
}

OVRFSR_API int ovrfsr_reset(ovrfsr_ctx *ctx)
{
    if (!ctx) return OVRFSR_ERR_INVALID_ARGUMENT;
    return guarded([&] { ctx->pp->Reset(); return (int)OVRFSR_OK; });
}

OVRFSR_API int ovrfsr_apply(ovrfsr_ctx *ctx, int eye, const ovrfsr_image *in, const ovrfsr_bounds *bounds,
                            ovrfsr_image *out, void *stream)
{
    if (!ctx) return OVRFSR_ERR_INVALID_ARGUMENT;
    return guarded([&] { return ctx->pp->Apply(eye, in, bounds, out, static_cast<hipStream_t>(stream)); });
}

OVRFSR_API int ovrfsr_apply_batch(ovrfsr_ctx *ctx, uint32_t n, int first_eye, int alternate_eyes, const ovrfsr_image *in0,
                                  size_t in_stride_bytes, const ovrfsr_image *out0, size_t out_stride_bytes, void *stream)
{
    if (!ctx) return OVRFSR_ERR_INVALID_ARGUMENT;
    return guarded([&] {
        return ctx->pp->ApplyBatch(n, first_eye, alternate_eyes, in0, in_stride_bytes, out0, out_stride_bytes, static_cast<hipStream_t>(stream));
    });
}

OVRFSR_API int ovrfsr_apply_batch_shared(ovrfsr_ctx *ctx, uint32_t n, const ovrfsr_image *in0, size_t in_stride_bytes,
                                         const ovrfsr_image *out0, size_t out_stride_bytes, void *stream)
{
    if (!ctx) return OVRFSR_ERR_INVALID_ARGUMENT;
    return guarded([&] {
        return ctx->pp->ApplyBatch(n, OVRFSR_EYE_LEFT, 0, in0, in_stride_bytes, out0, out_stride_bytes, static_cast<hipStream_t>(stream), true);
    });
}

OVRFSR_API const char *ovrfsr_last_error(const ovrfsr_ctx *ctx) { return ctx ? ctx->pp->LastError() : "null ctx"; }

OVRFSR_API int ovrfsr_last_gpu_time_ms(ovrfsr_ctx *ctx, float *ms)
{
    if (!ctx) return OVRFSR_ERR_INVALID_ARGUMENT;
    return guarded([&] { return ctx->pp->LastGpuTimeMs(ms); });
}

OVRFSR_API int ovrfsr_average_gpu_time_ms(ovrfsr_ctx *ctx, float *ms, uint32_t *reports)
{
    if (!ctx) return OVRFSR_ERR_INVALID_ARGUMENT;
    return guarded([&] { return ctx->pp->AverageGpuTimeMs(ms, reports); });
}

OVRFSR_API void ovrfsr_easu_con(uint32_t con[16], float vw, float vh, float iw, float ih, float ow, float oh)
{
    if (con) ovrfsr::easu_con(con, vw, vh, iw, ih, ow, oh); // (null outputs: nothing to do -- no entry point dereferences a null it was handed)
}

OVRFSR_API void ovrfsr_rcas_con(uint32_t con[4], float stops) { if (con) ovrfsr::rcas_con(con, stops); }

OVRFSR_API void ovrfsr_mask_constants(uint32_t centre[4], uint32_t radius[4], uint32_t out_w, uint32_t out_h,
                                      const float proj_centre[4], float cfg_radius, int only_one_eye, int eye)
{
    if (centre && radius && proj_centre) ovrfsr::mask_constants(centre, radius, out_w, out_h, proj_centre, cfg_radius, only_one_eye, eye);
}

OVRFSR_API int ovrfsr_nis_scaler_config(void *cfg256, float sharpness, uint32_t in_w, uint32_t in_h, uint32_t out_w, uint32_t out_h)
{
    return cfg256 ? ovrfsr::nis_scaler_config(cfg256, sharpness, in_w, in_h, out_w, out_h) : 0;
}

OVRFSR_API int ovrfsr_nis_sharpen_config(void *cfg256, float sharpness, uint32_t in_w, uint32_t in_h)
{
    return cfg256 ? ovrfsr::nis_scaler_config(cfg256, sharpness, in_w, in_h, in_w, in_h) : 0;
}

OVRFSR_API const float *ovrfsr_nis_coef_scale(void) { return ovrfsr::nis_coef_scale(); }
OVRFSR_API const float *ovrfsr_nis_coef_usm(void) { return ovrfsr::nis_coef_usm(); }

} // extern "C"
