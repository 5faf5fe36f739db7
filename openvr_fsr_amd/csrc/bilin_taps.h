// bilin_taps.h -- one tap of the bilinear fallback / NIS DirectCopy tables (Plan::taps): SampleLevel at o / outN, texel space u * inN - 0.5, D3D11's
// 8-bit sub-texel snap -- the same IEEE operations as fsr_device.inc's bilinear_uv / fixed8, evaluated once per column and row.  One
// definition with two callers, like tile_records.h: the planner's tap_tables (pipeline_plan.cpp, host) and tap_tables_kernel
// (fsr_tap_tables.inc, device), which refills the tables of a rescale-capable ctx when the input size moves.  Both sides round identically:
// a correctly rounded division, every product and sum rounded on its own (no contraction), floor.
#pragma once
#include <math.h>
#include <stdint.h>
#include "fsr_params.h"

namespace ovrfsr {

namespace taps_detail {
// one IEEE operation each, round to nearest even.  Host: through a volatile, so that no compiler setting contracts or re-associates them;
// device: the plain operators under contract(off) -- the division compiles to the correctly rounded v_div_scale / v_div_fmas / v_div_fixup
// sequence (this unit is built without fast-math and without -fno-hip-fp32-correctly-rounded-divide-sqrt)
#if defined(__HIP_DEVICE_COMPILE__)
__device__ inline float div_rn(float a, float b)
{
#pragma clang fp contract(off)
    return a / b;
}
__device__ inline float mul_rn(float a, float b)
{
#pragma clang fp contract(off)
    return a * b;
}
__device__ inline float add_rn(float a, float b)
{
#pragma clang fp contract(off)
    return a + b;
}
#else
inline float div_rn(float a, float b) { volatile float r = a / b; return r; }
inline float mul_rn(float a, float b) { volatile float r = a * b; return r; }
inline float add_rn(float a, float b) { volatile float r = a + b; return r; }
#endif
} // namespace taps_detail

// tap `o` of an axis of outN output pixels over inN input texels: the left / upper texel (-1 .. inN - 1) and the weight of the next one
OVRFSR_HD inline BilinTap bilin_tap(uint32_t o, uint32_t outN, uint32_t inN)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    using namespace taps_detail;
    const float u = div_rn((float)o, (float)outN);
    const float tt = add_rn(mul_rn(u, (float)inN), -0.5f);
    const float s = floorf(add_rn(mul_rn(tt, 256.0f), 0.5f));
    const float f = floorf(mul_rn(s, 1.0f / 256.0f));
    BilinTap t;
    t.i0 = (int32_t)f;
    t.frac = mul_rn(add_rn(mul_rn(f, -256.0f), s), 1.0f / 256.0f); // exact: s, f * 256 are integers < 2^24
    return t;
}

// entry i of the table [outW column taps, padded to tapYOff with copies of the last | outH row taps at tapYOff]; i < tapYOff + outH
OVRFSR_HD inline BilinTap tap_table_entry(uint32_t i, uint32_t outW, uint32_t outH, uint32_t inW, uint32_t inH, uint32_t tapYOff)
{
    const bool row = i >= tapYOff;
    const uint32_t o = row ? i - tapYOff : (i < outW ? i : outW - 1u);
    return bilin_tap(o, row ? outH : outW, row ? inH : inW);
}

} // namespace ovrfsr
