// mask_feather.h -- the rule of ovrfsr_set_mask_feather (header, "Mask feather"): the ramp's constants, the weight of a pixel and the blend.
// ONE definition for the host (ovrfsr_mask_feather_weights in capi.cpp, the launch manager's grid) and the device (fsr_mask_feather.inc),
// like hdr_map.h and bilin_taps.h.  Integers decide everything but the blend itself: whether an eye is feathered, which pixels belong to the
// band, and the weight w8 in 1/256ths; the blend is two fp32 operations and a product, each rounded once (no a * b + c may contract here).
//   F   = f2u(0.5f * width * outH)       the expression of radius[0] (constants.cpp), the same float -> uint rule
//   Ro  = R > 12 ? R - 12 : 0            outer edge of the ramp, R = radius[0]; 12 = the guard (below)
//   Ri  = Ro > F ? Ro - F : 0            inner edge
//   den = Ro * Ro - Ri * Ri              64-bit
//   d2  = min over the two centres k of (cx_k - x)^2 + (cy_k - y)^2        signed 64-bit, the centre words zero-extended
//   w8  = clamp(floor(256 * (Ro * Ro - d2) / den), 0, 256)
// The guard: a pixel is at most sqrt(8^2 + 8^2) = 11.32 from the centre of its 16x16 group, so a pixel with w8 > 0 (d < Ro = R - 12) has
// its group's centre closer than R to the mask centre -- the group is inside by the reference's rule (group_inside).  w8 is therefore 0
// all along the staircase of groups, on its inside.
// (64-bit arithmetic wraps modulo 2^64 for mask constants that no image reaches -- words of 2^27 and above; it is written on unsigned
// operands so that nothing here is undefined for any input.)
#pragma once
#include <stdint.h>
#include "tile_records.h" // OVRFSR_HD

namespace ovrfsr {

constexpr uint32_t kFeatherGuard = 12;

struct FeatherCon {
    uint32_t ro, ri;   // outer and inner edge of the ramp, pixels
    uint64_t ro2, ri2; // their squares
    uint64_t den;      // ro2 - ri2
};

// the float -> uint32 rule of the mask constants (constants.cpp, f2u_sat): truncation where that is defined, 0 for NaN and negatives,
// 0xffffffff from 2^32 upwards
OVRFSR_HD inline uint32_t feather_f2u(float x)
{
    if (!(x > 0.0f)) return 0u;
    if (x >= 4294967296.0f) return 0xffffffffu;
    return (uint32_t)x;
}

// F of a width in cfg.radius's unit (outH / 2)
OVRFSR_HD inline uint32_t feather_px(float width, uint32_t outH)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float half = 0.5f * width;
    return feather_f2u(half * (float)outH);
}

// the ramp of (R, F); false: no ramp (F = 0 or Ro = 0) -- the feather is not active, *c is zeroed
OVRFSR_HD inline bool feather_constants(uint32_t R, uint32_t F, FeatherCon *c)
{
    c->ro = R > kFeatherGuard ? R - kFeatherGuard : 0u;
    c->ri = c->ro > F ? c->ro - F : 0u;
    c->ro2 = (uint64_t)c->ro * c->ro;
    c->ri2 = (uint64_t)c->ri * c->ri;
    c->den = c->ro2 - c->ri2;
    return F >= 1u && c->ro >= 1u;
}

// d2 of pixel (x, y): the nearer of the two centres
OVRFSR_HD inline uint64_t feather_d2(const uint32_t centre[4], uint32_t x, uint32_t y)
{
    const uint64_t ax = (uint64_t)centre[0] - x, ay = (uint64_t)centre[1] - y, bx = (uint64_t)centre[2] - x, by = (uint64_t)centre[3] - y;
    const uint64_t a = ax * ax + ay * ay, b = bx * bx + by * by; // (the squares of the signed differences, modulo 2^64)
    return (int64_t)a < (int64_t)b ? a : b;
}

// w8 from d2; c from feather_constants() == true (den >= 1)
OVRFSR_HD inline uint32_t feather_w8(const FeatherCon &c, uint64_t d2)
{
    const int64_t num = (int64_t)(c.ro2 - d2);
    if (num <= 0) return 0u;
    if ((uint64_t)num >= c.den) return 256u;
    return (uint32_t)((256u * (uint64_t)num) / c.den);
}

// w8 == 256 without the division: the pixel keeps its stored value
OVRFSR_HD inline bool feather_full(const FeatherCon &c, uint64_t d2) { return (int64_t)d2 <= (int64_t)c.ri2; }

// the reference's group rule (fsr_easu.hlsl:41-45) for the 16x16 group of pixel (x, y), uint32 wrap-around and all
OVRFSR_HD inline bool feather_group_inside(const uint32_t centre[4], uint32_t r2, uint32_t x, uint32_t y)
{
    const uint32_t cx = (x & ~15u) + 8u, cy = (y & ~15u) + 8u;
    const uint32_t d1x = centre[0] - cx, d1y = centre[1] - cy, d2x = centre[2] - cx, d2y = centre[3] - cy;
    return (d1x * d1x + d1y * d1y <= r2) || (d2x * d2x + d2y * d2y <= r2);
}

// v = o + (s - o) * t, t = w8 / 256 (exact), every operator rounded once
OVRFSR_HD inline float feather_blend(float s, float o, uint32_t w8)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float t = (float)w8 / 256.0f;
    const float d = s - o;
    const float p = d * t;
    return o + p;
}

// The pixels of an image that can be band pixels, as a box [x0, x1) x [y0, y1): every pixel of an inside group is closer than R + 12 to a
// mask centre (its group's centre is within R, the pixel within 11.32 of that), so the box of the two discs of radius R + 12, cut to the
// image, holds them all.  Mask constants large enough for the group rule's 32-bit products to wrap (words of 32768 and above -- three
// times the largest image) give the whole image.  false: the box is empty.
inline bool feather_box(const uint32_t centre[4], uint32_t R, uint32_t outW, uint32_t outH, uint32_t box[4])
{
    box[0] = 0; box[1] = 0; box[2] = outW; box[3] = outH;
    uint32_t big = R;
    for (int i = 0; i < 4; ++i) big = centre[i] > big ? centre[i] : big;
    if (big >= 32768u) return outW != 0 && outH != 0;
    const uint32_t reach = R + kFeatherGuard;
    const uint32_t xlo = centre[0] < centre[2] ? centre[0] : centre[2], xhi = centre[0] < centre[2] ? centre[2] : centre[0];
    const uint32_t ylo = centre[1] < centre[3] ? centre[1] : centre[3], yhi = centre[1] < centre[3] ? centre[3] : centre[1];
    box[0] = xlo > reach ? xlo - reach : 0u;
    box[1] = ylo > reach ? ylo - reach : 0u;
    box[2] = xhi + reach + 1u < outW ? xhi + reach + 1u : outW;
    box[3] = yhi + reach + 1u < outH ? yhi + reach + 1u : outH;
    return box[0] < box[2] && box[1] < box[3];
}

} // namespace ovrfsr
