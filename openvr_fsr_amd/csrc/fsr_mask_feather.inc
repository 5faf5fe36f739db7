// fsr_mask_feather.inc -- the pass of ovrfsr_set_mask_feather (header, "Mask feather"; the rule itself: mask_feather.h), included at the end
// of fsr_kernels.hip behind fsr_tap_tables.inc.  It runs behind the unchanged pipeline, on the caller's stream, over the band only: one
// workgroup per 32x32 output tile of the box that holds the disc(s) (feather_box), 256 threads, four pixels of one column each.  A band
// pixel -- its 16x16 group inside by the reference's rule, its weight w8 below 256 -- is read from the destination (s: what the pipeline
// stored), given the value it has when its group is OUTSIDE (o: the bilinear fallback in the reference's operator order, through the
// intermediate's and the destination's store conversions, RCAS's debug tint between them), and written back as o + (s - o) * w8 / 256 with
// the destination's store conversion; alpha keeps the stored value.  Every thread touches its own pixels only: no hazard, no LDS.
// One rule for every build and precision (contraction off, like the HDR passes), and ONE kernel: the three formats are arguments behind
// workgroup-uniform switches, not template parameters -- the pass touches a few per cent of the pixels.  The conversions are the strict
// build's (load_unit's decode rules and ovrfsr_strict::store_unit, whose half store keeps "round to fp32, then to half"); the taps are the tables every
// launch already carries, which a re-scale refills on the device.
#include "mask_feather.h"

namespace ovrfsr_fast {
#pragma clang fp contract(off)

// The texel at byte offset `off` of an image whose texels are `tb` bytes (workgroup-uniform), raw: the words wait in registers until every
// load of the thread has been issued ...
template <typename IMG>
__device__ __forceinline__ uint4 feather_raw(uint32_t tb, IMG img, uint32_t off)
{
    uint4 r = make_uint4(0u, 0u, 0u, 0u);
    const auto p = img + off;
    if (tb == 4u) {
        r.x = *OVRFSR_AT(const uint32_t, p);
    } else if (tb == 8u) {
        const uint2 v = *OVRFSR_AT(const uint2, p);
        r.x = v.x; r.y = v.y;
    } else {
        r = *OVRFSR_AT(const uint4, p);
    }
    return r;
}

// ... and their unit-domain RGBA by the rules of load_unit (fsr_device.inc), format by format
__device__ __forceinline__ float4 feather_decode(int fmt, const uint4 &w)
{
    switch (fmt) {
    case ovrfsr::FMT_RGBA8:
        return make_float4(ovrfsr_strict::unorm8_to_unit((float)(w.x & 0xffu)), ovrfsr_strict::unorm8_to_unit((float)((w.x >> 8) & 0xffu)),
                           ovrfsr_strict::unorm8_to_unit((float)((w.x >> 16) & 0xffu)), ovrfsr_strict::unorm8_to_unit((float)(w.x >> 24)));
    case ovrfsr::FMT_RGBA16F:
        return make_float4((float)__builtin_bit_cast(_Float16, (uint16_t)(w.x & 0xffffu)), (float)__builtin_bit_cast(_Float16, (uint16_t)(w.x >> 16)),
                           (float)__builtin_bit_cast(_Float16, (uint16_t)(w.y & 0xffffu)), (float)__builtin_bit_cast(_Float16, (uint16_t)(w.y >> 16)));
    case ovrfsr::FMT_RGB10A2:
        return make_float4((float)(w.x & 1023u) / 1023.0f, (float)((w.x >> 10) & 1023u) / 1023.0f, (float)((w.x >> 20) & 1023u) / 1023.0f, (float)(w.x >> 30) / 3.0f);
    case ovrfsr::FMT_R11G11B10F: {
        float4 c;
        ovrfsr_strict::unpack_r11g11b10f(w.x, c.x, c.y, c.z);
        c.w = 1.0f;
        return c;
    }
    default:
        return make_float4(__uint_as_float(w.x), __uint_as_float(w.y), __uint_as_float(w.z), __uint_as_float(w.w));
    }
}

// x stored to a texture of format `fmt` and loaded again (fmt < 0: no texture in between).  A half is rounded from the fp32 value in integer
// arithmetic (hdr_half_bits: equal to the hardware conversion, and nothing the backend can fold a preceding operation into)
__device__ __forceinline__ float feather_through(int fmt, float x)
{
    switch (fmt) {
    case ovrfsr::FMT_RGBA8: return ovrfsr_strict::unorm8_to_unit((float)ovrfsr_strict::unit_to_unorm8(x));
    case ovrfsr::FMT_RGBA16F: return (float)__builtin_bit_cast(_Float16, (uint16_t)ovrfsr::hdr_half_bits(x));
    case ovrfsr::FMT_RGB10A2: return (float)ovrfsr_strict::unit_to_unorm10(x) / 1023.0f;
    default: return x;
    }
}

__device__ __forceinline__ uint32_t feather_texel_bytes(int fmt)
{
    return fmt == ovrfsr::FMT_RGBA16F ? 8u : fmt == ovrfsr::FMT_RGBA32F ? 16u : 4u;
}

// (a template, like tap_tables_kernel: a plain kernel would take bgra_to_rgba_kernel's place at the end of the code object)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void mask_feather_kernel(const ovrfsr::FeatherArgs a)
{
    static_assert(THREADS == 256, "a 32x32 tile, four rows per thread");
    const uint32_t img_i = blockIdx.z;
    const uint32_t eye = (a.m.first_eye ^ (img_i & a.m.alternate)) & 1u;
    if ((eye ? a.m.mode[1] : a.m.mode[0]) != ovrfsr::MASK_MIXED) return;
    ovrfsr::FeatherCon fc;
    if (!ovrfsr::feather_constants(a.R, a.F, &fc)) return;
    // (selected, not indexed: the argument block stays in scalar registers)
    const uint32_t centre[4] = {eye ? a.m.centre[1][0] : a.m.centre[0][0], eye ? a.m.centre[1][1] : a.m.centre[0][1],
                                eye ? a.m.centre[1][2] : a.m.centre[0][2], eye ? a.m.centre[1][3] : a.m.centre[0][3]};
    const uint32_t *hidden = eye ? a.hiddenBits[1] : a.hiddenBits[0];
    const uint32_t tileX = a.tile0X + blockIdx.x, tileY = a.tile0Y + blockIdx.y;
    const uint32_t outW = (uint32_t)a.v.outW, outH = (uint32_t)a.v.outH;
    const uint32_t x0 = tileX * 32u, y0 = tileY * 32u;
    if (x0 >= outW || y0 >= outH) return;
    // ---- the workgroup-uniform part: integers only.  A tile the plan skips (hidden-area mesh) is neither read nor written ...
    if (hidden) {
        const uint32_t t = tileY * a.tilesX + tileX;
        OVRFSR_PTR(const uint32_t) bits = OVRFSR_PLANE(const uint32_t, hidden, (a.tilesX * a.tilesY + 31u) / 32u, 0, K_TILE_LIST);
        if ((*OVRFSR_AT(const uint32_t, bits + (t >> 5)) >> (t & 31u)) & 1u) return;
    }
    // ... a tile with no group inside has no band pixel, nor has one whose four corners are all within Ri of one centre (w8 = 256 throughout)
    const uint32_t x1 = x0 + 31u < outW - 1u ? x0 + 31u : outW - 1u, y1 = y0 + 31u < outH - 1u ? y0 + 31u : outH - 1u;
    uint32_t inside = 0;
#pragma unroll
    for (uint32_t g = 0; g < 4; ++g) {
        const uint32_t gx = x0 + 16u * (g & 1u), gy = y0 + 16u * (g >> 1);
        if (gx < outW && gy < outH && ovrfsr::feather_group_inside(centre, a.m.r2, gx, gy)) inside |= 1u << g;
    }
    if (!inside) return;
#pragma unroll
    for (uint32_t k = 0; k < 2; ++k) {
        const uint64_t cx = centre[2 * k], cy = centre[2 * k + 1];
        const uint64_t dxa = cx - x0, dxb = cx - x1, dya = cy - y0, dyb = cy - y1;
        const uint64_t xa2 = dxa * dxa, xb2 = dxb * dxb, ya2 = dya * dya, yb2 = dyb * dyb; // (squares of small signed differences: no wrap on any image)
        if ((cx | cy) < 32768u && (xa2 > xb2 ? xa2 : xb2) + (ya2 > yb2 ? ya2 : yb2) <= fc.ri2) return;
    }
    // ---- the pixels: (ox, oyb + 8k)
    const uint32_t ox = x0 + (threadIdx.x & 31u), oyb = y0 + (threadIdx.x >> 5);
    if (ox >= outW) return;
    if (!((inside >> ((threadIdx.x >> 4) & 1u)) & 5u)) return; // neither group of this column is inside
    const uint32_t itb = feather_texel_bytes(a.inFmt), otb = feather_texel_bytes(a.outFmt);
    OVRFSR_PTR(const uint8_t) in = OVRFSR_IMAGE(const uint8_t, a.v.in + (size_t)img_i * a.v.in_stride, a.v.in_pitch, a.v.inW, a.v.inH, itb, K_IMAGE_IN);
    OVRFSR_PTR(uint8_t) out = OVRFSR_IMAGE(uint8_t, a.v.out + (size_t)img_i * a.v.out_stride, a.v.out_pitch, a.v.outW, a.v.outH, otb, K_IMAGE_OUT);
    OVRFSR_PTR(const ovrfsr::BilinTap) bilX = OVRFSR_PLANE(const ovrfsr::BilinTap, a.bilX, outW, (32u - (outW & 31u)) & 31u, K_BIL_X);
    OVRFSR_PTR(const ovrfsr::BilinTap) bilY = OVRFSR_PLANE(const ovrfsr::BilinTap, a.bilY, outH, 0, K_BIL_Y);
    const uint2 txw = *OVRFSR_AT(const uint2, bilX + ox);
    const int txi = (int)txw.x;
    const float fx = __uint_as_float(txw.y);
    const uint32_t xoa = (uint32_t)ovrfsr_strict::clampi(txi, 0, a.v.inW - 1) * itb, xob = (uint32_t)ovrfsr_strict::clampi(txi + 1, 0, a.v.inW - 1) * itb;
    const float dbg = (float)a.debug;
    const float mulG = 1.0f - dbg * 0.3f; // fsr_rcas.hlsl:46: mul = 1 - debug * (0, .3, .3, 0)
    // Three memory round trips per thread, not three per pixel: the row taps of the four pixels, then every texel and the four stored
    // values (raw words), then the arithmetic and the stores.  No store of this thread precedes any of its loads.
    uint32_t w8[4];
    uint2 tyw[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t oy = oyb + 8u * k;
        w8[k] = 256u; // not a band pixel: behind the image, its group outside (never touched), or inside the ramp's inner edge
        tyw[k] = make_uint2(0u, 0u);
        if (oy < outH && ((inside >> (((threadIdx.x >> 4) & 1u) + 2u * (k >> 1))) & 1u)) {
            const uint64_t d2 = ovrfsr::feather_d2(centre, ox, oy);
            if (!ovrfsr::feather_full(fc, d2)) {
                w8[k] = ovrfsr::feather_w8(fc, d2);
                tyw[k] = *OVRFSR_AT(const uint2, bilY + oy);
            }
        }
    }
    uint4 t00[4], t10[4], t01[4], t11[4], sw[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        if (w8[k] < 256u) {
            const int tyi = (int)tyw[k].x;
            const uint32_t ra = (uint32_t)ovrfsr_strict::clampi(tyi, 0, a.v.inH - 1) * a.v.in_pitch, rb = (uint32_t)ovrfsr_strict::clampi(tyi + 1, 0, a.v.inH - 1) * a.v.in_pitch;
            t00[k] = feather_raw(itb, in, ra + xoa); t10[k] = feather_raw(itb, in, ra + xob);
            t01[k] = feather_raw(itb, in, rb + xoa); t11[k] = feather_raw(itb, in, rb + xob);
            sw[k] = feather_raw(otb, out, (oyb + 8u * k) * a.v.out_pitch + ox * otb);
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        if (w8[k] < 256u) {
            const uint32_t oy = oyb + 8u * k;
            // o, step 1: the bilinear fallback sample (D3D rule, unfused)
            const float fy = __uint_as_float(tyw[k].y);
            const float4 c00 = feather_decode(a.inFmt, t00[k]), c10 = feather_decode(a.inFmt, t10[k]);
            const float4 c01 = feather_decode(a.inFmt, t01[k]), c11 = feather_decode(a.inFmt, t11[k]);
            const float w00 = (1.0f - fx) * (1.0f - fy), w10 = fx * (1.0f - fy), w01 = (1.0f - fx) * fy, w11 = fx * fy;
            float r = ovrfsr_strict::bilerp<true>(c00.x, c10.x, c01.x, c11.x, w00, w10, w01, w11);
            float g = ovrfsr_strict::bilerp<true>(c00.y, c10.y, c01.y, c11.y, w00, w10, w01, w11);
            float b = ovrfsr_strict::bilerp<true>(c00.z, c10.z, c01.z, c11.z, w00, w10, w01, w11);
            // step 2: where a sharpen stage follows, through the intermediate, then the RCAS outside branch's tint
            if (a.midFmt >= 0) {
                r = feather_through(a.midFmt, r);
                g = feather_through(a.midFmt, g) * mulG;
                b = feather_through(a.midFmt, b) * mulG;
            }
            // step 3: through the destination
            r = feather_through(a.outFmt, r); g = feather_through(a.outFmt, g); b = feather_through(a.outFmt, b);
            // s, the blend, and the store
            const float4 s = feather_decode(a.outFmt, sw[k]);
            const float vr = ovrfsr::feather_blend(s.x, r, w8[k]), vg = ovrfsr::feather_blend(s.y, g, w8[k]), vb = ovrfsr::feather_blend(s.z, b, w8[k]);
            switch (a.outFmt) {
            case ovrfsr::FMT_RGBA8: ovrfsr_strict::store_unit<ovrfsr::FMT_RGBA8>(out, a.v.out_pitch, (int)ox, (int)oy, vr, vg, vb, s.w); break;
            case ovrfsr::FMT_RGBA16F: ovrfsr_strict::store_unit<ovrfsr::FMT_RGBA16F>(out, a.v.out_pitch, (int)ox, (int)oy, vr, vg, vb, s.w); break;
            case ovrfsr::FMT_RGB10A2: ovrfsr_strict::store_unit<ovrfsr::FMT_RGB10A2>(out, a.v.out_pitch, (int)ox, (int)oy, vr, vg, vb, s.w); break;
            default: ovrfsr_strict::store_unit<ovrfsr::FMT_RGBA32F>(out, a.v.out_pitch, (int)ox, (int)oy, vr, vg, vb, s.w); break;
            }
        }
    }
}

} // namespace ovrfsr_fast
#pragma clang fp contract(on)

namespace ovrfsr {

// One launch: the tiles [a.tile0X, + tilesW) x [a.tile0Y, + tilesH) of `batch` images.  The caller has decided that an eye of the pass is
// active; the kernel decides per image and per tile.
hipError_t launch_mask_feather(const FeatherArgs &a, uint32_t tilesW, uint32_t tilesH, uint32_t batch, hipStream_t s)
{
    launch_fresh();
    if (!a.v.in || !a.v.out || !a.bilX || !a.bilY || tilesW == 0 || tilesH == 0 || batch == 0) return hipErrorInvalidValue;
    if (a.tile0X + tilesW > a.tilesX || a.tile0Y + tilesH > a.tilesY) return hipErrorInvalidValue; // (the bitmap and the images end there)
    const int i = a.inFmt, m = a.midFmt, o = a.outFmt;
    if ((i != FMT_RGBA8 && i != FMT_RGBA16F && i != FMT_RGBA32F && i != FMT_RGB10A2 && i != FMT_R11G11B10F) ||
        (m >= 0 && m != FMT_RGBA8 && m != FMT_RGBA16F && m != FMT_RGBA32F && m != FMT_RGB10A2) ||
        (o != FMT_RGBA8 && o != FMT_RGBA16F && o != FMT_RGBA32F && o != FMT_RGB10A2))
        return hipErrorInvalidValue; // not a format the pass converts: an error, never a pass that does something else
    return launch_kernel<ovrfsr_fast::mask_feather_kernel<256>>(dim3(tilesW, tilesH, batch), dim3(256), 0, s, a);
}

} // namespace ovrfsr
