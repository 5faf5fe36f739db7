// fsr_hdr_domain.inc -- the two passes of OVRFSR_HDR_DOMAIN_SRTM (header, "HDR domain"; the mapping itself: hdr_map.h), included at the end of
// fsr_kernels.hip: they join the resolve kernels' code object, which every process loads anyway.
//   forward  the pipeline's float input (RGBA16F or RGBA32F: the submission, or the single-sample copy the resolve pass wrote) -> a ctx-owned
//            RGBA32F copy holding the mapped values, rows tight (16 * w bytes), image i of the batch behind image i - 1
//   back     the pipeline's RGBA32F result, laid out the same way -> the destination the call names, un-mapped, with that format's store
//            conversion: RGBA32F as is, RGBA16F rounded to nearest even, RGBA8 saturate, x 255, + 0.5, truncate (unit_to_unorm8)
// One rule for every build and precision (the mapping is exact already), so one instantiation per format, like resolve_kernel.  Memory-bound
// copies: every thread moves 16 bytes of the NARROWER side -- 16 / texel bytes texels -- in one 16-byte access where that side is 16-byte
// aligned (`vec`), texel by texel otherwise and in the last group of a row; the RGBA32F side is always 16-byte texels.  Alpha passes through.
#include "hdr_map.h"

namespace ovrfsr_fast {
#pragma clang fp contract(off)

template <int F>
__global__ __launch_bounds__(256) void hdr_forward_kernel(const uint8_t *__restrict__ src, uint32_t srcPitch, uint64_t srcStride,
                                                          uint8_t *__restrict__ dst, uint32_t w, uint32_t h, uint32_t vec)
{
    static_assert(F == ovrfsr::FMT_RGBA16F || F == ovrfsr::FMT_RGBA32F, "float pipeline inputs");
    constexpr uint32_t T = F == ovrfsr::FMT_RGBA16F ? 2u : 1u; // texels per thread
    constexpr uint32_t TB = 16u / T;                           // source texel bytes
    const uint32_t x0 = (blockIdx.x * 256u + threadIdx.x) * T, y = blockIdx.y, img = blockIdx.z;
    if (x0 >= w) return;
    OVRFSR_PTR(const uint8_t) s = OVRFSR_IMAGE(const uint8_t, src + (size_t)img * srcStride, srcPitch, (int)w, (int)h, TB, K_IMAGE_IN);
    OVRFSR_PTR(uint8_t) d = OVRFSR_IMAGE(uint8_t, dst, w * 16u, (int)w, (int)(h * gridDim.z), 16u, K_IMAGE_OUT);
    OVRFSR_PTR(const uint8_t) row = s + ((size_t)y * srcPitch + (size_t)x0 * TB);
    OVRFSR_PTR(uint8_t) out = d + (((size_t)img * h + y) * w + x0) * 16u;
    if constexpr (F == ovrfsr::FMT_RGBA32F) {
        float4 c = *OVRFSR_AT(const float4, row);
        ovrfsr::hdr_map(c.x, c.y, c.z, false);
        *OVRFSR_AT(float4, out) = c;
    } else {
        const uint32_t n = min(2u, w - x0);
        uint32_t v[4] = {0u, 0u, 0u, 0u}; // texel t: dwords 2t (R | G << 16), 2t + 1 (B | A << 16)
        if (vec && n == 2u) {
            const uint4 q = *OVRFSR_AT(const uint4, row);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            const uint2 a = *OVRFSR_AT(const uint2, row);
            v[0] = a.x; v[1] = a.y;
            if (n == 2u) {
                const uint2 b = *OVRFSR_AT(const uint2, row + 8u);
                v[2] = b.x; v[3] = b.y;
            }
        }
#pragma unroll
        for (uint32_t t = 0; t < 2u; ++t) {
            if (t < n) {
                float4 c;
                c.x = (float)__builtin_bit_cast(_Float16, (uint16_t)(v[2 * t] & 0xffffu));
                c.y = (float)__builtin_bit_cast(_Float16, (uint16_t)(v[2 * t] >> 16));
                c.z = (float)__builtin_bit_cast(_Float16, (uint16_t)(v[2 * t + 1] & 0xffffu));
                c.w = (float)__builtin_bit_cast(_Float16, (uint16_t)(v[2 * t + 1] >> 16));
                ovrfsr::hdr_map(c.x, c.y, c.z, false);
                *OVRFSR_AT(float4, out + 16u * t) = c;
            }
        }
    }
}

template <int O>
__global__ __launch_bounds__(256) void hdr_back_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint32_t dstPitch, uint64_t dstStride,
                                                       uint32_t w, uint32_t h, uint32_t vec)
{
    static_assert(O == ovrfsr::FMT_RGBA8 || O == ovrfsr::FMT_RGBA16F || O == ovrfsr::FMT_RGBA32F, "the destinations of a float pipeline");
    constexpr uint32_t T = O == ovrfsr::FMT_RGBA32F ? 1u : O == ovrfsr::FMT_RGBA16F ? 2u : 4u; // texels per thread
    constexpr uint32_t TB = 16u / T;                                                           // destination texel bytes
    constexpr uint32_t TW = TB / 4u;                                                           // ... and dwords
    const uint32_t x0 = (blockIdx.x * 256u + threadIdx.x) * T, y = blockIdx.y, img = blockIdx.z;
    if (x0 >= w) return;
    OVRFSR_PTR(const uint8_t) s = OVRFSR_IMAGE(const uint8_t, src, w * 16u, (int)w, (int)(h * gridDim.z), 16u, K_IMAGE_IN);
    OVRFSR_PTR(uint8_t) d = OVRFSR_IMAGE(uint8_t, dst + (size_t)img * dstStride, dstPitch, (int)w, (int)h, TB, K_IMAGE_OUT);
    OVRFSR_PTR(const uint8_t) in = s + (((size_t)img * h + y) * w + x0) * 16u;
    OVRFSR_PTR(uint8_t) row = d + ((size_t)y * dstPitch + (size_t)x0 * TB);
    const uint32_t n = min(T, w - x0);
    uint32_t o[4] = {0u, 0u, 0u, 0u}; // texel t: dwords [t * TW, + TW)
#pragma unroll
    for (uint32_t t = 0; t < T; ++t) {
        if (t < n) {
            float4 c = *OVRFSR_AT(const float4, in + 16u * t);
            ovrfsr::hdr_map(c.x, c.y, c.z, true);
            if constexpr (O == ovrfsr::FMT_RGBA32F) {
                o[0] = __float_as_uint(c.x); o[1] = __float_as_uint(c.y); o[2] = __float_as_uint(c.z); o[3] = __float_as_uint(c.w);
            } else if constexpr (O == ovrfsr::FMT_RGBA16F) {
                // (the products are fp32 values first, as a D3D fp32 shader in front of an RGBA16F store has them: hdr_half_bits, hdr_map.h)
                o[2 * t] = ovrfsr::hdr_half_bits(c.x) | (ovrfsr::hdr_half_bits(c.y) << 16);
                o[2 * t + 1] = ovrfsr::hdr_half_bits(c.z) | (ovrfsr::hdr_half_bits(c.w) << 16);
            } else {
                o[t] = unit_to_unorm8(c.x) | (unit_to_unorm8(c.y) << 8) | (unit_to_unorm8(c.z) << 16) | (unit_to_unorm8(c.w) << 24);
            }
        }
    }
    if (T == 1u || (vec && n == T)) {
        *OVRFSR_AT(uint4, row) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (uint32_t t = 0; t < T; ++t) {
            if (t < n) {
                if constexpr (TW == 1u) *OVRFSR_AT(uint32_t, row + 4u * t) = o[t];
                else *OVRFSR_AT(uint2, row + 8u * t) = make_uint2(o[2 * t], o[2 * t + 1]);
            }
        }
    }
}
} // namespace ovrfsr_fast
#pragma clang fp contract(on)

namespace ovrfsr {

// image i of the batch at src + i * srcStride; dst: batch images of w x h RGBA32F texels, tight
hipError_t launch_hdr_forward(int fmt, const uint8_t *src, uint32_t srcPitch, uint64_t srcStride, uint8_t *dst, uint32_t w, uint32_t h,
                              uint32_t batch, hipStream_t s)
{
    launch_fresh();
    const uint32_t vec = rows_vectorizable(src, srcPitch, srcStride, batch, 16u);
    if (fmt == FMT_RGBA16F)
        return launch_kernel<ovrfsr_fast::hdr_forward_kernel<FMT_RGBA16F>>(dim3((w + 511u) / 512u, h, batch), dim3(256), 0, s, src, srcPitch, srcStride, dst, w, h, vec);
    if (fmt == FMT_RGBA32F)
        return launch_kernel<ovrfsr_fast::hdr_forward_kernel<FMT_RGBA32F>>(dim3((w + 255u) / 256u, h, batch), dim3(256), 0, s, src, srcPitch, srcStride, dst, w, h, vec);
    return hipErrorInvalidValue; // not a float pipeline input: no kernel is built for it
}

// src: batch images of w x h RGBA32F texels, tight; image i of the destination at dst + i * dstStride
hipError_t launch_hdr_back(int fmt, const uint8_t *src, uint8_t *dst, uint32_t dstPitch, uint64_t dstStride, uint32_t w, uint32_t h,
                           uint32_t batch, hipStream_t s)
{
    launch_fresh();
    const uint32_t vec = rows_vectorizable(dst, dstPitch, dstStride, batch, 16u);
    if (fmt == FMT_RGBA8)
        return launch_kernel<ovrfsr_fast::hdr_back_kernel<FMT_RGBA8>>(dim3((w + 1023u) / 1024u, h, batch), dim3(256), 0, s, src, dst, dstPitch, dstStride, w, h, vec);
    if (fmt == FMT_RGBA16F)
        return launch_kernel<ovrfsr_fast::hdr_back_kernel<FMT_RGBA16F>>(dim3((w + 511u) / 512u, h, batch), dim3(256), 0, s, src, dst, dstPitch, dstStride, w, h, vec);
    if (fmt == FMT_RGBA32F)
        return launch_kernel<ovrfsr_fast::hdr_back_kernel<FMT_RGBA32F>>(dim3((w + 255u) / 256u, h, batch), dim3(256), 0, s, src, dst, dstPitch, dstStride, w, h, vec);
    return hipErrorInvalidValue; // (RGB10A2 is no destination of a float pipeline: destination_refusal)
}

} // namespace ovrfsr
