// fsr_kernels.hip -- instantiates the gfx950 FSR1 kernels twice (product build and strict
// validation build, see fsr_kernels.inc) and exposes typed launchers to the host launch manager.
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdlib>
#include <type_traits>
#include "fsr_params.h"
#include "fsr_launch.h"
#include "fsr_formats.h"
#include "fsr_bounds.h"

#ifdef OVRFSR_TIE_AUDIT
// AUDIT BUILD (-DOVRFSR_TIE_AUDIT, never shipped): every pixel the product EASU resolves is resolved a second time in the reference's
// operator order, and what the product build stores is compared with what the strict build would store.  Counters, per device:
//   [0] pixels audited   [1] pixels the near-tie guard listed (re-resolved in reference order: equal by construction)
//   [2] FLIPS: pixels NOT listed whose stored UNORM8 bytes / guarded halves differ from the strict build's  -- the guard's claim is [2] == 0
//   [3] unlisted pixels whose half store differs in a channel BELOW xmin (outside the guard's contract: a flipped half-ulp there stays under 1e-3)
//   [4] max |product - strict| over all audited channels, fp32 bit pattern: bytes (UNORM8 stores) ...  [5] ... or half spacings (half stores)
__device__ unsigned long long g_ovrfsr_tie_audit[6];
// The exact-stores RCAS instances (rcas_exact_bytes): every stored pixel evaluated in reference order as well.
//   [0] pixels audited   [1] pixels the guard listed (stored from the reference-order evaluation)
//   [2] FLIPS: unlisted pixels whose product bytes differ from the reference-order bytes -- the mode's claim is [2] == 0
//   [3] max |product - reference-order| over all audited channels, in bytes, fp32 bit pattern: what the band is derived from
__device__ unsigned long long g_ovrfsr_tie_audit_rcas[4];
#endif

namespace ovrfsr_fast {
#define OVRFSR_STRICT 0
#pragma clang fp contract(fast)
#include "fsr_device.inc"
#include "fsr_kernels.inc"
#undef OVRFSR_STRICT
} // namespace ovrfsr_fast

namespace ovrfsr_strict {
#define OVRFSR_STRICT 1
#pragma clang fp contract(off)
#include "fsr_device.inc"
#include "fsr_kernels.inc"
#undef OVRFSR_STRICT
} // namespace ovrfsr_strict

// Resolve of a multisampled input (header, OVRFSR_FORMAT_MS): S samples per texel, interleaved, into a single-sample image of the base
// format (BGRA8 re-ordered to RGBA8 in the same pass).  One rule for every build and precision, so one instantiation per format and S:
// UNORM channels (sum + S/2) >> log2 S in integers; float channels summed in fp32 in sample order (contraction off), times 1/S (exact:
// S is a power of two), half rounded to nearest even.  Memory-bound: every thread writes 16 bytes (16 / texel bytes texels) and reads
// the S x 16 bytes behind them -- 16-byte loads where the source rows are 16-byte aligned (`vec`), texel loads otherwise and in the
// last group of a row.  The destination rows are padded to 16 bytes (launch_resolve), so the store is always one 16-byte store; the
// texels past the row's width that it writes land in that padding.
namespace ovrfsr_fast {
#pragma clang fp contract(off)
template <int F, int S>
__global__ __launch_bounds__(256) void resolve_kernel(const uint8_t *__restrict__ src, uint32_t srcPitch, uint64_t srcStride,
                                                      uint8_t *__restrict__ dst, uint32_t dstPitch, uint32_t w, uint32_t h, uint32_t vec)
{
    constexpr uint32_t TB = F == ovrfsr::FMT_RGBA16F ? 8u : F == ovrfsr::FMT_RGBA32F ? 16u : 4u; // texel bytes
    constexpr uint32_t T = 16u / TB;                                                             // texels per thread
    constexpr uint32_t TW = TB / 4u;                                                             // dwords per texel
    constexpr uint32_t L = S == 2 ? 1u : S == 4 ? 2u : 3u;
    static_assert(S == 2 || S == 4 || S == 8, "2, 4 or 8 samples");
    const uint32_t x0 = (blockIdx.x * 256u + threadIdx.x) * T, y = blockIdx.y, img = blockIdx.z;
    if (x0 >= w) return;
    OVRFSR_PTR(const uint8_t) s = OVRFSR_IMAGE(const uint8_t, src + (size_t)img * srcStride, srcPitch, (int)(w * S), (int)h, TB, K_IMAGE_IN);
    OVRFSR_PTR(uint8_t) d = OVRFSR_IMAGE(uint8_t, dst, dstPitch, (int)(dstPitch / TB), (int)(h * gridDim.z), TB, K_IMAGE_OUT);
    OVRFSR_PTR(const uint8_t) row = s + ((size_t)y * srcPitch + (size_t)x0 * S * TB);
    uint32_t v[4 * S]; // sample sm of texel t: dwords [(t * S + sm) * TW, + TW)
    if (vec && x0 + T <= w) {
#pragma unroll
        for (uint32_t k = 0; k < S; ++k) {
            const uint4 q = *OVRFSR_AT(const uint4, row + 16u * k);
            v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
        }
    } else {
        const uint32_t n = min(T, w - x0);
#pragma unroll
        for (uint32_t t = 0; t < T; ++t)
#pragma unroll
            for (uint32_t sm = 0; sm < S; ++sm) {
                uint32_t *p = v + (t * S + sm) * TW;
                if (t < n) {
                    OVRFSR_PTR(const uint8_t) q = row + (t * S + sm) * TB;
                    if constexpr (TB == 4) { p[0] = *OVRFSR_AT(const uint32_t, q); }
                    else if constexpr (TB == 8) { const uint2 u = *OVRFSR_AT(const uint2, q); p[0] = u.x; p[1] = u.y; }
                    else { const uint4 u = *OVRFSR_AT(const uint4, q); p[0] = u.x; p[1] = u.y; p[2] = u.z; p[3] = u.w; }
                } else {
#pragma unroll
                    for (uint32_t j = 0; j < TW; ++j) p[j] = 0u;
                }
            }
    }
    uint32_t o[4];
    if constexpr (F == ovrfsr::FMT_RGBA8 || F == ovrfsr::FMT_BGRA8) {
#pragma unroll
        for (uint32_t t = 0; t < 4; ++t) {
            uint32_t r = resolve_unorm8<S>(v + t * S);
            if constexpr (F == ovrfsr::FMT_BGRA8) r = (r & 0xff00ff00u) | ((r >> 16) & 0xffu) | ((r & 0xffu) << 16); // B,G,R,A -> R,G,B,A
            o[t] = r;
        }
    } else if constexpr (F == ovrfsr::FMT_RGB10A2) {
#pragma unroll
        for (uint32_t t = 0; t < 4; ++t) {
            uint32_t r = S / 2, g = S / 2, b = S / 2, a = S / 2;
#pragma unroll
            for (uint32_t sm = 0; sm < S; ++sm) {
                const uint32_t q = v[t * S + sm];
                r += q & 0x3ffu; g += (q >> 10) & 0x3ffu; b += (q >> 20) & 0x3ffu; a += q >> 30;
            }
            o[t] = (r >> L) | ((g >> L) << 10) | ((b >> L) << 20) | ((a >> L) << 30);
        }
    } else if constexpr (F == ovrfsr::FMT_RGBA16F) {
#pragma unroll
        for (uint32_t t = 0; t < 2; ++t)
#pragma unroll
            for (uint32_t c = 0; c < 4; ++c) {
                float acc = 0.0f;
#pragma unroll
                for (uint32_t sm = 0; sm < S; ++sm) {
                    const uint32_t dw = v[(t * S + sm) * 2 + (c >> 1)];
                    const float f = (float)__builtin_bit_cast(_Float16, (uint16_t)(c & 1 ? dw >> 16 : dw & 0xffffu));
                    acc = sm == 0 ? f : acc + f;
                }
                const uint32_t hb = __builtin_bit_cast(uint16_t, (_Float16)(acc * (1.0f / S)));
                if (c & 1) o[2 * t + (c >> 1)] |= hb << 16;
                else o[2 * t + (c >> 1)] = hb;
            }
    } else {
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) {
            float acc = __uint_as_float(v[c]);
#pragma unroll
            for (uint32_t sm = 1; sm < S; ++sm) acc = acc + __uint_as_float(v[sm * 4 + c]);
            o[c] = __float_as_uint(acc * (1.0f / S));
        }
    }
    *OVRFSR_AT(uint4, d + ((size_t)img * h + y) * dstPitch + (size_t)x0 * TB) = make_uint4(o[0], o[1], o[2], o[3]);
}

// R11G11B10F input (header, OVRFSR_FORMAT_R11G11B10F) unpacked to RGBA16F, S samples per texel (1 = single-sample) resolved on the way.
// One 32-bit word per sample: R bits 0-10, G 11-21, B 22-31; every channel IS a half float without its sign and low mantissa bits
// (5-bit exponent, bias 15): half bits = channel << 4 (R, G) or << 5 (B), exact for every code, denormals, Inf and NaN included; alpha
// reads 1.0.  S > 1: the float rule of resolve_kernel on the decoded samples (fp32 sum in sample order, contraction off, times 1/S, half
// rounded to nearest even).  The first resolve-type kernel whose source (4 bytes) and destination (8 bytes) texels differ in size: every
// thread takes two texels -- 8 x S bytes in 16-byte loads (one 8-byte load at S = 1) where the source rows allow it (`vec`), word loads
// otherwise and in the last group of an odd-width row -- and writes them as one 16-byte store into rows padded to 16 bytes.
template <int S>
__global__ __launch_bounds__(256) void packed_resolve_kernel(const uint8_t *__restrict__ src, uint32_t srcPitch, uint64_t srcStride,
                                                             uint8_t *__restrict__ dst, uint32_t dstPitch, uint32_t w, uint32_t h, uint32_t vec)
{
    static_assert(S == 1 || S == 2 || S == 4 || S == 8, "1, 2, 4 or 8 samples");
    const uint32_t x0 = (blockIdx.x * 256u + threadIdx.x) * 2u, y = blockIdx.y, img = blockIdx.z;
    if (x0 >= w) return;
    OVRFSR_PTR(const uint8_t) s = OVRFSR_IMAGE(const uint8_t, src + (size_t)img * srcStride, srcPitch, (int)(w * S), (int)h, 4u, K_IMAGE_IN);
    OVRFSR_PTR(uint8_t) d = OVRFSR_IMAGE(uint8_t, dst, dstPitch, (int)(dstPitch / 8u), (int)(h * gridDim.z), 8u, K_IMAGE_OUT);
    OVRFSR_PTR(const uint8_t) row = s + ((size_t)y * srcPitch + (size_t)x0 * S * 4u);
    uint32_t v[2 * S]; // sample sm of texel t: word t * S + sm
    if (vec && x0 + 2u <= w) {
        if constexpr (S == 1) {
            const uint2 q = *OVRFSR_AT(const uint2, row);
            v[0] = q.x; v[1] = q.y;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < S / 2; ++k) {
                const uint4 q = *OVRFSR_AT(const uint4, row + 16u * k);
                v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
            }
        }
    } else {
        const uint32_t n = min(2u, w - x0);
#pragma unroll
        for (uint32_t t = 0; t < 2; ++t)
#pragma unroll
            for (uint32_t sm = 0; sm < S; ++sm) v[t * S + sm] = t < n ? *OVRFSR_AT(const uint32_t, row + (t * S + sm) * 4u) : 0u;
    }
    uint32_t o[4];
#pragma unroll
    for (uint32_t t = 0; t < 2; ++t) {
        if constexpr (S == 1) {
            const uint32_t q = v[t];
            o[2 * t] = ((q & 0x7ffu) << 4) | ((q & 0x3ff800u) << 9);
            o[2 * t + 1] = ((q >> 22) << 5) | 0x3c000000u;
        } else {
            float r = 0.0f, g = 0.0f, b = 0.0f;
#pragma unroll
            for (uint32_t sm = 0; sm < S; ++sm) {
                const uint32_t q = v[t * S + sm];
                const float fr = (float)__builtin_bit_cast(_Float16, (uint16_t)((q & 0x7ffu) << 4));
                const float fg = (float)__builtin_bit_cast(_Float16, (uint16_t)(((q >> 11) & 0x7ffu) << 4));
                const float fb = (float)__builtin_bit_cast(_Float16, (uint16_t)((q >> 22) << 5));
                r = sm == 0 ? fr : r + fr;
                g = sm == 0 ? fg : g + fg;
                b = sm == 0 ? fb : b + fb;
            }
            const uint32_t hr = __builtin_bit_cast(uint16_t, (_Float16)(r * (1.0f / S))), hg = __builtin_bit_cast(uint16_t, (_Float16)(g * (1.0f / S)));
            const uint32_t hb = __builtin_bit_cast(uint16_t, (_Float16)(b * (1.0f / S)));
            o[2 * t] = hr | (hg << 16);
            o[2 * t + 1] = hb | 0x3c000000u; // alpha: S ones summed, times 1/S
        }
    }
    *OVRFSR_AT(uint4, d + ((size_t)img * h + y) * dstPitch + (size_t)x0 * 8u) = make_uint4(o[0], o[1], o[2], o[3]);
}
} // namespace ovrfsr_fast
#pragma clang fp contract(on)

// The launchers.  fsr_launch_impl.h holds what they share with the other kernel units; here, and in that header, a kernel is emitted
// where a launcher first names it: the order of the launch_* definitions below, of the two includes between them and of the branches
// inside every launcher IS the order of the kernels in the code object.  The byte comparison of the code objects against the parent
// commit's (profiles/launch_layer.txt) holds it; that is the only reason launch_easu and launch_rcas stand behind the includes.
#define OVRFSR_LAUNCH_FSR 1
#include "fsr_launch_impl.h"

namespace ovrfsr {

template <int I, int O>
static hipError_t easu_go(bool strict, const EasuArgs &a, dim3 grid, size_t lds, hipStream_t s)
{
    const int pitch = easu_kernel_pitch(a.cellsW);
    if (strict) return launch_kernel<ovrfsr_strict::easu_kernel<I, O>>(grid, dim3(kThreads), lds, s, a);
    // footprints wider than the fixed pitches, and the 10-bit format (a quantised destination without a near-tie guard of
    // its own): the generic kernel, whose resolve is the reference-order one in every build
    if (pitch == 0 || I == FMT_RGB10A2 || O == FMT_RGB10A2) return launch_kernel<ovrfsr_fast::easu_kernel<I, O>>(grid, dim3(kThreads), lds, s, a);
    return is_masked(a.m) ? easu_fast_go<I, O, true>(pitch, a, grid, s) : easu_fast_go<I, O, false>(pitch, a, grid, s);
}

// The fast RCAS kernels of an RGBA8 source, as two sets with the same three members: the plain instances by destination format, and the
// guarded exact-stores instances (RGBA8 -> RGBA8 only).
template <int O>
struct RcasPlainSet {
    template <bool SPANS, int TH> static constexpr auto dpp() { return &ovrfsr_fast::rcas_dpp_kernel<O, SPANS, TH>; }
    static constexpr auto direct() { return &ovrfsr_fast::rcas_direct_kernel<FMT_RGBA8, O>; }
};
struct RcasExactSet {
    template <bool SPANS, int TH> static constexpr auto dpp() { return &ovrfsr_fast::rcas_dpp_exact_kernel<SPANS, TH>; }
    static constexpr auto direct() { return &ovrfsr_fast::rcas_direct_exact_kernel; }
};

// The form of a fast RCAS launch from an RGBA8 image, one rule for both sets: the DPP kernel on whole rows of 32- or 16-row workgroups
// (unmasked: rcas_dpp_small, fsr_sizes.h), on the span records of a mask-sorted launch, or the per-lane-loads kernel on `grid`.
template <class Set>
static hipError_t rcas_fast_go(bool dpp, const RcasArgs &a, dim3 grid, hipStream_t s)
{
    if (dpp && !a.tileList && !is_masked(a.m)) {
        const uint32_t tx = rcas_dpp_tiles_x(a.v.outW);
        if (rcas_dpp_small(a.v.outW, a.v.outH, grid.z))
            return launch_kernel<*Set::template dpp<false, 16>()>(dim3(tx * rcas_dpp_tiles_y(a.v.outH, 16), 1, grid.z), dim3(kThreads), 0, s, a);
        return launch_kernel<*Set::template dpp<false, kRcasDppTileH>()>(dim3(tx * rcas_dpp_tiles_y(a.v.outH, kRcasDppTileH), 1, grid.z), dim3(kThreads), 0, s, a);
    }
    // mask-sorted form: the DPP kernel on 62-column segments of the runs of tiles touching the radius
    if (dpp && a.tileList && a.spanRec && a.nSpans) return launch_kernel<*Set::template dpp<true, kRcasDppTileH>()>(dim3(a.nSpans, 1, grid.z), dim3(kThreads), 0, s, a);
    return launch_kernel<*Set::direct()>(grid, dim3(kThreads), 0, s, a);
}

template <int I, int O>
static hipError_t rcas_go(bool strict, bool exact, const RcasArgs &a, dim3 grid, hipStream_t s)
{
#ifdef OVRFSR_RCAS_NO_DPP /* measurement build: the per-lane-loads kernel only (reference side of tests/test_gpu_parity.py's DPP equality test) */
    constexpr bool dpp = false;
#else
    constexpr bool dpp = true;
#endif
    if (strict) return launch_kernel<ovrfsr_strict::rcas_kernel<I, O>>(grid, dim3(kThreads), 0, s, a);
    if (exact) {
        // exact stores: the guarded RGBA8 -> RGBA8 instances; no other pair has any
        if constexpr (I == FMT_RGBA8 && O == FMT_RGBA8) return rcas_fast_go<RcasExactSet>(true, a, grid, s);
        else return hipErrorInvalidValue;
    }
    if constexpr (I == FMT_RGBA8 && O != FMT_RGB10A2) return rcas_fast_go<RcasPlainSet<O>>(dpp, a, grid, s);
    else return launch_kernel<ovrfsr_fast::rcas_direct_kernel<I, O>>(grid, dim3(kThreads), 0, s, a);
}

// (which intermediates a source has, and the dynamic-LDS cap: mid_reachable, launch_kernel_big_lds, fsr_launch_impl.h)
template <int I, int M, int O>
struct FusedAny {
    static hipError_t go(bool strict, const FusedArgs &a, dim3 grid, size_t lds, hipStream_t s)
    {
        if (strict) return launch_kernel_big_lds<ovrfsr_strict::fused_kernel<I, M, O, 0>>(grid, dim3(kThreads), lds, s, a);
        return FusedFast<I, M, O>::go(a, grid, lds, s);
    }
};
template <int I, int O>
static hipError_t fused_any_go(int mid_fmt, bool strict, const FusedArgs &a, dim3 grid, size_t lds, hipStream_t s)
{
    return fused_go<FusedAny, I, O, FMT_RGBA8, FMT_RGBA16F, FMT_RGBA32F>(mid_fmt, strict, a, grid, lds, s);
}

hipError_t launch_fused(int prec, int in_fmt, int mid_fmt, int out_fmt, const FusedArgs &a_in, uint32_t batch, hipStream_t s, uint32_t nTiles)
{
    launch_fresh();
    const FusedArgs a = prepared(a_in);
    if (prec != PREC_FP32 && prec != PREC_FP32_STRICT) return hipErrorInvalidValue;
    const bool strict = prec == PREC_FP32_STRICT;
    if (!strict && easu_fast_pitch(a.cellsW) == 0) return hipErrorInvalidValue;
    const dim3 grid = tile_grid(a, nTiles, batch);
    const size_t lds = fused_lds_bytes(prec, in_fmt, mid_fmt, a.cellsW, a.cellsH);
    if (lds > kFusedLdsMax) return hipErrorInvalidValue; // never launch with less LDS than the plane layout assumes (callers pre-check: PrepareResources)
    if (in_fmt == FMT_R11G11B10F) return strict ? hipErrorInvalidValue : launch_fused_packed(mid_fmt, out_fmt, a, grid, lds, s); // fsr_packed_kernels.hip
    OVRFSR_DISPATCH_FMT(OVRFSR_NO_TEN_BIT, fused_any_go, mid_fmt, strict, a, grid, lds, s)
}

template <int I, int O>
static hipError_t easu_outside_any(int mid_fmt, const EasuArgs &a, dim3 grid, hipStream_t s)
{
    return easu_outside_go<I, O, -1, FMT_RGBA32F, FMT_RGBA16F, FMT_RGBA8>(mid_fmt, a, grid, s);
}

// nTiles blocks, each resolving tile a.tileList[block]: tiles entirely outside the radius (product build only).
// mid_fmt < 0: EASU pass only; mid_fmt >= 0: write the FINAL pixel of the EASU->RCAS pipeline (RCAS outside the radius
// is a tinted copy of the intermediate texel, so the intermediate's format rounding is applied in registers).
// LDS-staged outside-tile kernel (outside_staged_kernel): where outside_staged_ok (fsr_sizes.h) says so.
// mid_fmt < 0: the EASU pass alone; >= 0: final pixel = tint(value read back from a mid_fmt intermediate), RGBA32F = tint
// of the un-rounded value (also NIS DirectCopy, tileH = 24).
template <int TH, int I, int O>
static hipError_t outside_staged_go(int mid_fmt, const OutsideArgs &a, dim3 grid, hipStream_t s)
{
    [[maybe_unused]] const size_t lds = (size_t)a.lds_rows * 3 * kOutsidePitch * sizeof(float); // [row][channel][kOutsidePitch]
    if constexpr (I != FMT_RGBA8) {
        return hipErrorInvalidValue;
    } else if constexpr (TH == 24) { // NIS DirectCopy
        return launch_kernel<ovrfsr_fast::outside_staged_kernel<24, I, O, FMT_RGBA32F>>(grid, dim3(8 * 24), lds, s, a);
    } else {
        switch (mid_fmt) { // RGBA8 sources: a UNORM8 or a float intermediate, or the EASU pass alone
        case FMT_RGBA8: return launch_kernel<ovrfsr_fast::outside_staged_kernel<32, I, O, FMT_RGBA8>>(grid, dim3(256), lds, s, a);
        case FMT_RGBA32F: return launch_kernel<ovrfsr_fast::outside_staged_kernel<32, I, O, FMT_RGBA32F>>(grid, dim3(256), lds, s, a);
        case FMT_RGBA16F: return hipErrorInvalidValue;
        default: return launch_kernel<ovrfsr_fast::outside_staged_kernel<32, I, O, -1>>(grid, dim3(256), lds, s, a);
        }
    }
}
template <int I, int O> static hipError_t outside_staged_go32(int mid_fmt, const OutsideArgs &a, dim3 grid, hipStream_t s) { return outside_staged_go<32, I, O>(mid_fmt, a, grid, s); }
template <int I, int O> static hipError_t outside_staged_go24(int mid_fmt, const OutsideArgs &a, dim3 grid, hipStream_t s) { return outside_staged_go<24, I, O>(mid_fmt, a, grid, s); }

hipError_t launch_outside_staged(int tileH, int in_fmt, int mid_fmt, int out_fmt, const OutsideArgs &a_in, uint32_t nTiles, uint32_t batch, hipStream_t s)
{
    launch_fresh();
    OutsideArgs a = prepared(a_in);
    if (!a.tileList || !a.tileRec || !a.bilX || !a.bilY || nTiles == 0 || !outside_staged_ok(a.v, in_fmt)) return hipErrorInvalidValue;
    if (a.lds_cols < 2 || a.lds_cols > 36 || a.lds_rows < 2 || a.lds_rows > 34) return hipErrorInvalidValue;
    // persistent workgroups: block b walks list entries b, b + G, ... (G a multiple of 8: the list is XCD-banded, entry e
    // belongs to band e % 8, so a workgroup stays in its XCD's band), kOutsideTilesPerWg entries each
    a.nTiles = nTiles;
    uint32_t G = ((nTiles + kOutsideTilesPerWg - 1) / kOutsideTilesPerWg + 7u) & ~7u;
    if (G > nTiles) G = nTiles;
    const dim3 grid(G, 1, batch);
    if (tileH == 24) { OVRFSR_DISPATCH_FMT(OVRFSR_NO_TEN_BIT, outside_staged_go24, mid_fmt, a, grid, s) }
    if (tileH != 32) return hipErrorInvalidValue;
    OVRFSR_DISPATCH_FMT(OVRFSR_NO_TEN_BIT, outside_staged_go32, mid_fmt, a, grid, s)
}

// nTiles blocks, each resolving tile a.tileList[block]: tiles entirely outside the radius (product build only).
hipError_t launch_easu_outside(int in_fmt, int mid_fmt, int out_fmt, const EasuArgs &a_in, uint32_t nTiles, uint32_t batch, hipStream_t s)
{
    launch_fresh();
    const EasuArgs a = prepared(a_in);
    if (!a.tileList || nTiles == 0) return hipErrorInvalidValue;
    if (a.bilX && a.bilY && a.tileRec && outside_staged_ok(a.v, in_fmt)) // no records: the per-pixel kernel below needs none
        return launch_outside_staged(kTileH, in_fmt, mid_fmt, out_fmt, outside_args(a, a.debug), nTiles, batch, s);
    const dim3 grid(nTiles, 1, batch);
    if (in_fmt == FMT_R11G11B10F) return launch_easu_outside_packed(mid_fmt, out_fmt, a, grid, s); // fsr_packed_kernels.hip
    OVRFSR_DISPATCH_FMT(OVRFSR_TEN_BIT_PAIRS, easu_outside_any, mid_fmt, a, grid, s)
}

// B8G8R8A8 -> R8G8B8A8 into a tightly packed buffer (dst pitch = 4*w, image stride = 4*w*h): a byte shuffle, 16 texels
// per thread row segment; the pipeline behind it is the RGBA8 one.
__global__ __launch_bounds__(256) void bgra_to_rgba_kernel(const uint8_t *__restrict__ src, uint32_t srcPitch, uint64_t srcStride,
                                                            uint8_t *__restrict__ dst, uint32_t w, uint32_t h)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x, y = blockIdx.y, img = blockIdx.z;
    if (x >= w) return;
    // (checked builds: image `img` of the submission, and the tight copy of the whole batch as one image of gridDim.z * h rows, through the
    // accessors of fsr_bounds.h; the address expressions are the ones the product build has always had)
    OVRFSR_PTR(const uint8_t) s = OVRFSR_IMAGE(const uint8_t, src + (size_t)img * srcStride, srcPitch, (int)w, (int)h, 4u, K_IMAGE_IN);
    OVRFSR_PTR(uint8_t) d = OVRFSR_IMAGE(uint8_t, dst, w * 4u, (int)w, (int)(h * gridDim.z), 4u, K_IMAGE_OUT);
    const uint32_t v = *OVRFSR_AT(const uint32_t, s + (size_t)y * srcPitch + (size_t)x * 4);
    // byte order in memory B,G,R,A -> R,G,B,A: swap bytes 0 and 2
    const uint32_t o = (v & 0xff00ff00u) | ((v >> 16) & 0xffu) | ((v & 0xffu) << 16);
    *OVRFSR_AT(uint32_t, d + ((size_t)img * h + y) * (size_t)w * 4 + (size_t)x * 4) = o;
}

hipError_t launch_bgra_to_rgba(const uint8_t *src, uint32_t srcPitch, uint64_t srcStride, uint8_t *dst, uint32_t w, uint32_t h,
                               uint32_t batch, hipStream_t s)
{
    launch_fresh();
    return launch_kernel<bgra_to_rgba_kernel>(dim3((w + 255) / 256, h, batch), dim3(256), 0, s, src, srcPitch, srcStride, dst, w, h);
}

// one launch of the resolve pass: what both resolve kernels take, and where they run
struct ResolveJob {
    const uint8_t *src; uint32_t srcPitch; uint64_t srcStride; uint8_t *dst; uint32_t dstPitch, w, h, vec;
    dim3 grid; hipStream_t s;
};
template <int F, int S>
static hipError_t resolve_launch(const ResolveJob &j)
{
    if constexpr (F == FMT_R11G11B10F)
        return launch_kernel<ovrfsr_fast::packed_resolve_kernel<S>>(j.grid, dim3(256), 0, j.s, j.src, j.srcPitch, j.srcStride, j.dst, j.dstPitch, j.w, j.h, j.vec);
    else
        return launch_kernel<ovrfsr_fast::resolve_kernel<F, S>>(j.grid, dim3(256), 0, j.s, j.src, j.srcPitch, j.srcStride, j.dst, j.dstPitch, j.w, j.h, j.vec);
}
// the kernel of the run-time sample count; none is built for any other (one sample: R11G11B10F only, which is unpacked whatever the count)
template <int F>
static hipError_t resolve_go(int samples, const ResolveJob &j)
{
    switch (samples) {
    case 1: if constexpr (F == FMT_R11G11B10F) return resolve_launch<F, 1>(j); else break;
    case 2: return resolve_launch<F, 2>(j);
    case 4: return resolve_launch<F, 4>(j);
    case 8: return resolve_launch<F, 8>(j);
    default: break;
    }
    return hipErrorInvalidValue;
}

hipError_t launch_resolve(int fmt, int samples, const uint8_t *src, uint32_t srcPitch, uint64_t srcStride, uint8_t *dst, uint32_t w, uint32_t h,
                          uint32_t batch, hipStream_t s)
{
    launch_fresh();
    // every thread writes 16 bytes: 16 / texel bytes texels, read from samples x 16 source bytes -- R11G11B10F (unpack, and resolve): two
    // texels, 8 x samples source bytes (one 8-byte load at one sample)
    const bool packed = fmt == FMT_R11G11B10F;
    const uint32_t per = 256u * (packed ? 2u : 16u / texel_bytes((uint32_t)fmt));
    const uint32_t vec = rows_vectorizable(src, srcPitch, srcStride, batch, packed && samples == 1 ? 8u : 16u);
    const ResolveJob j{src, srcPitch, srcStride, dst, resolve_pitch(fmt, w), w, h, vec, dim3((w + per - 1) / per, h, batch), s};
    switch (fmt) { // (a format no kernel is built for: hipErrorInvalidValue)
    case FMT_R11G11B10F: return resolve_go<FMT_R11G11B10F>(samples, j);
    case FMT_RGBA8: return resolve_go<FMT_RGBA8>(samples, j);
    case FMT_RGBA16F: return resolve_go<FMT_RGBA16F>(samples, j);
    case FMT_RGBA32F: return resolve_go<FMT_RGBA32F>(samples, j);
    case FMT_RGB10A2: return resolve_go<FMT_RGB10A2>(samples, j);
    case FMT_BGRA8: return resolve_go<FMT_BGRA8>(samples, j);
    default: return hipErrorInvalidValue;
    }
}

#ifdef OVRFSR_BOUNDS
// Drives the checked accessors through every kind of violation exactly once (tests/test_gpu_bounds.py asserts the counts): proof that a
// zero from a campaign means "nothing out of bounds", not "nothing checked".  64 threads, 1024 bytes of dynamic LDS.
__global__ void bounds_selftest_kernel(const uint8_t *img, uint32_t ldsBytes)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using namespace ovrfsr_chk;
    const int lane = threadIdx.x;
    ptr<float> plane = carve<float>(reinterpret_cast<float *>(smem), 64, 16, K_SELFTEST, smem, ldsBytes);
    plane[lane] = (float)lane;                                   // 64 accesses inside the plane
    __syncthreads();
    float sink = 0.0f;
    if (lane == 0) sink += plane[64 + 3];                        // inside the declared pad: 1 pad access
    if (lane == 1) sink += plane[64 + 16];                       // behind the pad: out of bounds
    if (lane == 2) sink += plane[-1];                            // in front of the plane: out of bounds
    // a 12 x 4 image of 4-byte texels with a 64-byte row pitch
    const ptr<const uint8_t> im = image<const uint8_t>(img, 64, 12, 4, 4, K_IMAGE_IN);
    if (lane == 3) sink += (float)*at<const uint32_t>(im + 48);            // row 0, pitch padding: out of bounds
    if (lane == 4) sink += (float)*at<const uint32_t>(im + (3 * 64 + 44)); // the last texel: fine
    if (lane == 5) sink += (float)*at<const uint32_t>(im + (3 * 64 + 48)); // behind the last texel: out of bounds
    if (lane == 6) sink += (float)*at<const uint32_t>(im + 46);            // straddles the end of row 0: out of bounds
    // a plane carved beyond the launch's dynamic LDS: one K_LDS_ALLOC record (thread 0)
    const ptr<float> beyond = carve<float>(reinterpret_cast<float *>(smem) + 250, 16, 0, K_SELFTEST, smem, ldsBytes);
    if (sink == 12345.678f && beyond.p) plane[0] = sink; // keep the reads alive
}
hipError_t bounds_selftest()
{
    uint8_t *img = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&img), 4 * 64);
    if (e != hipSuccess) return e;
    e = hipMemset(img, 1, 4 * 64);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(bounds_selftest_kernel, dim3(1), dim3(64), 1024, nullptr, img, 1024u);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    (void)hipFree(img);
    return e;
}
hipError_t bounds_read_fsr(unsigned long long *out, bool reset) { return ovrfsr_chk::read_counts(out, reset); }
#else
hipError_t bounds_read_fsr(unsigned long long *, bool) { return hipErrorNotSupported; }
hipError_t bounds_selftest() { return hipErrorNotSupported; }
#endif

// audit build: read (and optionally clear) the current device's counters; product build: hipErrorNotSupported
hipError_t tie_audit_read(unsigned long long out[6], bool reset)
{
#ifdef OVRFSR_TIE_AUDIT
    // the instances that read R11G11B10F words count in their own translation unit: sums, and the larger of the two maxima
    unsigned long long p[6];
    hipError_t e = read_counters(HIP_SYMBOL(g_ovrfsr_tie_audit), out, 6, reset);
    if (e == hipSuccess) e = tie_audit_read_packed(p, reset);
    if (e == hipSuccess)
        for (int i = 0; i < 6; ++i) out[i] = i < 4 ? out[i] + p[i] : (p[i] > out[i] ? p[i] : out[i]);
    return e;
#else
    (void)out; (void)reset;
    return hipErrorNotSupported;
#endif
}

// the exact-stores RCAS instances' counters (g_ovrfsr_tie_audit_rcas), same rules
hipError_t tie_audit_read_rcas(unsigned long long out[5], bool reset)
{
#ifdef OVRFSR_TIE_AUDIT
    out[4] = (unsigned long long)ovrfsr_fast::kRcasTieBits; // the band the listed count belongs to: 2^-out[4] byte
    return read_counters(HIP_SYMBOL(g_ovrfsr_tie_audit_rcas), out, 4, reset);
#else
    (void)out; (void)reset;
    return hipErrorNotSupported;
#endif
}

} // namespace ovrfsr
// The forward and back passes of OVRFSR_HDR_DOMAIN_SRTM with their launchers: a file of their own inside this unit (it opens its own
// namespaces) ...
#include "fsr_hdr_domain.inc"
// ... and the tile records of a gaze-capable ctx, built on the device (tile_records_kernel), likewise
#include "fsr_tile_records.inc"
// ... and the tap tables of a rescale-capable ctx, refilled on the device when the input size moves (tap_tables_kernel)
#include "fsr_tap_tables.inc"
// ... and the pass of ovrfsr_set_mask_feather over the band of the radius mask's edge (mask_feather_kernel)
#include "fsr_mask_feather.inc"
namespace ovrfsr {

hipError_t launch_easu(int prec, int in_fmt, int out_fmt, const EasuArgs &a_in, uint32_t batch, hipStream_t s, uint32_t nTiles)
{
    launch_fresh();
    const EasuArgs a = prepared(a_in);
    if (prec != PREC_FP32 && prec != PREC_FP32_STRICT) return hipErrorInvalidValue;
    const bool strict = prec == PREC_FP32_STRICT;
    const dim3 grid = tile_grid(a, nTiles, batch);
    const size_t lds = easu_lds_bytes(prec, in_fmt, a.cellsW, a.cellsH);
    if (in_fmt == FMT_RGBA8_MS4) { // resolve fused into the staging sweep: only where easu_msaa_fused_ok says so
        if (a.tileList || is_masked(a.m) || !easu_msaa_fused_ok(prec, out_fmt, a.cellsW)) return hipErrorInvalidValue;
        return easu_fast_go<FMT_RGBA8_MS4, FMT_RGBA8, false>(easu_kernel_pitch(a.cellsW), a, grid, s);
    }
    if (in_fmt == FMT_R11G11B10F) return strict ? hipErrorInvalidValue : launch_easu_packed(out_fmt, a, grid, s); // fsr_packed_kernels.hip
    OVRFSR_DISPATCH_FMT(OVRFSR_TEN_BIT_PAIRS, easu_go, strict, a, grid, lds, s)
}

hipError_t launch_rcas(int prec, int in_fmt, int out_fmt, const RcasArgs &a_in, uint32_t batch, hipStream_t s, uint32_t nTiles)
{
    launch_fresh();
    RcasArgs a = prepared(a_in);
    a.dppTilesXMagic = div_magic(rcas_dpp_tiles_x(a.v.outW));
    if (prec != PREC_FP32 && prec != PREC_FP32_STRICT && prec != PREC_FP32_EXACT) return hipErrorInvalidValue;
    const bool strict = prec == PREC_FP32_STRICT, exact = prec == PREC_FP32_EXACT;
    if (a.tileList && (strict || nTiles == 0)) return hipErrorInvalidValue; // lists are a product-build feature
    OVRFSR_DISPATCH_FMT(OVRFSR_TEN_BIT_PAIRS, rcas_go, strict, exact, a, tile_grid(a, nTiles, batch), s)
}

} // namespace ovrfsr
