// hdr_map.h -- FSR 1's Simple Reversible Tone-Mapper (FsrSrtmF / FsrSrtmInvF, src/fsr/ffx_fsr1.h:1029-1046) as OVRFSR_HDR_DOMAIN_SRTM applies
// it (header, "HDR domain"): linear HDR -> {0 to 1} in front of the filters and back behind them, RGB ratios preserved, alpha untouched.
// ONE function for the host (ovrfsr_hdr_map, capi.cpp) and the device (fsr_hdr_domain.inc), evaluated as written so that the two agree
// bit for bit: fp32, one rounding per operator, IEEE division, nothing that can contract (no a * b + c in here), max as a comparison.
// Covered values: finite, >= 0.  The round trip is not the identity: the back mapping's divisor is clamped at 1/32768.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OVRFSR_HOST_DEVICE __host__ __device__
#else
#define OVRFSR_HOST_DEVICE
#endif

namespace ovrfsr {

OVRFSR_HOST_DEVICE inline float hdr_max(float a, float b) { return a > b ? a : b; }

// forward: k = 1 / (max3 + 1); back: k = 1 / max(1/32768, 1 - max3)
OVRFSR_HOST_DEVICE inline void hdr_map(float &r, float &g, float &b, bool inverse)
{
    const float m = hdr_max(hdr_max(r, g), b);
    const float k = 1.0f / (inverse ? hdr_max(1.0f / 32768.0f, 1.0f - m) : m + 1.0f);
    r *= k; g *= k; b *= k;
}

// fp32 -> the bits of the nearest half, ties to even, overflow to Inf: the RGBA16F store conversion of the back pass, in integer arithmetic.
// Written out because the value it converts is a product (texel * k): handed to the compiler as a float-to-half conversion, the backend
// folds the multiplication into v_fma_mixlo_f16 -- one rounding where "an fp32 result, then an RGBA16F store" has two.  Equal to the
// hardware conversion for every fp32 that is not a NaN (all 2^32 patterns compared on the host); a NaN gives the quiet NaN 0x7e00.
OVRFSR_HOST_DEVICE inline unsigned hdr_half_bits(float x)
{
    const unsigned u = __builtin_bit_cast(unsigned, x), sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return sign | 0x7e00u;
    if (a >= 0x38800000u) {                                     // 2^-14 and above: a normal half, or Inf
        const unsigned v = a - 0x38000000u;                     // exponent re-biased (127 -> 15), 23 mantissa bits
        const unsigned r = (v + 0xfffu + ((v >> 13) & 1u)) >> 13;
        return sign | (r < 0x7c00u ? r : 0x7c00u);
    }
    if (a <= 0x33000000u) return sign;                          // 2^-25 (a tie, to even) and below: zero
    const unsigned s = 126u - (a >> 23), m = (a & 0x7fffffu) | 0x800000u; // a denormal half: m * 2^-s units of 2^-24, s in [14, 24]
    const unsigned q = m >> s, rem = m & ((1u << s) - 1u), tie = 1u << (s - 1u);
    return sign | (q + ((rem > tie || (rem == tie && (q & 1u))) ? 1u : 0u));
}

} // namespace ovrfsr
