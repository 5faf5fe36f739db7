// fsr_device.inc -- device helpers shared by the FSR and NIS kernels (texel I/O, D3D conversions, radius
// mask, XCD-aware tile map, 8-bit sub-texel bilinear).  Included inside namespace ovrfsr_fast / ovrfsr_strict
// with OVRFSR_STRICT defined.

// ------------------------------------------------------------------------------------------------
// scalar helpers
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float prx_lo_rcp(float a) { return __uint_as_float(0x7ef07ebbu - __float_as_uint(a)); }
__device__ __forceinline__ float prx_lo_rsq(float a) { return __uint_as_float(0x5f347d74u - (__float_as_uint(a) >> 1)); }
__device__ __forceinline__ float prx_med_rcp(float a)
{
    float b = __uint_as_float(0x7ef19fffu - __float_as_uint(a));
    return b * (-b * a + 2.0f);
}
__device__ __forceinline__ float sat01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
__device__ __forceinline__ float rcp_f(float x)
{
#if OVRFSR_STRICT
    return 1.0f / x; // IEEE, correctly rounded (== the oracle's ARcpF1)
#else
    return __builtin_amdgcn_rcpf(x); // v_rcp_f32, <= 1 ulp (what HLSL rcp() is on this vendor's D3D stack)
#endif
}
// a*b+c with two roundings in every build: used where a fused result could flip a floor() or a
// rounding tie relative to the reference (output->input position, UNORM8 store).
__device__ __forceinline__ float mad_unfused(float a, float b, float c)
{
#pragma clang fp contract(off)
    float t = a * b;
    return t + c;
}
// Bilinear blend exactly as the sampler restatement writes it -- every product and sum rounded separately -- in every
// build.  8-bit weights on byte texels put the result on an exact UNORM8 rounding tie very often (5 % of all bytes at
// scale 3/4); which way a tie falls depends on these roundings, so a contracted (FMA) evaluation would disagree with the
// reference on a visible fraction of the pixels outside the radius.  With this, they are bit-identical to the oracle.
__device__ __forceinline__ float bilerp_unfused(float c00, float c10, float c01, float c11, float w00, float w10, float w01, float w11)
{
#pragma clang fp contract(off)
    return ((c00 * w00 + c10 * w10) + c01 * w01) + c11 * w11;
}
// the same blend on tap pairs (c00,c10), (c01,c11) and weight pairs: v_pk_mul_f32 rounds each half like v_mul_f32, so the value is
// bilerp_unfused's, bit for bit, in 2 packed + 3 scalar operations instead of 7
typedef float f2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2_t mk2(float a, float b) { f2_t r = {a, b}; return r; }
__device__ __forceinline__ float bilerp_pk_unfused(f2_t c0, f2_t c1, f2_t w0, f2_t w1)
{
#pragma clang fp contract(off)
    const f2_t a = c0 * w0, b = c1 * w1;
    return ((a.x + a.y) + b.x) + b.y;
}
// o/n correctly rounded, n a constant with rn = RN(1/n): q0 = RN(o*rn), exact remainder by FMA, one correction
// (Markstein).  3 VALU ops instead of the ~11 of an IEEE division; the host checks it against true division for every
// o it will be used with (PostProcessor::PrepareResources) and clears `ok` otherwise.
__device__ __forceinline__ float div_exact(float o, float n, float rn, bool ok)
{
    if (!ok) return o / n;
    const float q0 = o * rn;
    const float r = __builtin_fmaf(-q0, n, o);
    return __builtin_fmaf(r, rn, q0);
}
template <bool EXACT>
__device__ __forceinline__ float bilerp(float c00, float c10, float c01, float c11, float w00, float w10, float w01, float w11)
{
    if constexpr (EXACT) return bilerp_unfused(c00, c10, c01, c11, w00, w10, w01, w11);
    else return ((c00 * w00 + c10 * w10) + c01 * w01) + c11 * w11;
}
// b/255 correctly rounded for every integer b in [0,255] (D3D UNORM8 -> float) in two operations: 1/255 as a double-float
// constant k_hi + k_lo; fma(b, k_hi, RN(b*k_lo)) rounds b/255 + O(2^-48), and no b/255 lies that close to a rounding
// boundary (verified for all 256 values against exact rational arithmetic: tests/test_constants.py).
__device__ __forceinline__ float unorm8_to_unit(float b)
{
    const float k_hi = __uint_as_float(0x3b808081u), k_lo = __uint_as_float(0xaf7efeffu);
    return __builtin_fmaf(b, k_hi, b * k_lo);
}
// floor(sat(x)*255+0.5): D3D float -> UNORM8 (documented at fsr/ffx_fsr1.h:1075-1080)
__device__ __forceinline__ uint32_t unit_to_unorm8(float x) { return (uint32_t)mad_unfused(sat01(x), 255.0f, 0.5f); }
// floor(sat(x)*1023+0.5): float -> UNORM10 (R10G10B10A2_UNORM, the reference's texture format for 10-bit submissions,
// PostProcessor.cpp:63-74)
__device__ __forceinline__ uint32_t unit_to_unorm10(float x) { return (uint32_t)mad_unfused(sat01(x), 1023.0f, 0.5f); }

// Near-tie guard of the product build (easu_fast_kernel, fused_kernel): is a byte-domain value v in [0,255] within
// +-2^-TIE_BITS of a UNORM8 rounding boundary k + 0.5?  v + 256 has a fixed exponent (ulp 2^-15), so the low 15 mantissa
// bits are frac(v) in fixed point; adding 2^-TIE_BITS as well turns the two-sided band test into one masked compare.
// One fast-class add, one and, one compare per channel.  The product build's re-associated EASU differs from the
// reference-order evaluation by at most 6.5e-4 byte (measured over 1e8 values incl. uniform-random and 0/255-only
// content, profiles/r03_easu_err.txt; none above 2^-10 = 9.8e-4); the default band, 2^-9 = 1.95e-3, is 3 times that.
constexpr int kTieBits = 9;
// (K: the band's bit count -- kTieBits for EASU stores, kRcasTieBits for the exact-stores RCAS instances.  v + bias is rounded to 2^-15, so
// the band's edges sit within 2^-16 byte of where the comment puts them: 1.6 % of the narrowest band accepted)
template <int K = kTieBits>
__device__ __forceinline__ bool near_tie_byte(float v)
{
    static_assert(K >= 3 && K <= 12, "band half-width 2^-K byte");
    constexpr float bias = 256.0f + 1.0f / (float)(1 << K);
    constexpr uint32_t mask = ((1u << (K - 1)) - 1u) << (16 - K);
    return (__float_as_uint(v + bias) & mask) == 0x4000u;
}

// min/max of values that are known not to be NaN (LDS colour planes hold bytes or finite texels).  fminf/fmaxf
// on a loaded value makes the compiler emit a canonicalising `v_max_f32 x, x, x` first (IEEE sNaN quieting),
// one slow-class VALU op per operand; the raw instructions skip that.  Product build only.
__device__ __forceinline__ float raw_min3(float a, float b, float c) { float r; __asm__("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ float raw_max3(float a, float b, float c) { float r; __asm__("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ float raw_min(float a, float b) { float r; __asm__("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float raw_max(float a, float b) { float r; __asm__("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }

#define OVRFSR_RCAS_LIMIT ((float)(0.25 - (1.0 / 16.0))) /* fsr/ffx_fsr1.h:654 */

// FsrRcasF's lobe (ffx_fsr1.h:722-738) times sharp, from the per-channel extrema of the four ring taps in the BYTE domain (P = 255) --
// one quotient per channel instead of the reference's two.  For 0 <= mn <= mx <= P:
//     max(-mn/(4mx), (P-mx)/(4mn-4P)) = -min(mn, P-mx) / (4 min(mx, P-mn)),
// since mn/mx <= (P-mx)/(P-mn) <=> mn + mx <= P, where both minima pick (mn, mx); otherwise both pick (P-mx, P-mn).  The extrema of
// bytes are integers, so the selection is exact and the winning quotient is the very fp32 expression the two-quotient form evaluates
// (v_rcp_f32 is odd and scales exactly with powers of two).  Not for the unit domain: values above 1 break 0 <= mx <= P.
//   * The 4 of the denominator is a power of two: it moves, exactly, into the clamp limit and the sharpness factor (one multiply per
//     thread instead of one per channel).
//   * mn = mx in {0, P} gives 0 * rcp(0) = NaN where the two-quotient form drops its NaN against the other quotient's -1/4 ("this
//     channel does not limit").  Here v_min3_f32 drops it, and if all three channels are NaN, v_med3_f32 answers
//     min3(NaN, -4 LIMIT, 0) = -4 LIMIT: the same clamped lobe.
// tests/test_gpu_rcas_identity.py compares this helper with the two-quotient form on the device, bit for bit, over every (mn, mx).
__device__ __forceinline__ float rcas_lobe_bytes(float mnR, float mxR, float mnG, float mxG, float mnB, float mxB, float sharp)
{
    constexpr float P = 255.0f;
    const float qR = raw_min(mnR, P - mxR) * __builtin_amdgcn_rcpf(raw_min(mxR, P - mnR));
    const float qG = raw_min(mnG, P - mxG) * __builtin_amdgcn_rcpf(raw_min(mxG, P - mnG));
    const float qB = raw_min(mnB, P - mxB) * __builtin_amdgcn_rcpf(raw_min(mxB, P - mnB));
    return __builtin_amdgcn_fmed3f(-raw_min3(qR, qG, qB), -4.0f * OVRFSR_RCAS_LIMIT, 0.0f) * (0.25f * sharp);
}

// The same guard for RGBA16F stores (round 4 form): is a positive x, about to be rounded to half, within 2^-TIE_HALF_BITS of a
// half SPACING of a rounding boundary?  The low 13 bits of the fp32 pattern are x's position inside its half spacing in
// fixed point (boundary = 0x1000), whatever the binade: the band follows x's magnitude, as the re-association error it covers
// does (it is relative to the magnitude of the taps; measured <= 2.6e-6 in the unit domain, profiles/r03_easu_err.txt; the
// default 2^-6 of a spacing is 2^-17 = 7.6e-6 for values in [0.5, 1), 3 times that, and grows with the binade for HDR values).
// half_tie_code(x) == 0 iff x is in the band and x >= xmin: integer adds / ands / ors only; a pixel tests
// min3(codes) == 0.  Only channels >= xmin are guarded: a flipped half-ulp below xmin stays under the 1e-3
// tolerance even behind RCAS's largest gain (the host derives xmin from the sharpness: 0.25 or 0.5; +inf when no sharpening
// pass follows).  Rounds 2-3 tested |x - half(x)| against an ABSOLUTE 2^-17 per channel (7 VALU per channel, and no cover at
// all above 2.0 where the spacing outgrows the band).
constexpr int kTieHalfBits = 6;
__device__ __forceinline__ uint32_t half_tie_code(float x, uint32_t xmin_bits)
{
    constexpr uint32_t W = 1u << (13 - kTieHalfBits);      // band half-width in units of 2^-13 spacing
    static_assert(kTieHalfBits >= 2 && kTieHalfBits <= 12, "band = 2^-K of a half spacing");
    constexpr uint32_t M = 0x1fffu & ~(2u * W - 1u);
    const uint32_t bits = __float_as_uint(x);
    // 0 iff x is inside the band AND x >= xmin: below xmin (and for negative x) the unsigned difference wraps or the sign bit is set
    return (((bits + W) & M) ^ 0x1000u) | (((bits - xmin_bits) | bits) & 0x80000000u);
}
// a pixel is listed when one of its channels is: min3 of the codes == 0 (xmin = +inf: never)
__device__ __forceinline__ bool near_tie_half3(float r, float g, float b, float xmin)
{
    const uint32_t xb = __float_as_uint(xmin);
    uint32_t m;
    __asm__("v_min3_u32 %0, %1, %2, %3" : "=v"(m) : "v"(half_tie_code(r, xb)), "v"(half_tie_code(g, xb)), "v"(half_tie_code(b, xb)));
    return m == 0u;
}

// HDR tiles (round 5).  The re-association error the guard covers is proportional to the LARGEST TAP of the pixel (measured <= 2.6e-6 x
// max tap), the band above to the OUTPUT's binade: fine while every texel is <= 1 (the band of an output in [0.5, 1) is 2^-17 >= 3 x 2.6e-6),
// too narrow where a tap is many times the output -- a dark pixel next to an HDR highlight (round 4's adversarial search: taps 40x the output,
// 2.9 bands).  Tiles whose staged footprint holds a texel > 1 (tmax, the footprint's largest channel magnitude, workgroup-uniform) therefore
// test an ABSOLUTE band of 2^-(11+K) * tmax -- the unit-range band scaled with the largest value any tap can have: with e = x's exponent the
// band is (2^-(1+K) tmax) * 2^-e half spacings; x's low 13 mantissa bits, moved to the top of a [1, 2) float, minus 1.5 is its distance
// from the rounding boundary in spacings.  A band >= 0.5 spacing lists every pixel (a tile mixing a highlight with dark content is
// then resolved in reference order throughout).
__device__ __forceinline__ bool near_tie_half_abs(float x, float band_pre /* 2^-(1+K) * tmax */, float xmin)
{
    const uint32_t bits = __float_as_uint(x);
    const float t = __uint_as_float(((bits << 10) & 0x007ffc00u) | 0x3f800000u) - 1.5f;      // (p - 4096) / 8192, p = bits & 0x1fff
    const float thr = band_pre * __uint_as_float(0x7f000000u - (bits & 0x7f800000u));          // band_pre * 2^-e
    return (int)(fabsf(t) < thr) & (int)(x >= xmin);
}
__device__ __forceinline__ bool near_tie_half3_hdr(float r, float g, float b, float xmin, float tmax)
{
    constexpr float kPre = 1.0f / (float)(1u << (1 + kTieHalfBits));
    if (tmax <= 1.0f) return near_tie_half3(r, g, b, xmin); // workgroup-uniform: unit-range footprints keep the binade-relative band
    const float bp = kPre * tmax;
    return (int)near_tie_half_abs(r, bp, xmin) | (int)near_tie_half_abs(g, bp, xmin) | (int)near_tie_half_abs(b, bp, xmin);
}

// The same guard for UNORM8 stores of FLOAT sources (cfg.reference_formats: the reference's R8G8B8A8_UNORM intermediate of an HDR
// submission).  x: a unit-domain channel of the product resolve; what is stored is floor(sat(x) * 255 + 0.5), so the test runs on
// sat(x) * 255: is it within `band` bytes of a rounding boundary k + 0.5?  band = 2^-kTieBits byte (the byte guard's) x max(1, tmax), tmax
// the largest |channel| of the tile's staged footprint (the HDR half guard's reasoning: the re-association error follows the largest
// tap, not the output, and 2^-9 byte = 2^-17 of the unit range is that guard's band).  Saturated channels sit at 0 or 255, half a byte
// from the nearest boundary: they are listed only where the band reaches 0.5 byte (tmax >= 256) -- there a product value just above 1
// can be a strict value just below 254.5 / 255, and every pixel of the tile is re-resolved in reference order.  band = 0: never (guard off).
__device__ __forceinline__ bool near_tie_unorm8_unit(float x, float band)
{
    const float v = sat01(x) * 255.0f;
    return fabsf((v - floorf(v)) - 0.5f) < band;
}
__device__ __forceinline__ bool near_tie_unorm8_unit3(float r, float g, float b, float band)
{
    return (int)near_tie_unorm8_unit(r, band) | (int)near_tie_unorm8_unit(g, band) | (int)near_tie_unorm8_unit(b, band);
}

typedef _Float16 half_t;
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
typedef _Float16 half4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// ------------------------------------------------------------------------------------------------
// texel I/O on linear buffers (the reference binds SRVs/UAVs: PostProcessor.cpp:387-392)
// ------------------------------------------------------------------------------------------------
template <int FMT> struct TexelBytes;
template <> struct TexelBytes<ovrfsr::FMT_RGBA8> { static constexpr int v = 4; };
template <> struct TexelBytes<ovrfsr::FMT_RGBA16F> { static constexpr int v = 8; };
template <> struct TexelBytes<ovrfsr::FMT_RGBA32F> { static constexpr int v = 16; };
template <> struct TexelBytes<ovrfsr::FMT_RGB10A2> { static constexpr int v = 4; };
template <> struct TexelBytes<ovrfsr::FMT_RGBA8_MS4> { static constexpr int v = 16; }; // one texel = its 4 samples
template <> struct TexelBytes<ovrfsr::FMT_R11G11B10F> { static constexpr int v = 4; };  // one packed word (product build: decoded where it is staged / loaded)

// R11G11B10F word -> fp32 (r, g, b) (header, OVRFSR_FORMAT_R11G11B10F): R bits 0-10, G 11-21, B 22-31, each the half float whose bits are the
// channel's bits shifted left by 4 (R, G) or 5 (B) -- exact for every code, denormals, Inf and NaN included; alpha reads 1.0 (the callers'
// constant).  These are the fp32 values a load of the resolve pass's RGBA16F copy (packed_resolve_kernel) delivers, bit for bit.
__device__ __forceinline__ void unpack_r11g11b10f(uint32_t w, float &r, float &g, float &b)
{
    r = (float)__builtin_bit_cast(_Float16, (uint16_t)((w & 0x7ffu) << 4));
    g = (float)__builtin_bit_cast(_Float16, (uint16_t)(((w >> 11) & 0x7ffu) << 4));
    b = (float)__builtin_bit_cast(_Float16, (uint16_t)((w >> 22) << 5));
}

// The multisample resolve rule of UNORM8 channels (header, OVRFSR_FORMAT_MS): per channel (sum + S/2) >> log2 S.  R+B and G+A sum as two
// 16-bit lanes per dword (8 x 255 + 4 fits a lane; the shift moves nothing across the mask).  resolve_kernel and the resolving staging
// sweep of easu_fast_kernel both call this: what the fused path stages is what the resolve pass writes.
template <uint32_t S>
__device__ __forceinline__ uint32_t resolve_unorm8(const uint32_t *v)
{
    constexpr uint32_t L = S == 2 ? 1u : S == 4 ? 2u : 3u;
    uint32_t rb = (S / 2) * 0x00010001u, ga = rb;
#pragma unroll
    for (uint32_t sm = 0; sm < S; ++sm) {
        rb += v[sm] & 0x00ff00ffu;
        ga += (v[sm] >> 8) & 0x00ff00ffu;
    }
    return ((rb >> L) & 0x00ff00ffu) | (((ga >> L) & 0x00ff00ffu) << 8);
}

// The images and device tables of a kernel, declared through the checked accessors of fsr_bounds.h (plain pointers in the product build).
// OVRFSR_IMAGES needs `a` (the kernel's argument block) and `img_i` in scope and declares `in` / `out`.
#ifndef OVRFSR_IMAGES
#ifdef OVRFSR_BOUNDS
#define OVRFSR_IMAGES(IF, OF)                                                                                                          \
    const ovrfsr_chk::ptr<const uint8_t> in = ovrfsr_chk::image<const uint8_t>(a.v.in + (size_t)img_i * a.v.in_stride, a.v.in_pitch, a.v.inW, a.v.inH, \
                                                                                (uint32_t)TexelBytes<IF>::v, ovrfsr_chk::K_IMAGE_IN);     \
    const ovrfsr_chk::ptr<uint8_t> out = ovrfsr_chk::image<uint8_t>(a.v.out + (size_t)img_i * a.v.out_stride, a.v.out_pitch, a.v.outW, a.v.outH, \
                                                                    (uint32_t)TexelBytes<OF>::v, ovrfsr_chk::K_IMAGE_OUT)
// tile / group list of a launch: one entry per workgroup (blockIdx.x); records: 4 dwords per entry of the persistent kernel's list;
// span records: 2 dwords per workgroup; column taps: [outW] entries, read in whole quads of whole 32-pixel tiles -- the host pads them to a
// multiple of 32 with copies of the last tap (PrepareResources); row taps: [outH] entries
#define OVRFSR_TILE_LIST(a) ovrfsr_chk::ptr<const uint32_t>((a).tileList, gridDim.x, 0, ovrfsr_chk::K_TILE_LIST)
#define OVRFSR_TILE_REC(a) ovrfsr_chk::ptr<const uint32_t>((a).tileRec, 4ull * (a).nTiles, 0, ovrfsr_chk::K_TILE_REC)
#define OVRFSR_SPAN_REC(a) ovrfsr_chk::ptr<const uint32_t>((a).spanRec, 2ull * gridDim.x, 0, ovrfsr_chk::K_SPAN_REC)
#define OVRFSR_BIL_X(a) ovrfsr_chk::ptr<const ovrfsr::BilinTap>((a).bilX, (a).v.outW, (32 - ((a).v.outW & 31)) & 31, ovrfsr_chk::K_BIL_X)
#define OVRFSR_BIL_Y(a) ovrfsr_chk::ptr<const ovrfsr::BilinTap>((a).bilY, (a).v.outH, 0, ovrfsr_chk::K_BIL_Y)
#else
#define OVRFSR_IMAGES(IF, OF)                                                    \
    const uint8_t *__restrict__ in = a.v.in + (size_t)img_i * a.v.in_stride;     \
    uint8_t *__restrict__ out = a.v.out + (size_t)img_i * a.v.out_stride
#define OVRFSR_TILE_LIST(a) (a).tileList
#define OVRFSR_TILE_REC(a) (a).tileRec
#define OVRFSR_SPAN_REC(a) (a).spanRec
#define OVRFSR_BIL_X(a) (a).bilX
#define OVRFSR_BIL_Y(a) (a).bilY
#endif
#endif

// unit-domain ([0,1]) RGBA of texel (x,y); x,y already in range
// IMG: const uint8_t * (product build) or its checked form (fsr_bounds.h)
template <int FMT, typename IMG>
__device__ __forceinline__ float4 load_unit(IMG img, uint32_t pitch, int x, int y)
{
    const auto p = img + (size_t)y * pitch + (size_t)x * TexelBytes<FMT>::v;
    if constexpr (FMT == ovrfsr::FMT_RGBA8) {
        uint32_t v = *OVRFSR_AT(const uint32_t, p);
        return make_float4(unorm8_to_unit((float)(v & 0xffu)), unorm8_to_unit((float)((v >> 8) & 0xffu)),
                           unorm8_to_unit((float)((v >> 16) & 0xffu)), unorm8_to_unit((float)(v >> 24)));
    } else if constexpr (FMT == ovrfsr::FMT_RGBA16F) {
        half4_t h = *OVRFSR_AT(const half4_t, p);
        return make_float4((float)h.x, (float)h.y, (float)h.z, (float)h.w);
    } else if constexpr (FMT == ovrfsr::FMT_RGB10A2) {
        // DXGI_FORMAT_R10G10B10A2_UNORM: R in bits 0-9, G 10-19, B 20-29, A 30-31; UNORM decode k/1023, a/3 (IEEE division:
        // correctly rounded in every build; this format is not a throughput path)
        const uint32_t v = *OVRFSR_AT(const uint32_t, p);
        return make_float4((float)(v & 1023u) / 1023.0f, (float)((v >> 10) & 1023u) / 1023.0f, (float)((v >> 20) & 1023u) / 1023.0f,
                           (float)(v >> 30) / 3.0f);
    } else if constexpr (FMT == ovrfsr::FMT_R11G11B10F) {
        float4 c;
        unpack_r11g11b10f(*OVRFSR_AT(const uint32_t, p), c.x, c.y, c.z);
        c.w = 1.0f;
        return c;
    } else {
        return *OVRFSR_AT(const float4, p);
    }
}

// the same from a 32-bit byte offset off the (uniform) image base: every image spans at most 4 GiB (CheckImage), so the
// address is base + zero-extended VGPR offset -- one 32-bit add per texel instead of a 64-bit multiply-add chain
template <int FMT, typename IMG>
__device__ __forceinline__ float4 load_unit_off(IMG img, uint32_t off)
{
    const auto p = img + off;
    if constexpr (FMT == ovrfsr::FMT_RGBA8) {
        const uint32_t v = *OVRFSR_AT(const uint32_t, p);
        return make_float4(unorm8_to_unit((float)(v & 0xffu)), unorm8_to_unit((float)((v >> 8) & 0xffu)),
                           unorm8_to_unit((float)((v >> 16) & 0xffu)), unorm8_to_unit((float)(v >> 24)));
    } else if constexpr (FMT == ovrfsr::FMT_RGBA16F) {
        const half4_t h = *OVRFSR_AT(const half4_t, p);
        return make_float4((float)h.x, (float)h.y, (float)h.z, (float)h.w);
    } else if constexpr (FMT == ovrfsr::FMT_RGB10A2) {
        const uint32_t v = *OVRFSR_AT(const uint32_t, p);
        return make_float4((float)(v & 1023u) / 1023.0f, (float)((v >> 10) & 1023u) / 1023.0f, (float)((v >> 20) & 1023u) / 1023.0f,
                           (float)(v >> 30) / 3.0f);
    } else if constexpr (FMT == ovrfsr::FMT_R11G11B10F) {
        float4 c;
        unpack_r11g11b10f(*OVRFSR_AT(const uint32_t, p), c.x, c.y, c.z);
        c.w = 1.0f;
        return c;
    } else {
        return *OVRFSR_AT(const float4, p);
    }
}
// min(max(v, 0), hi) as one v_med3_i32 (hi >= 0)
__device__ __forceinline__ int clamp0(int v, int hi) { int r; __asm__("v_med3_i32 %0, %1, 0, %2" : "=v"(r) : "v"(v), "v"(hi)); return r; }

// store unit-domain RGBA
template <int FMT, typename IMG>
__device__ __forceinline__ void store_unit(IMG img, uint32_t pitch, int x, int y, float r, float g, float b, float a)
{
    const auto p = img + (size_t)y * pitch + (size_t)x * TexelBytes<FMT>::v;
    if constexpr (FMT == ovrfsr::FMT_RGBA8) {
        uint32_t v = unit_to_unorm8(r) | (unit_to_unorm8(g) << 8) | (unit_to_unorm8(b) << 16) | (unit_to_unorm8(a) << 24);
        *OVRFSR_AT(uint32_t, p) = v;
    } else if constexpr (FMT == ovrfsr::FMT_RGBA16F) {
#if OVRFSR_STRICT
        // keep "round to fp32, then to fp16": without the barrier the backend folds a preceding fmul into
        // v_fma_mixlo_f16 (one rounding), which is not what a D3D fp32 shader + RGBA16F store does
        __asm__ volatile("" : "+v"(r), "+v"(g), "+v"(b), "+v"(a));
#endif
        half4_t h = {(half_t)r, (half_t)g, (half_t)b, (half_t)a};
        *OVRFSR_AT(half4_t, p) = h;
    } else if constexpr (FMT == ovrfsr::FMT_RGB10A2) {
        *OVRFSR_AT(uint32_t, p) = unit_to_unorm10(r) | (unit_to_unorm10(g) << 10) | (unit_to_unorm10(b) << 20) |
                                           ((uint32_t)mad_unfused(sat01(a), 3.0f, 0.5f) << 30);
    } else {
        *OVRFSR_AT(float4, p) = make_float4(r, g, b, a);
    }
}

// ------------------------------------------------------------------------------------------------
// radius mask (fsr_easu.hlsl:41-45 == fsr_rcas.hlsl:32-36): uint32 wrap-around arithmetic on the
// centre of each 16x16 group
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool group_inside(uint32_t gx, uint32_t gy, const uint32_t c[4], uint32_t r2)
{
    uint32_t cx = (gx << 4) + 8u, cy = (gy << 4) + 8u;
    uint32_t d1x = c[0] - cx, d1y = c[1] - cy, d2x = c[2] - cx, d2y = c[3] - cy;
    return (d1x * d1x + d1y * d1y <= r2) || (d2x * d2x + d2y * d2y <= r2);
}

// bit (gx&1) + 2*(gy&1) of the result = group (2*tileX + gx, 2*tileY + gy) is inside
__device__ __forceinline__ uint32_t tile_mask_bits(const ovrfsr::MaskArgs &m, uint32_t eye, uint32_t tileX, uint32_t tileY)
{
    uint32_t mode = m.mode[eye];
    if (mode == ovrfsr::MASK_ALL_INSIDE) return 0xfu;
    if (mode == ovrfsr::MASK_ALL_OUTSIDE) return 0u;
    uint32_t bits = 0;
#pragma unroll
    for (uint32_t g = 0; g < 4; ++g)
        bits |= (group_inside(2 * tileX + (g & 1u), 2 * tileY + (g >> 1), m.centre[eye], m.r2) ? 1u : 0u) << g;
    return bits;
}

// tile -> (tileX, tileY) without a hardware divide (see div_magic, fsr_params.h)
__device__ __forceinline__ void tile_xy(uint32_t tile, uint32_t tilesX, uint32_t magic, uint32_t &tileX, uint32_t &tileY)
{
    tileY = magic ? __umulhi(tile, magic) : tile;
    tileX = tile - tileY * tilesX;
}

// XCD-aware block -> tile map: consecutive block ids are dispatched round-robin over the 8 XCDs
// (each with a private 4 MiB L2), so give XCD k the k-th contiguous band of tiles and neighbouring
// tiles (which share their input apron) meet in the same L2.  Pure performance: any bijection is correct.
__device__ __forceinline__ uint32_t xcd_tile_index(uint32_t b, uint32_t n)
{
    const uint32_t full = n & ~7u; // the n%8 trailing blocks keep their own index
    return (b < full) ? ((b & 7u) * (full >> 3) + (b >> 3)) : b;
}

// Lane -> position permutation for kernels whose lanes read float4 LDS cells at consecutive positions.  A ds_read_b128 is
// served in four groups of 16 lanes -- {0-3,12-15,20-27}, {4-11,16-19,28-31} and the same +32 (MI355X_MICROARCH.md, LDS)
// -- and a cell takes 4 of the 64 banks, so a group is conflict-free iff its lanes read at most 16 consecutive cells.
// With lanes in pixel order a group spans 28 pixels = 21+ cells at scale 3/4 (2-way conflicts: 42 % of the LDS cycles of
// the round-1 EASU kernel).  This maps the low 5 bits of a lane index so that each group gets 16 CONSECUTIVE positions;
// a row of 32 pixels is still one 128-byte store segment.
// (the permutation also keeps every group of 8 consecutive lanes -- the unit of a ds_write_b128 -- on 8 distinct cells
// mod 8, so a plane WRITTEN in lane order of this map is conflict-free as well: the fused kernel's intermediate plane)
__device__ __forceinline__ int lane32_to_pos(int l5) { return l5 + (int)((0x1000081808182010ull >> (8 * (l5 >> 2))) & 0xffu) - 16; }

// D3D11 fixed-point texel addressing: texel-space coordinate snapped to 8 fractional bits, round to nearest
__device__ __forceinline__ void fixed8(float t, int &i0, float &frac)
{
    const float s = floorf(mad_unfused(t, 256.0f, 0.5f));
    const float f = floorf(s * (1.0f / 256.0f));
    i0 = (int)f;
    frac = mad_unfused(f, -256.0f, s) * (1.0f / 256.0f); // exact: s, f*256 are integers < 2^24
}

// bilinear SampleLevel(linearClamp, pos/outSize) straight from global memory (fsr_easu.hlsl:33-36).
// texel space = u*W-0.5, 8-bit sub-texel weights, clamp addressing.  Returns unit-domain RGBA.
template <int IN_FMT, typename IMG>
__device__ __forceinline__ float4 bilinear_uv(IMG img, uint32_t pitch, int inW, int inH, float u, float v)
{
    const float tx = mad_unfused(u, (float)inW, -0.5f), ty = mad_unfused(v, (float)inH, -0.5f);
    int x0, y0;
    float fx, fy;
    fixed8(tx, x0, fx);
    fixed8(ty, y0, fy);
    int xa = clampi(x0, 0, inW - 1), xb = clampi(x0 + 1, 0, inW - 1);
    int ya = clampi(y0, 0, inH - 1), yb = clampi(y0 + 1, 0, inH - 1);
    float4 c00 = load_unit<IN_FMT>(img, pitch, xa, ya), c10 = load_unit<IN_FMT>(img, pitch, xb, ya);
    float4 c01 = load_unit<IN_FMT>(img, pitch, xa, yb), c11 = load_unit<IN_FMT>(img, pitch, xb, yb);
    float w00 = (1.0f - fx) * (1.0f - fy), w10 = fx * (1.0f - fy), w01 = (1.0f - fx) * fy, w11 = fx * fy;
    float4 o;
    o.x = bilerp_unfused(c00.x, c10.x, c01.x, c11.x, w00, w10, w01, w11);
    o.y = bilerp_unfused(c00.y, c10.y, c01.y, c11.y, w00, w10, w01, w11);
    o.z = bilerp_unfused(c00.z, c10.z, c01.z, c11.z, w00, w10, w01, w11);
    o.w = bilerp_unfused(c00.w, c10.w, c01.w, c11.w, w00, w10, w01, w11);
    return o;
}

template <int IN_FMT, typename IMG>
__device__ __forceinline__ float4 bilinear_global(IMG img, uint32_t pitch, int inW, int inH, int x, int y, float outWf, float outHf)
{
    return bilinear_uv<IN_FMT>(img, pitch, inW, inH, (float)x / outWf, (float)y / outHf);
}

