// nis_kernels.inc -- NVIDIA Image Scaling (NVScaler, NVSharpen) for gfx950, written from scratch.
// Included twice by nis_kernels.hip (namespace ovrfsr_fast: contraction on; ovrfsr_strict: every
// operator as written, IEEE division -> bit-identical to oracle/nis_oracle.c).
//
// What is computed is fixed by the reference (file:line under /root/reference/src):
//   nis/NIS_Scaler.h:160-169 getY, :176-293 GetEdgeMap, :343-375 CalcLTI, :399-434 EvalPoly6,
//   :436-453 FilterNormal, :455-583 GetDirFilters, :377-397 GetInterpEdgeMap, :589-770 NVScaler,
//   :790-971 CalcLTIFast/EvalUSM/GetDirUSM/NVSharpen; entry points + radius mask + DirectCopy
//   nis/NIS_Upscale.hlsl:77-107, nis/NIS_Sharpen.hlsl:75-105.
// How: one 256-thread workgroup per mask group (32x24 output pixels for the scaler, 32x32 for the
// sharpener -- the reference's own group sizes, because the radius test is per group).  The input
// footprint is staged once: RGBA8 unpacked once per texel into an LDS luma plane (unit and x255),
// the per-texel edge map (GetEdgeMap depends only on the 3x3 lumas around a texel) into an LDS
// float4 plane, the two 64x8 coefficient banks into LDS.  The shader's float index arithmetic for
// its 2x2 staging batches is not reproduced: every tile cell is a pure function of its texel.
// The chroma tap (one bilinear sample per output pixel, 8-bit sub-texel weights as D3D11 defines)
// is read from global memory (L1/L2 resident: the same texels were just staged).

__device__ __forceinline__ float nis_lerp(float x, float y, float s) { return x + s * (y - x); }
// getY (NIS_Scaler.h:160-169) is evaluated as written -- three products and two sums, each rounded -- in EVERY build.  The
// luma feeds GetEdgeMap's hard thresholds (g_max > g_min*kDetectRatio, > kDetectThres, equality selects): a contracted
// (FMA) luma differs by an ulp, flips a comparison on a near-tie and an edge weight jumps 0 <-> 1 (round 1's product build
// was 0.05 off the oracle on such pixels).  With the unfused luma the edge maps of the product build are the oracle's.
__device__ __forceinline__ float nis_getY(float r, float g, float b)
{
#pragma clang fp contract(off)
    return 0.2126f * r + 0.7152f * g + 0.0722f * b;
}
__device__ __forceinline__ float nis_div(float a, float b)
{
#if OVRFSR_STRICT
    return a / b;
#else
    return a * __builtin_amdgcn_rcpf(b);
#endif
}

// NIS_Scaler.h:176-293 on the 3x3 block q (row-major, q[r*3+c])
#if OVRFSR_STRICT
__device__ __forceinline__ float4 nis_edge_map(const float q[9], float kDetectRatio, float kDetectThres)
{
    const float g_0 = fabsf(q[0] + q[1] + q[2] - q[6] - q[7] - q[8]);
    const float g_45 = fabsf(q[3] + q[0] + q[1] - q[7] - q[8] - q[5]);
    const float g_90 = fabsf(q[0] + q[3] + q[6] - q[2] - q[5] - q[8]);
    const float g_135 = fabsf(q[3] + q[6] + q[7] - q[1] - q[2] - q[5]);
    const float g_0_90_max = fmaxf(g_0, g_90), g_0_90_min = fminf(g_0, g_90);
    const float g_45_135_max = fmaxf(g_45, g_135), g_45_135_min = fminf(g_45, g_135);
    float e_0_90 = 0.0f, e_45_135 = 0.0f;
    if ((g_0_90_max + g_45_135_max) != 0.0f) {
        e_0_90 = nis_div(g_0_90_max, (g_0_90_max + g_45_135_max));
        e_0_90 = fminf(e_0_90, 1.0f);
        e_45_135 = 1.0f - e_0_90;
    }
    float edge_0 = 0.0f, edge_45 = 0.0f, edge_90 = 0.0f, edge_135 = 0.0f;
    if ((g_0_90_max > (g_0_90_min * kDetectRatio)) && (g_0_90_max > kDetectThres) && (g_0_90_max > g_45_135_min)) {
        if (g_0_90_max == g_0) edge_0 = 1.0f; else edge_90 = 1.0f;
    }
    if ((g_45_135_max > (g_45_135_min * kDetectRatio)) && (g_45_135_max > kDetectThres) && (g_45_135_max > g_0_90_min)) {
        if (g_45_135_max == g_45) edge_45 = 1.0f; else edge_135 = 1.0f;
    }
    const float esum = edge_0 + edge_90 + edge_45 + edge_135;
    float4 w = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (esum >= 2.0f) {
        w.x = (edge_0 == 1.0f) ? e_0_90 : 0.0f;
        w.y = (edge_0 == 1.0f) ? 0.0f : e_0_90;
        w.z = (edge_45 == 1.0f) ? e_45_135 : 0.0f;
        w.w = (edge_45 == 1.0f) ? 0.0f : e_45_135;
    } else if (esum >= 1.0f) {
        w = make_float4(edge_0, edge_90, edge_45, edge_135);
    }
    return w;
}
#else
// Product build: the same decisions and the same values, without the float edge flags, their sum and the two levels of
// divergent branches.  With A / B = "an edge in {0,90} / {45,135} was detected":
//   both      -> (A0 ? e_0_90 : 0, A90 ? e_0_90 : 0, B45 ? e_45_135 : 0, B135 ? e_45_135 : 0)      (esum == 2)
//   only one  -> 1 in the slot of the detected direction                                              (esum == 1)
// i.e. slot = flag ? (other pair detected ? e : 1) : 0.  e_0_90 is only read when A and B hold, where both maxima exceed
// kDetectThres > 0, so the reference's guard against a zero denominator is never the deciding branch there.
// Compares land in SGPR masks and combine on the scalar unit; ~46 VALU instead of ~70 per texel.
__device__ __forceinline__ float4 nis_edge_map(const float q[9], float kDetectRatio, float kDetectThres)
{
    const float d_0 = q[0] + q[1] + q[2] - q[6] - q[7] - q[8];
    const float d_45 = q[3] + q[0] + q[1] - q[7] - q[8] - q[5];
    const float d_90 = q[0] + q[3] + q[6] - q[2] - q[5] - q[8];
    const float d_135 = q[3] + q[6] + q[7] - q[1] - q[2] - q[5];
    float g_0_90_max, g_0_90_min, g_45_135_max, g_45_135_min; // |x| as source modifiers: no separate abs / canonicalise ops
    __asm__("v_max_f32 %0, |%1|, |%2|" : "=v"(g_0_90_max) : "v"(d_0), "v"(d_90));
    __asm__("v_min_f32 %0, |%1|, |%2|" : "=v"(g_0_90_min) : "v"(d_0), "v"(d_90));
    __asm__("v_max_f32 %0, |%1|, |%2|" : "=v"(g_45_135_max) : "v"(d_45), "v"(d_135));
    __asm__("v_min_f32 %0, |%1|, |%2|" : "=v"(g_45_135_min) : "v"(d_45), "v"(d_135));
    // Both edge tests require their maximum gradient to exceed kDetectThres; where no lane of the wave has one that does,
    // every weight is 0 (exact): smooth regions skip the ratio, the division and the selects.
    if (__builtin_amdgcn_ballot_w64((g_0_90_max > kDetectThres) || (g_45_135_max > kDetectThres)) == 0)
        return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const bool A = (g_0_90_max > (g_0_90_min * kDetectRatio)) && (g_0_90_max > kDetectThres) && (g_0_90_max > g_45_135_min);
    const bool B = (g_45_135_max > (g_45_135_min * kDetectRatio)) && (g_45_135_max > kDetectThres) && (g_45_135_max > g_0_90_min);
    const bool is0 = g_0_90_max == fabsf(d_0), is45 = g_45_135_max == fabsf(d_45);
    const float e_0_90 = fminf(g_0_90_max * __builtin_amdgcn_rcpf(g_0_90_max + g_45_135_max), 1.0f);
    const float e_45_135 = 1.0f - e_0_90;
    const float vA = B ? e_0_90 : 1.0f, vB = A ? e_45_135 : 1.0f;
    return make_float4((A && is0) ? vA : 0.0f, (A && !is0) ? vA : 0.0f, (B && is45) ? vB : 0.0f, (B && !is45) ? vB : 0.0f);
}
#endif

// LDS row of a coefficient phase (8 floats per row).  Neighbouring output pixels are fx = scale apart, so the lanes of a
// read hit a handful of phases that are multiples of 64*scale apart -- 16, 32, 48 at scale 3/4 --, and with rows in phase
// order (phase*8 dwords) those alias onto the same 8 banks: 4-way conflicts on every fx-phase lookup.  Rows are stored
// as ((phase & 15) << 2) | (phase >> 4): phases 16 apart become neighbouring rows (distinct banks), consecutive phases sit
// 4 rows = 32 dwords apart.  Any bijection of the 64 rows is correct; this one is nis_load_coefs' and the lookups'.
__device__ __forceinline__ int nis_coef_row(int phase) { return (((phase & 15) << 2) | (phase >> 4)) * 8; }

// cell types of the x255 luma plane and the edge-map plane.  (The reference's NIS_USE_HALF_PRECISION mode, NIS_Scaler.h:133-148 -- these
// two planes in half / half4, arithmetic in float -- was measured in round 3: 4.9e-3 off and half the speed, profiles/r03_nis_variants.txt.)
typedef float nis_lum_t;
typedef float4 nis_edge_t;
__device__ __forceinline__ float4 nis_edge_load(const float4 &e) { return e; }
__device__ __forceinline__ void nis_edge_store(float4 &d, const float4 &e) { d = e; }

struct NisTune { // the tuning floats of NISConfig the filters read
    float kMinContrastRatio, kRatioNorm, kContrastBoost, kEps;
    float kSharpStartY, kSharpScaleY, kSharpStrengthMin, kSharpStrengthScale, kSharpLimitMin, kSharpLimitScale;
};

// NIS_Scaler.h:343-375
__device__ __forceinline__ float nis_calc_lti(const float p[6], int phase_index, const NisTune &t)
{
    const bool lo = phase_index <= 32;
    const float y0 = lo ? p[0] : p[1], y1 = lo ? p[1] : p[2], y2 = lo ? p[2] : p[3], y3 = lo ? p[3] : p[4], y4 = lo ? p[4] : p[5];
    const float a_min = fminf(fminf(y0, y1), y2), a_max = fmaxf(fmaxf(y0, y1), y2);
    const float b_min = fminf(fminf(y2, y3), y4), b_max = fmaxf(fmaxf(y2, y3), y4);
    const float a_cont = a_max - a_min, b_cont = b_max - b_min;
    const float cont_ratio = nis_div(fmaxf(a_cont, b_cont), (fminf(a_cont, b_cont) + t.kEps));
    return (1.0f - sat01((cont_ratio - t.kMinContrastRatio) * t.kRatioNorm)) * t.kContrastBoost;
}

// NIS_Scaler.h:399-434.  cs/cu: LDS coefficient banks [64][8]
__device__ __forceinline__ float nis_eval_poly6(const float pxl[6], int phase_int, const NisTune &t, OVRFSR_PTR_C(float) cs, OVRFSR_PTR_C(float) cu)
{
    const int row = nis_coef_row(phase_int);
    const float4 s0 = *OVRFSR_AT(const float4, cs + row);
    const float2 s1 = *OVRFSR_AT(const float2, cs + row + 4);
    const float4 u0 = *OVRFSR_AT(const float4, cu + row);
    const float2 u1 = *OVRFSR_AT(const float2, cu + row + 4);
    float y = 0.f;
    y += s0.x * pxl[0]; y += s0.y * pxl[1]; y += s0.z * pxl[2]; y += s0.w * pxl[3]; y += s1.x * pxl[4]; y += s1.y * pxl[5];
    float y_usm = 0.f;
    y_usm += u0.x * pxl[0]; y_usm += u0.y * pxl[1]; y_usm += u0.z * pxl[2]; y_usm += u0.w * pxl[3]; y_usm += u1.x * pxl[4]; y_usm += u1.y * pxl[5];
    const float y_scale = 1.0f - sat01((y * (1.0f / 255) - t.kSharpStartY) * t.kSharpScaleY);
    const float y_sharpness = y_scale * t.kSharpStrengthScale + t.kSharpStrengthMin;
    y_usm *= y_sharpness;
    const float y_sharpness_limit = (y_scale * t.kSharpLimitScale + t.kSharpLimitMin) * y;
    y_usm = fminf(y_sharpness_limit, fmaxf(-y_sharpness_limit, y_usm));
    y_usm *= nis_calc_lti(pxl, phase_int, t);
    return y + y_usm;
}

// NVScaler for one output pixel.  Y255: LDS luma plane (x255), E: LDS edge plane, both pitch PITCH;
// c0 = index of the pixel's top-left support cell (texel floor(srcX)-2, floor(srcY)-2).
// vcol (product build): the vertical half of FilterNormal for this pixel's output row, shared through LDS -- vcol[j] =
// sum_i p[i][j] * coef_y[i] of support column j, computed once per (output row, texel column) instead of by every pixel that
// reads the column (see nis_scaler_kernel); nullptr = evaluate the 6x6 here, as the reference writes it.
template <int PITCH>
__device__ __forceinline__ float nis_scaler_luma(OVRFSR_PTR_RC(nis_lum_t) Y255, OVRFSR_PTR_RC(nis_edge_t) E, int c0, float fx, float fy,
                                                 const NisTune &t, OVRFSR_PTR_C(float) cs, OVRFSR_PTR_C(float) cu, OVRFSR_PTR_RC(float) vcol = nullptr)
{
    float p[6][6];
    const int fx_int = (int)(fx * 64), fy_int = (int)(fy * 64);
    auto load_support = [&]() {
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) p[i][j] = (float)Y255[c0 + i * PITCH + j];
    };

    // FilterNormal, NIS_Scaler.h:436-453
    float pixel_n;
    if (vcol) {
        const int rowx = nis_coef_row(fx_int);
        const float4 b0 = *OVRFSR_AT(const float4, cs + rowx);
        const float2 b1 = *OVRFSR_AT(const float2, cs + rowx + 4);
        const float cx[6] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y};
        float h_acc = 0.0f;
#pragma unroll
        for (int j = 0; j < 6; ++j) h_acc += vcol[j] * cx[j];
        pixel_n = h_acc;
    } else {
        load_support();
        const int rowy = nis_coef_row(fy_int), rowx = nis_coef_row(fx_int);
        const float4 a0 = *OVRFSR_AT(const float4, cs + rowy);
        const float2 a1 = *OVRFSR_AT(const float2, cs + rowy + 4);
        const float4 b0 = *OVRFSR_AT(const float4, cs + rowx);
        const float2 b1 = *OVRFSR_AT(const float2, cs + rowx + 4);
        const float cy[6] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y};
        const float cx[6] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y};
        float h_acc = 0.0f;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            float v_acc = 0.0f;
#pragma unroll
            for (int i = 0; i < 6; ++i) v_acc += p[i][j] * cy[i];
            h_acc += v_acc * cx[j];
        }
        pixel_n = h_acc;
    }

    // GetInterpEdgeMap (NIS_Scaler.h:377-397) of the 2x2 edge maps centred in the 6x6 support, x NIS_SCALE_INT
    const float4 e00 = nis_edge_load(E[c0 + 2 * PITCH + 2]), e01 = nis_edge_load(E[c0 + 2 * PITCH + 3]), e10 = nis_edge_load(E[c0 + 3 * PITCH + 2]),
                 e11 = nis_edge_load(E[c0 + 3 * PITCH + 3]);
    const float wx = nis_lerp(nis_lerp(e00.x, e01.x, fx), nis_lerp(e10.x, e11.x, fx), fy) * 255;
    const float wy = nis_lerp(nis_lerp(e00.y, e01.y, fx), nis_lerp(e10.y, e11.y, fx), fy) * 255;
    const float wz = nis_lerp(nis_lerp(e00.z, e01.z, fx), nis_lerp(e10.z, e11.z, fx), fy) * 255;
    const float ww = nis_lerp(nis_lerp(e00.w, e01.w, fx), nis_lerp(e10.w, e11.w, fx), fy) * 255;
    // NIS_Scaler.h:741-742
    // Exact early-out: where no edge was detected around the pixel all four weights are exactly 0 and the
    // directional filters are multiplied by 0 (NIS_Scaler.h:741).  f*0 = +-0 and 0 + x = x, so skipping them when
    // the whole wave agrees is bit-identical; smooth image regions (most of a frame) take this branch.
    if (__builtin_amdgcn_ballot_w64((wx != 0.0f) || (wy != 0.0f) || (wz != 0.0f) || (ww != 0.0f)) == 0)
        return (pixel_n * 255.0f) * (1.0f / 255.0f);
    if (vcol) load_support(); // the directional filters read the 6x6 lumas themselves: only waves that meet an edge fetch them

    // GetDirFilters, NIS_Scaler.h:455-583.  A direction whose weight is 0 in every lane of the wave is skipped
    // (f*0 = +-0 contributes nothing): sporadic single-direction edges then cost one filter, not four.
    float f0 = 0.0f, f1 = 0.0f, f2 = 0.0f, f3 = 0.0f;
    if (__builtin_amdgcn_ballot_w64(wx != 0.0f) != 0) {
        float d[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) d[i] = nis_lerp(p[i][2], p[i][3], fx);
        f0 = nis_eval_poly6(d, fy_int, t, cs, cu);
    }
    if (__builtin_amdgcn_ballot_w64(wy != 0.0f) != 0) {
        float d[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) d[i] = nis_lerp(p[2][i], p[3][i], fy);
        f1 = nis_eval_poly6(d, fx_int, t, cs, cu);
    }
    if (__builtin_amdgcn_ballot_w64(wz != 0.0f) != 0) {
        float b45 = 0.5f + 0.5f * (fx - fy);
        float t1 = nis_lerp(p[2][1], p[1][2], b45), t3 = nis_lerp(p[3][2], p[2][3], b45), t5 = nis_lerp(p[4][3], p[3][4], b45);
        const bool hi = b45 >= 0.5f;
        b45 = hi ? (b45 - 0.5f) : (0.5f - b45);
        const float t0 = nis_lerp(p[1][1], hi ? p[0][2] : p[2][0], b45);
        const float t2 = nis_lerp(p[2][2], hi ? p[1][3] : p[3][1], b45);
        const float t4 = nis_lerp(p[3][3], hi ? p[2][4] : p[4][2], b45);
        const float t6 = nis_lerp(p[4][4], hi ? p[3][5] : p[5][3], b45);
        float p45 = fx + fy;
        const bool sh = p45 >= 1;
        const float d[6] = {sh ? t1 : t0, sh ? t2 : t1, sh ? t3 : t2, sh ? t4 : t3, sh ? t5 : t4, sh ? t6 : t5};
        p45 = sh ? (p45 - 1) : p45;
        f2 = nis_eval_poly6(d, (int)(p45 * 64), t, cs, cu);
    }
    if (__builtin_amdgcn_ballot_w64(ww != 0.0f) != 0) {
        float b135 = 0.5f * (fx + fy);
        float t1 = nis_lerp(p[3][1], p[4][2], b135), t3 = nis_lerp(p[2][2], p[3][3], b135), t5 = nis_lerp(p[1][3], p[2][4], b135);
        const bool hi = b135 >= 0.5f;
        b135 = hi ? (b135 - 0.5f) : (0.5f - b135);
        const float t0 = nis_lerp(p[4][1], hi ? p[5][2] : p[3][0], b135);
        const float t2 = nis_lerp(p[3][2], hi ? p[4][3] : p[2][1], b135);
        const float t4 = nis_lerp(p[2][3], hi ? p[3][4] : p[1][2], b135);
        const float t6 = nis_lerp(p[1][4], hi ? p[2][5] : p[0][3], b135);
        float p135 = 1 + (fx - fy);
        const bool sh = p135 >= 1;
        const float d[6] = {sh ? t1 : t0, sh ? t2 : t1, sh ? t3 : t2, sh ? t4 : t3, sh ? t5 : t4, sh ? t6 : t5};
        p135 = sh ? (p135 - 1) : p135;
        f3 = nis_eval_poly6(d, (int)(p135 * 64), t, cs, cu);
    }

    return (f0 * wx + f1 * wy + f2 * wz + f3 * ww + pixel_n * (255.0f - wx - wy - wz - ww)) * (1.0f / 255.0f);
}

__device__ __forceinline__ void nis_load_coefs(OVRFSR_PTR_RC(float) gScale, OVRFSR_PTR_RC(float) gUsm, OVRFSR_PTR(float) cs, OVRFSR_PTR(float) cu)
{
    // 2 x 512 floats, 256 threads x float4
    // float4 t of a bank = half (t & 1) of phase row t >> 1, stored at the swizzled row (nis_coef_row)
    const int t = threadIdx.x & 127;
    const OVRFSR_PTR(float) g = threadIdx.x < 128 ? gScale : gUsm;
    OVRFSR_PTR(float) d = threadIdx.x < 128 ? cs : cu;
    *OVRFSR_AT(float4, d + nis_coef_row(t >> 1) + 4 * (t & 1)) = *OVRFSR_AT(const float4, OVRFSR_AS(const float4, g) + t);
}

// NIS radius test, NIS_Upscale.hlsl:98-101 (block 32 x BH, centre +16,+BH/2)
__device__ __forceinline__ bool nis_group_inside(uint32_t bx, uint32_t by, uint32_t bh, const uint32_t c[4], uint32_t r2)
{
    const uint32_t cx = bx * 32u + 16u, cy = by * bh + bh / 2u;
    const uint32_t d1x = c[0] - cx, d1y = c[1] - cy, d2x = c[2] - cx, d2y = c[3] - cy;
    return (d1x * d1x + d1y * d1y <= r2) || (d2x * d2x + d2y * d2y <= r2);
}

// NVScaler pass.  grid = (groupsX*groupsY, 1, batch), block 256, one 32x24 output group per workgroup.
// Dynamic LDS: Yu[PITCH*rows] | Y255[PITCH*rows] | E[PITCH*rows] (float4) | cs[512] | cu[512].
template <int IN_FMT, int OUT_FMT, int PITCH>
__global__ __launch_bounds__(256) void nis_scaler_kernel(const ovrfsr::NisArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    OVRFSR_LDS_POISON(smem, a.ldsBytes);
    constexpr int BW = 32, BH = 24;
    const uint32_t img_i = blockIdx.z;
    const uint32_t eye = (a.m.first_eye ^ (img_i & a.m.alternate)) & 1u;
    const uint32_t grp = a.tileList ? OVRFSR_TILE_LIST(a)[blockIdx.x] : xcd_tile_index(blockIdx.x, a.tilesX * a.tilesY);
    uint32_t bx, by;
    tile_xy(grp, a.tilesX, a.tilesXMagic, bx, by);
    OVRFSR_IMAGES(IN_FMT, OUT_FMT);
    const int inW = a.v.inW, inH = a.v.inH, outW = a.v.outW, outH = a.v.outH;
    const float dbg = a.reserved1;

    const uint32_t mode = a.m.mode[eye];
    const bool inside = mode == ovrfsr::MASK_ALL_INSIDE ? true
                      : mode == ovrfsr::MASK_ALL_OUTSIDE ? false : nis_group_inside(bx, by, BH, a.m.centre[eye], a.m.r2);
    const int dstBlockX = BW * (int)bx, dstBlockY = BH * (int)by;

    if (!inside) {
        // DirectCopy, NIS_Upscale.hlsl:77-90: bilinear at pos/outSize, tint, alpha = 1
        for (int k = threadIdx.x; k < BW * BH; k += ovrfsr::kThreads) {
            const int dstX = dstBlockX + (k & 31), dstY = dstBlockY + (k >> 5);
            if (dstX >= outW || dstY >= outH) continue;
            const float4 c = bilinear_uv<IN_FMT>(in, a.v.in_pitch, inW, inH, (float)dstX / (float)outW, (float)dstY / (float)outH);
            store_unit<OUT_FMT>(out, a.v.out_pitch, dstX, dstY, sat01(c.x * (1 - dbg * 0)), sat01(c.y * (1 - dbg * 0.3f)), sat01(c.z * (1 - dbg * 0.3f)), 1.0f * (1 - dbg * 0));
        }
        return;
    }

    // input footprint: cell (cx,cy) <-> texel (X0 - 3 + cx, Y0 - 3 + cy); X0 = floor(srcX of first pixel)
    const int X0 = (int)floorf(mad_unfused(0.5f + dstBlockX, a.kScaleX, -0.5f));
    const int Y0 = (int)floorf(mad_unfused(0.5f + dstBlockY, a.kScaleY, -0.5f));
    const int rows = a.cellsH;
    const int ncell = PITCH * rows;
    // (the unit-luma plane later holds the BH x PITCH vertical sums V: rows >= BH whenever V is used)
    OVRFSR_PTR(float) Yu = OVRFSR_CARVE(float, reinterpret_cast<float *>(smem), ncell, 0, K_NIS_YU, smem, a.ldsBytes);
    OVRFSR_PTR(nis_lum_t) Y255 = OVRFSR_CARVE(nis_lum_t, reinterpret_cast<nis_lum_t *>(OVRFSR_RAW(Yu) + ncell), ncell, 0, K_NIS_Y255, smem, a.ldsBytes);
    OVRFSR_PTR(nis_edge_t) E = OVRFSR_CARVE(nis_edge_t, reinterpret_cast<nis_edge_t *>(OVRFSR_RAW(Yu) + 2 * ncell), ncell, 0, K_NIS_EDGE, smem, a.ldsBytes);
    OVRFSR_PTR(float) cs = OVRFSR_CARVE(float, OVRFSR_RAW(Yu) + 6 * ncell, 512, 0, K_NIS_COEF_LDS, smem, a.ldsBytes);
    OVRFSR_PTR(float) cu = OVRFSR_CARVE(float, OVRFSR_RAW(cs) + 512, 512, 0, K_NIS_COEF_LDS, smem, a.ldsBytes);
    nis_load_coefs(OVRFSR_PLANE_C(float, a.coefScale, 512, 0, K_NIS_COEF), OVRFSR_PLANE_C(float, a.coefUsm, 512, 0, K_NIS_COEF), cs, cu);

#if !OVRFSR_STRICT
    // per output row of the group: the row's fractional source position, the LDS row of its 6x6 support and of its chroma
    // tap, and the tap's sub-texel weight -- the same for the 32 pixels of a row, so 24 lanes compute them once (the same
    // expressions the pixel loop used to evaluate per pixel: ~22 VALU instructions per pixel less)
    OVRFSR_LDS_ARRAY(float4, rowinfo, BH, K_NIS_ROWINFO);
    if (threadIdx.x < BH) {
        const int dstY = dstBlockY + (int)threadIdx.x;
        const float srcY = mad_unfused(0.5f + dstY, a.kScaleY, -0.5f);
        const float fly = floorf(srcY);
        int tapy; float tfy;
        fixed8(mad_unfused((dstY + 0.5f) * a.kDstNormY, (float)inH, -0.5f), tapy, tfy);
        rowinfo[threadIdx.x] = make_float4(srcY - fly, __int_as_float(((int)fly - Y0 + 1) * PITCH), __int_as_float((tapy - (Y0 - 3)) * PITCH), tfy);
    }
    // product build, RGBA8 input: the raw texel is kept in LDS too, so that the chroma tap (below) needs neither
    // global addressing nor clamping (cells are staged with clamped coordinates) and blends in the byte domain
    constexpr bool kRawTap = IN_FMT == ovrfsr::FMT_RGBA8;
    OVRFSR_PTR(uint32_t) RAW = OVRFSR_CARVE(uint32_t, reinterpret_cast<uint32_t *>(OVRFSR_RAW(cu) + 512), ncell, 0, K_NIS_RAW, smem, a.ldsBytes);
#endif
    bool staged = false;
#if !OVRFSR_STRICT
    if constexpr (kRawTap) {
        // groups whose footprint lies inside the image (all but the border groups; workgroup-uniform): a lane takes 4
        // consecutive texels with one 16-byte load -- no clamps, no per-texel index split or 64-bit addressing -- and writes
        // the 4 lumas / scaled lumas / raw texels with one 16-byte LDS store each (27 -> 15 VALU instructions per texel)
        static_assert(PITCH % 4 == 0, "quad staging needs a row pitch that is a multiple of 4 cells");
        if (X0 - 3 >= 0 && Y0 - 3 >= 0 && X0 - 3 + PITCH <= inW && Y0 - 3 + rows <= inH) {
            typedef uint32_t u32x4_a4_t __attribute__((ext_vector_type(4), aligned(4)));
            constexpr int SEGS = PITCH / 4;
            OVRFSR_PTR_R(const uint8_t) base = in + ((size_t)(Y0 - 3) * a.v.in_pitch + (size_t)(X0 - 3) * 4u);
#pragma clang loop vectorize(disable) interleave(disable)
#pragma unroll 1
            for (int t = threadIdx.x; t < SEGS * rows; t += ovrfsr::kThreads) {
                const int row = t / SEGS, seg = t - row * SEGS;
                const u32x4_a4_t v = *OVRFSR_AT(const u32x4_a4_t, base + ((uint32_t)row * a.v.in_pitch + (uint32_t)seg * 16u));
                const int idx = row * PITCH + 4 * seg;
                float y[4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    y[j] = nis_getY(unorm8_to_unit((float)(v[j] & 0xffu)), unorm8_to_unit((float)((v[j] >> 8) & 0xffu)),
                                    unorm8_to_unit((float)((v[j] >> 16) & 0xffu)));
                *OVRFSR_AT(float4, Yu + idx) = make_float4(y[0], y[1], y[2], y[3]);
                *OVRFSR_AT(float4, Y255 + idx) = make_float4(y[0] * 255.0f, y[1] * 255.0f, y[2] * 255.0f, y[3] * 255.0f);
                *OVRFSR_AT(u32x4_a4_t, RAW + idx) = v;
            }
            staged = true;
        }
    }
#endif
    if (!staged)
    for (int idx = threadIdx.x; idx < ncell; idx += ovrfsr::kThreads) {
        const int cy = idx / PITCH, cx = idx - cy * PITCH;
        const int sx = clampi(X0 - 3 + cx, 0, inW - 1), sy = clampi(Y0 - 3 + cy, 0, inH - 1);
        const float4 c = load_unit<IN_FMT>(in, a.v.in_pitch, sx, sy);
        const float y = nis_getY(c.x, c.y, c.z);
        Yu[idx] = y;
        Y255[idx] = (nis_lum_t)(y * 255.0f);
#if !OVRFSR_STRICT
        if constexpr (kRawTap) RAW[idx] = *OVRFSR_AT(const uint32_t, in + (uint32_t)sy * a.v.in_pitch + (uint32_t)sx * 4u);
#endif
    }
    __syncthreads();
    // edge maps are read at cells (celly+2..3, cellx+2..3) with celly in [1, rows-6]: rows 3 .. rows-3
    for (int idx = 3 * PITCH + threadIdx.x; idx < ncell - 2 * PITCH; idx += ovrfsr::kThreads) {
        // border columns wrap into neighbouring rows: finite garbage in cells never used as edge texels
        const float q[9] = {Yu[idx - PITCH - 1], Yu[idx - PITCH], Yu[idx - PITCH + 1], Yu[idx - 1], Yu[idx], Yu[idx + 1],
                            Yu[idx + PITCH - 1], Yu[idx + PITCH], Yu[idx + PITCH + 1]};
        const float4 w = nis_edge_map(q, a.kDetectRatio, a.kDetectThres);
        nis_edge_store(E[idx], w);
    }
    __syncthreads();
#if !OVRFSR_STRICT
    // FilterNormal (NIS_Scaler.h:436-453) is separable as written: v_acc[j] = sum_i p[i][j] * coef_y[i], then
    // sum_j v_acc[j] * coef_x[j].  v_acc depends on the output ROW (its fy phase and support rows) and the texel COLUMN only,
    // and 32 pixels x 6 columns per row share 31 columns: computed here once per (row, column) -- same products, same order --
    // into the unit-luma plane, which nothing reads after the edge map.  A pixel then costs 6 reads + 6 FMAs instead of 36 + 42,
    // and waves without an edge (most of a frame) never fetch their 6x6 lumas at all.
    OVRFSR_PTR(float) V = Yu;
    const bool useV = kRawTap && rows >= BH; // the plane holds BH rows of PITCH sums: smaller footprints (> 1.4x upscales) keep the 6x6 form
    if (useV) { // workgroup-uniform
#pragma unroll 1
        for (int idx = threadIdx.x; idx < BH * PITCH; idx += ovrfsr::kThreads) {
            const int r = idx / PITCH, c = idx - r * PITCH;
            const float4 ri = rowinfo[r];
            const int rowy = nis_coef_row((int)(ri.x * 64));
            const float4 a0 = *OVRFSR_AT(const float4, cs + rowy);
            const float2 a1 = *OVRFSR_AT(const float2, cs + rowy + 4);
            const float cy[6] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y};
            // support rows of output row r, column c (rows beyond the plane only for cells no pixel of the group reads)
            const OVRFSR_PTR(nis_lum_t) yp = Y255 + min(__float_as_int(ri.y), (rows - 6) * PITCH) + c;
            float v_acc = 0.0f;
#pragma unroll
            for (int i = 0; i < 6; ++i) v_acc += (float)yp[i * PITCH] * cy[i];
            V[idx] = v_acc;
        }
        __syncthreads();
    }
#endif

    NisTune t;
    t.kMinContrastRatio = a.kMinContrastRatio; t.kRatioNorm = a.kRatioNorm; t.kContrastBoost = a.kContrastBoost; t.kEps = a.kEps;
    t.kSharpStartY = a.kSharpStartY; t.kSharpScaleY = a.kSharpScaleY; t.kSharpStrengthMin = a.kSharpStrengthMin;
    t.kSharpStrengthScale = a.kSharpStrengthScale; t.kSharpLimitMin = a.kSharpLimitMin; t.kSharpLimitScale = a.kSharpLimitScale;

    // (Round 4 measured this pixel loop in two passes with the edge lanes compacted into an LDS list: 10 % fewer VALU instructions, 11 %
    // slower -- a barrier and a one-wave tail per workgroup, scattered LDS reads: profiles/r04_nis_compaction.txt.)
    // product build, 4-byte output texels: lanes permuted so that every 16-lane ds_read_b128 group (the edge-map plane)
    // reads 16 consecutive cells (lane32_to_pos, fsr_device.inc); a row of 32 pixels stays one 128-byte store line
    const int lx = (OVRFSR_STRICT == 0 && TexelBytes<OUT_FMT>::v == 4) ? lane32_to_pos(threadIdx.x & 31) : (int)(threadIdx.x & 31);
    const int dstX = dstBlockX + lx;
    if (dstX >= outW) return;
    const float srcX = mad_unfused(0.5f + dstX, a.kScaleX, -0.5f); // unfused in every build: floor() must pick the reference's texel
    const float flx = floorf(srcX);
    const float fx = srcX - flx;
    const int cellx = (int)flx - X0 + 1; // support starts at texel floor(srcX)-2 = cell (floor(srcX) - X0 + 1)
#if !OVRFSR_STRICT
    int tapx; float tfx; // chroma tap column: same position math as bilinear_uv, resolved to an LDS cell
    fixed8(mad_unfused((dstX + 0.5f) * a.kDstNormX, (float)inW, -0.5f), tapx, tfx);
    tapx -= X0 - 3;
#endif
#pragma unroll 1
    for (int k = 0; k < 3; ++k) {
        const int dstY = dstBlockY + (int)(threadIdx.x >> 5) + 8 * k;
        if (dstY >= outH) break;
#if OVRFSR_STRICT
        const float srcY = mad_unfused(0.5f + dstY, a.kScaleY, -0.5f);
        const float fly = floorf(srcY);
        const float fy = srcY - fly;
        const int crow = ((int)fly - Y0 + 1) * PITCH;
#else
        const float4 ri = rowinfo[(threadIdx.x >> 5) + 8 * k];
        const float fy = ri.x;
        const int crow = __float_as_int(ri.y);
#endif
#if OVRFSR_STRICT
        const float opY = nis_scaler_luma<PITCH>(Y255, E, crow + cellx, fx, fy, t, cs, cu);
#else
        const float opY = nis_scaler_luma<PITCH>(Y255, E, crow + cellx, fx, fy, t, cs, cu, useV ? V + ((threadIdx.x >> 5) + 8 * k) * PITCH + cellx : nullptr);
#endif
#if !OVRFSR_STRICT
        if constexpr (kRawTap) {
            // chroma tap (NIS_Scaler.h:747,758-761) from the staged raw texels, blended in the byte domain: the
            // weighted byte sum is exact in fp32, so this is closer to the real-number result than the reference's
            // unit-domain blend; the tap always lies inside the 6x6 support (|tap - src| < 1 texel)
            const float tfy = ri.w;
            const OVRFSR_PTR(uint32_t) rp = RAW + __float_as_int(ri.z) + tapx;
            const uint32_t t00 = rp[0], t10 = rp[1], t01 = rp[PITCH], t11 = rp[PITCH + 1];
            const float w11 = tfx * tfy, w10 = tfx - w11, w01 = tfy - w11, w00 = (1.0f - tfx) - w01;
            float o[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int sh = 8 * c;
                o[c] = (float)((t00 >> sh) & 0xffu) * w00 + (float)((t10 >> sh) & 0xffu) * w10 +
                       (float)((t01 >> sh) & 0xffu) * w01 + (float)((t11 >> sh) & 0xffu) * w11;
            }
            const float corr = opY - nis_getY(o[0], o[1], o[2]); // opY is in the x255 domain
            const float r = o[0] + corr, g = o[1] + corr, b = o[2] + corr;
            if constexpr (OUT_FMT == ovrfsr::FMT_RGBA8) {
                uint32_t v = 0;
                v = __builtin_amdgcn_cvt_pk_u8_f32(r, 0, v);
                v = __builtin_amdgcn_cvt_pk_u8_f32(g, 1, v);
                v = __builtin_amdgcn_cvt_pk_u8_f32(b, 2, v);
                v = __builtin_amdgcn_cvt_pk_u8_f32(o[3], 3, v);
                *OVRFSR_AT(uint32_t, out + (uint32_t)dstY * a.v.out_pitch + (uint32_t)dstX * 4u) = v;
            } else {
                const float s = 1.0f / 255.0f;
                store_unit<OUT_FMT>(out, a.v.out_pitch, dstX, dstY, sat01(r * s), sat01(g * s), sat01(b * s), sat01(o[3] * s));
            }
            continue;
        }
#endif
        // chroma: one bilinear tap at the output pixel centre, NIS_Scaler.h:747,758-761
        float4 op = bilinear_uv<IN_FMT>(in, a.v.in_pitch, inW, inH, (dstX + 0.5f) * a.kDstNormX, (dstY + 0.5f) * a.kDstNormY);
        const float corr = opY * (1.0f / 255.0f) - nis_getY(op.x, op.y, op.z);
        op.x += corr; op.y += corr; op.z += corr;
        // `unorm` UAV: clamp to [0,1] (also what the UNORM8 store does; explicit for the float formats)
        store_unit<OUT_FMT>(out, a.v.out_pitch, dstX, dstY, sat01(op.x), sat01(op.y), sat01(op.z), sat01(op.w));
    }
}

#if !OVRFSR_STRICT
// DirectCopy (NIS_Upscale.hlsl:77-90) for the 32x24 groups entirely outside the radius, launched from a host-built
// group list: no LDS (twice the occupancy of the scaler kernel), the 12 texel loads of a thread in flight before the
// first use.  Latency- / instruction-bound (2-3 TB/s); runs concurrently with the VALU-bound scaler kernel on the ctx's
// auxiliary stream.
template <int IN_FMT, int OUT_FMT>
__global__ __launch_bounds__(256) void nis_outside_kernel(const ovrfsr::NisArgs a)
{
    const uint32_t img_i = blockIdx.z;
    const uint32_t grp = OVRFSR_TILE_LIST(a)[blockIdx.x];
    uint32_t bx, by;
    tile_xy(grp, a.tilesX, a.tilesXMagic, bx, by);
    OVRFSR_IMAGES(IN_FMT, OUT_FMT);
    const int inW = a.v.inW, inH = a.v.inH, outW = a.v.outW, outH = a.v.outH;
    const int dstX = 32 * (int)bx + (int)(threadIdx.x & 31);
    const int dstY0 = 24 * (int)by + (int)(threadIdx.x >> 5);
    if (dstX >= outW) return;
    int x0; float fx;
    fixed8(mad_unfused((float)dstX / (float)outW, (float)inW, -0.5f), x0, fx);
    const int xa = clampi(x0, 0, inW - 1), xb = clampi(x0 + 1, 0, inW - 1);
    int y0[3]; float fy[3];
    float4 c00[3], c10[3], c01[3], c11[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        fixed8(mad_unfused((float)min(dstY0 + 8 * k, outH - 1) / (float)outH, (float)inH, -0.5f), y0[k], fy[k]);
        const int ya = clampi(y0[k], 0, inH - 1), yb = clampi(y0[k] + 1, 0, inH - 1);
        c00[k] = load_unit<IN_FMT>(in, a.v.in_pitch, xa, ya); c10[k] = load_unit<IN_FMT>(in, a.v.in_pitch, xb, ya);
        c01[k] = load_unit<IN_FMT>(in, a.v.in_pitch, xa, yb); c11[k] = load_unit<IN_FMT>(in, a.v.in_pitch, xb, yb);
    }
    __builtin_amdgcn_sched_barrier(0);
    const float dbg = a.reserved1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int dstY = dstY0 + 8 * k;
        const float w00 = (1.0f - fx) * (1.0f - fy[k]), w10 = fx * (1.0f - fy[k]), w01 = (1.0f - fx) * fy[k], w11 = fx * fy[k];
        const float r = bilerp_unfused(c00[k].x, c10[k].x, c01[k].x, c11[k].x, w00, w10, w01, w11);
        const float g = bilerp_unfused(c00[k].y, c10[k].y, c01[k].y, c11[k].y, w00, w10, w01, w11);
        const float b = bilerp_unfused(c00[k].z, c10[k].z, c01[k].z, c11[k].z, w00, w10, w01, w11);
        if (dstY < outH)
            store_unit<OUT_FMT>(out, a.v.out_pitch, dstX, dstY, sat01(r * (1 - dbg * 0)), sat01(g * (1 - dbg * 0.3f)), sat01(b * (1 - dbg * 0.3f)), 1.0f * (1 - dbg * 0));
    }
}
#endif

// ---- NVSharpen, NIS_Scaler.h:783-971 ----------------------------------------------------------------
__device__ __forceinline__ float nis_calc_lti_fast(const float y[5], const NisTune &t)
{
    const float a_min = fminf(fminf(y[0], y[1]), y[2]), a_max = fmaxf(fmaxf(y[0], y[1]), y[2]);
    const float b_min = fminf(fminf(y[2], y[3]), y[4]), b_max = fmaxf(fmaxf(y[2], y[3]), y[4]);
    const float a_cont = a_max - a_min, b_cont = b_max - b_min;
    const float cont_ratio = nis_div(fmaxf(a_cont, b_cont), (fminf(a_cont, b_cont) + t.kEps * (1.0f / 255.0f)));
    return (1.0f - sat01((cont_ratio - t.kMinContrastRatio) * t.kRatioNorm)) * t.kContrastBoost;
}
__device__ __forceinline__ float nis_eval_usm(const float pxl[5], float strength, float limit, const NisTune &t)
{
    float y_usm = -0.6001f * pxl[1] + 1.2002f * pxl[2] - 0.6001f * pxl[3];
    y_usm *= strength;
    y_usm = fminf(limit, fmaxf(-limit, y_usm));
    y_usm *= nis_calc_lti_fast(pxl, t);
    return y_usm;
}

// NVSharpen pass: 32x32 output group per workgroup, 36x36 luma tile (pitch 36), 4 pixels per thread.
template <int IN_FMT, int OUT_FMT>
__global__ __launch_bounds__(256) void nis_sharpen_kernel(const ovrfsr::NisArgs a)
{
    constexpr int BW = 32, BH = 32, LP = 36;
    OVRFSR_LDS_ARRAY(float, Yt, LP * LP, K_NIS_SHARPEN_Y);
    const uint32_t img_i = blockIdx.z;
    const uint32_t eye = (a.m.first_eye ^ (img_i & a.m.alternate)) & 1u;
    const uint32_t grp = xcd_tile_index(blockIdx.x, a.tilesX * a.tilesY);
    uint32_t bx, by;
    tile_xy(grp, a.tilesX, a.tilesXMagic, bx, by);
    OVRFSR_IMAGES(IN_FMT, OUT_FMT);
    const int W = a.v.outW, H = a.v.outH;
    const float dbg = a.reserved1;
    const uint32_t mode = a.m.mode[eye];
    const bool inside = mode == ovrfsr::MASK_ALL_INSIDE ? true
                      : mode == ovrfsr::MASK_ALL_OUTSIDE ? false : nis_group_inside(bx, by, BH, a.m.centre[eye], a.m.r2);
    const int dstBlockX = BW * (int)bx, dstBlockY = BH * (int)by;
    const int lx = threadIdx.x & 31;
    const int dstX = dstBlockX + lx;

    if (!inside) {
        // DirectCopy, NIS_Sharpen.hlsl:75-88: plain load, tint, alpha = 1
        for (int k = 0; k < 4; ++k) {
            const int dstY = dstBlockY + (int)(threadIdx.x >> 5) + 8 * k;
            if (dstX >= W || dstY >= H) continue;
            const float4 c = load_unit<IN_FMT>(in, a.v.in_pitch, dstX, dstY);
            store_unit<OUT_FMT>(out, a.v.out_pitch, dstX, dstY, sat01(c.x * (1 - dbg * 0)), sat01(c.y * (1 - dbg * 0.3f)),
                                sat01(c.z * (1 - dbg * 0.3f)), 1.0f * (1 - dbg * 0));
        }
        return;
    }
    for (int idx = threadIdx.x; idx < LP * LP; idx += ovrfsr::kThreads) {
        const int cy = idx / LP, cx = idx - cy * LP;
        const int sx = clampi(dstBlockX - 2 + cx, 0, W - 1), sy = clampi(dstBlockY - 2 + cy, 0, H - 1);
        const float4 c = load_unit<IN_FMT>(in, a.v.in_pitch, sx, sy);
        Yt[idx] = nis_getY(c.x, c.y, c.z);
    }
    __syncthreads();
    if (dstX >= W) return;
    NisTune t;
    t.kMinContrastRatio = a.kMinContrastRatio; t.kRatioNorm = a.kRatioNorm; t.kContrastBoost = a.kContrastBoost; t.kEps = a.kEps;
    t.kSharpStartY = a.kSharpStartY; t.kSharpScaleY = a.kSharpScaleY; t.kSharpStrengthMin = a.kSharpStrengthMin;
    t.kSharpStrengthScale = a.kSharpStrengthScale; t.kSharpLimitMin = a.kSharpLimitMin; t.kSharpLimitScale = a.kSharpLimitScale;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const int ly = (int)(threadIdx.x >> 5) + 8 * k;
        const int dstY = dstBlockY + ly;
        if (dstY >= H) break;
        float p[5][5];
#pragma unroll
        for (int i = 0; i < 5; ++i)
#pragma unroll
            for (int j = 0; j < 5; ++j) p[i][j] = Yt[(ly + i) * LP + lx + j];
        // GetDirUSM, NIS_Scaler.h:819-871
        const float scaleY = 1.0f - sat01((p[2][2] - t.kSharpStartY) * t.kSharpScaleY);
        const float strength = scaleY * t.kSharpStrengthScale + t.kSharpStrengthMin;
        const float limit = (scaleY * t.kSharpLimitScale + t.kSharpLimitMin) * p[2][2];
        const float d0[5] = {p[0][2], p[1][2], p[2][2], p[3][2], p[4][2]};
        const float d90[5] = {p[2][0], p[2][1], p[2][2], p[2][3], p[2][4]};
        const float d45[5] = {p[1][1], nis_lerp(p[2][1], p[1][2], 0.5f), p[2][2], nis_lerp(p[3][2], p[2][3], 0.5f), p[3][3]};
        const float d135[5] = {p[3][1], nis_lerp(p[3][2], p[2][1], 0.5f), p[2][2], nis_lerp(p[2][3], p[1][2], 0.5f), p[1][3]};
        const float q[9] = {p[1][1], p[1][2], p[1][3], p[2][1], p[2][2], p[2][3], p[3][1], p[3][2], p[3][3]};
        const float4 w = nis_edge_map(q, a.kDetectRatio, a.kDetectThres);
#if OVRFSR_STRICT
        const float r0 = nis_eval_usm(d0, strength, limit, t), r1 = nis_eval_usm(d90, strength, limit, t);
        const float r2 = nis_eval_usm(d45, strength, limit, t), r3 = nis_eval_usm(d135, strength, limit, t);
#else
        // Exact wave-uniform skips (as in NVScaler): a directional USM term whose edge weight is 0 in all 64 lanes
        // contributes r*0 = +-0 (r is finite: the LTI divisor is >= kEps/255 > 0), and x + 0 = x.  Smooth regions -- most
        // of a frame -- evaluate no EvalUSM at all, and where no lane of the wave has any edge the output texel is the
        // input texel: for an RGBA8 -> RGBA8 pass the dword is copied as is (decode + encode of the same byte).
        if (__builtin_amdgcn_ballot_w64((w.x != 0.0f) || (w.y != 0.0f) || (w.z != 0.0f) || (w.w != 0.0f)) == 0) {
            if constexpr (IN_FMT == ovrfsr::FMT_RGBA8 && OUT_FMT == ovrfsr::FMT_RGBA8) {
                *OVRFSR_AT(uint32_t, out + (uint32_t)dstY * a.v.out_pitch + (uint32_t)dstX * 4u) =
                    *OVRFSR_AT(const uint32_t, in + (uint32_t)dstY * a.v.in_pitch + (uint32_t)dstX * 4u);
            } else {
                const float4 c = load_unit<IN_FMT>(in, a.v.in_pitch, dstX, dstY);
                store_unit<OUT_FMT>(out, a.v.out_pitch, dstX, dstY, sat01(c.x), sat01(c.y), sat01(c.z), sat01(c.w));
            }
            continue;
        }
        float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f, r3 = 0.0f;
        if (__builtin_amdgcn_ballot_w64(w.x != 0.0f) != 0) r0 = nis_eval_usm(d0, strength, limit, t);
        if (__builtin_amdgcn_ballot_w64(w.y != 0.0f) != 0) r1 = nis_eval_usm(d90, strength, limit, t);
        if (__builtin_amdgcn_ballot_w64(w.z != 0.0f) != 0) r2 = nis_eval_usm(d45, strength, limit, t);
        if (__builtin_amdgcn_ballot_w64(w.w != 0.0f) != 0) r3 = nis_eval_usm(d135, strength, limit, t);
#endif
        const float usmY = (r0 * w.x + r1 * w.y + r2 * w.z + r3 * w.w);
        // bilinear tap at the pixel centre of a same-size image == the texel itself (NIS_Scaler.h:949)
        float4 op = load_unit<IN_FMT>(in, a.v.in_pitch, dstX, dstY);
        op.x += usmY; op.y += usmY; op.z += usmY;
        store_unit<OUT_FMT>(out, a.v.out_pitch, dstX, dstY, sat01(op.x), sat01(op.y), sat01(op.z), sat01(op.w));
    }
}
