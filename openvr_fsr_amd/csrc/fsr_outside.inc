// fsr_outside.inc -- product build only, included by fsr_kernels.inc inside `#if !OVRFSR_STRICT`: the kernels that resolve the tiles
// OUTSIDE the radius of a masked configuration -- the reference's `Bilinear` fallback (fsr/fsr_easu.hlsl:33-36), optionally followed by
// RCAS's tinted copy (fsr/fsr_rcas.hlsl:46-47) so that the tile is written in final form with no intermediate image:
//   bilinear_column4          4 pixels of one column per thread, texels from global memory (paired wide loads)
//   easu_outside_kernel       one 32x32 tile per workgroup from a host-built tile list, no LDS
//   outside_staged_kernel     persistent, software-pipelined, LDS-staged 4-pixels-per-thread form (RGBA8 sources, upscaling only)

// Bilinear fallback for the 4 pixels (ox, oy + 8k) of one thread: issue the 4 row-tap loads, then all 16 texel
// loads, before any arithmetic -- this path is latency-bound, not VALU-bound.
// MID_FMT < 0: this is the EASU pass (alpha = 1).  MID_FMT >= 0: the pixel is ALSO outside the radius for RCAS,
// whose fallback is a tinted copy of the intermediate texel with no neighbours (fsr_rcas.hlsl:46-47), so the final
// pixel = tint(value read back from a MID_FMT intermediate) is written directly: no intermediate image at all.
template <int IN_FMT, int OUT_FMT, int MID_FMT = -1>
__device__ __forceinline__ void bilinear_column4(OVRFSR_PTR_R(const uint8_t) in, OVRFSR_PTR_R(uint8_t) out, const ovrfsr::EasuArgs &a,
                                                 int ox, int oyb, int bxa, int bxb, float bfx)
{
    // row taps computed in registers (same IEEE operations as the host table): a table lookup here would put a
    // second dependent memory round trip in front of the 16 texel loads
    ovrfsr::BilinTap ty[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float v = div_exact((float)min(oyb + 8 * k, a.v.outH - 1), (float)a.v.outH, a.rcpOutH, a.rcpExact != 0u);
        fixed8(mad_unfused(v, (float)a.v.inH, -0.5f), ty[k].i0, ty[k].frac);
    }
    // one pixel: blend, intermediate rounding, tint, store
    auto finish = [&](int k, const float4 &c00, const float4 &c10, const float4 &c01, const float4 &c11) {
        const int oy = oyb + 8 * k;
        const float fy = ty[k].frac;
        const float w00 = (1.0f - bfx) * (1.0f - fy), w10 = bfx * (1.0f - fy), w01 = (1.0f - bfx) * fy, w11 = bfx * fy;
        // exact (unfused) blend where the result is rounded to UNORM8 somewhere downstream: that is where ties are
        // frequent and visible (see bilerp_unfused); half/float destinations take the contracted form
        constexpr bool kExact = OUT_FMT == ovrfsr::FMT_RGBA8 || MID_FMT == ovrfsr::FMT_RGBA8 || OUT_FMT == ovrfsr::FMT_RGB10A2;
        const float r = bilerp<kExact>(c00.x, c10.x, c01.x, c11.x, w00, w10, w01, w11);
        const float g = bilerp<kExact>(c00.y, c10.y, c01.y, c11.y, w00, w10, w01, w11);
        const float b = bilerp<kExact>(c00.z, c10.z, c01.z, c11.z, w00, w10, w01, w11);
        if constexpr (MID_FMT < 0) {
            if (oy < a.v.outH) store_unit<OUT_FMT>(out, a.v.out_pitch, ox, oy, r, g, b, 1.0f);
        } else {
            float mr, mg, mb;
            if constexpr (MID_FMT == ovrfsr::FMT_RGBA8) {
                mr = unorm8_to_unit((float)unit_to_unorm8(r)); mg = unorm8_to_unit((float)unit_to_unorm8(g)); mb = unorm8_to_unit((float)unit_to_unorm8(b));
            } else if constexpr (MID_FMT == ovrfsr::FMT_RGBA16F) {
                mr = (float)(half_t)r; mg = (float)(half_t)g; mb = (float)(half_t)b;
            } else {
                mr = r; mg = g; mb = b;
            }
            if (a.debug) { // wave-uniform
                const float mulG = 1.0f - 0.3f;
                if (oy < a.v.outH) store_unit<OUT_FMT>(out, a.v.out_pitch, ox, oy, mr, mg * mulG, mb * mulG, 1.0f);
            } else if constexpr (MID_FMT == ovrfsr::FMT_RGBA16F && OUT_FMT == ovrfsr::FMT_RGBA16F) {
                // no tint: half -> float -> half is the half itself; store the blend with ONE rounding (6 v_cvt per pixel less)
                if (oy < a.v.outH) store_unit<OUT_FMT>(out, a.v.out_pitch, ox, oy, r, g, b, 1.0f);
            } else {
                if (oy < a.v.outH) store_unit<OUT_FMT>(out, a.v.out_pitch, ox, oy, mr, mg, mb, 1.0f);
            }
        }
    };
    // 16 texel loads per thread: 32-bit offsets off the uniform image base (one add per texel; the 64-bit row*pitch + x*size
    // chains and two-instruction clamps were half of this kernel's VALU work)
    const uint32_t xoa = (uint32_t)bxa * (uint32_t)TexelBytes<IN_FMT>::v, xob = (uint32_t)bxb * (uint32_t)TexelBytes<IN_FMT>::v;
    // Where no lane of the wave sits on a clamped column (all but the left / right image border), the two taps of a row are
    // adjacent texels: ONE 8- or 16-byte load instead of two -- 8 vector-memory instructions per thread instead of 16 (this
    // kernel is bound by the vector-memory path, not by VALU issue: profiles/r02_final_sq/sq_C5.txt, valu_busy 0.5)
    // In both forms ALL loads are issued (addresses are clamped, always valid) before the first use of any of them, and the
    // loaded words stay RAW across that fence: with the decode written next to the load, the scheduler hoists the first
    // shifts / converts between the load instructions and an `s_waitcnt vmcnt(1)` lands after the second load (round 3: that is
    // 2-4 loads in flight instead of 8); without the fence it sinks each pixel's loads behind the previous pixel's bounds branch.
    constexpr bool kPairable = IN_FMT == ovrfsr::FMT_RGBA8 || IN_FMT == ovrfsr::FMT_RGBA16F || IN_FMT == ovrfsr::FMT_R11G11B10F;
    bool paired = false;
    if constexpr (kPairable) paired = __builtin_amdgcn_ballot_w64(bxb != bxa + 1) == 0;
    if (paired) {
        if constexpr (IN_FMT == ovrfsr::FMT_RGBA8) {
            typedef uint32_t u32x2_a4_t __attribute__((ext_vector_type(2), aligned(4)));
            u32x2_a4_t pa[4], pb[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t ra = (uint32_t)clamp0(ty[k].i0, a.v.inH - 1) * a.v.in_pitch, rb = (uint32_t)clamp0(ty[k].i0 + 1, a.v.inH - 1) * a.v.in_pitch;
                pa[k] = *OVRFSR_AT(const u32x2_a4_t, in + (ra + xoa)); pb[k] = *OVRFSR_AT(const u32x2_a4_t, in + (rb + xoa));
            }
            __builtin_amdgcn_sched_barrier(0);
            auto dec = [](uint32_t v) {
                return make_float4(unorm8_to_unit((float)(v & 0xffu)), unorm8_to_unit((float)((v >> 8) & 0xffu)),
                                   unorm8_to_unit((float)((v >> 16) & 0xffu)), unorm8_to_unit((float)(v >> 24)));
            };
#pragma unroll
            for (int k = 0; k < 4; ++k) finish(k, dec(pa[k].x), dec(pa[k].y), dec(pb[k].x), dec(pb[k].y));
        } else if constexpr (IN_FMT == ovrfsr::FMT_RGBA16F) {
            typedef half_t half8_a8_t __attribute__((ext_vector_type(8), aligned(8)));
            half8_a8_t pa[4], pb[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t ra = (uint32_t)clamp0(ty[k].i0, a.v.inH - 1) * a.v.in_pitch, rb = (uint32_t)clamp0(ty[k].i0 + 1, a.v.inH - 1) * a.v.in_pitch;
                pa[k] = *OVRFSR_AT(const half8_a8_t, in + (ra + xoa)); pb[k] = *OVRFSR_AT(const half8_a8_t, in + (rb + xoa));
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                finish(k, make_float4((float)pa[k][0], (float)pa[k][1], (float)pa[k][2], (float)pa[k][3]),
                       make_float4((float)pa[k][4], (float)pa[k][5], (float)pa[k][6], (float)pa[k][7]),
                       make_float4((float)pb[k][0], (float)pb[k][1], (float)pb[k][2], (float)pb[k][3]),
                       make_float4((float)pb[k][4], (float)pb[k][5], (float)pb[k][6], (float)pb[k][7]));
        } else if constexpr (IN_FMT == ovrfsr::FMT_R11G11B10F) {
            // packed float words: the two taps of a row are one 8-byte load, as RGBA8's; decoded behind the fence
            typedef uint32_t u32x2_a4_t __attribute__((ext_vector_type(2), aligned(4)));
            u32x2_a4_t pa[4], pb[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t ra = (uint32_t)clamp0(ty[k].i0, a.v.inH - 1) * a.v.in_pitch, rb = (uint32_t)clamp0(ty[k].i0 + 1, a.v.inH - 1) * a.v.in_pitch;
                pa[k] = *OVRFSR_AT(const u32x2_a4_t, in + (ra + xoa)); pb[k] = *OVRFSR_AT(const u32x2_a4_t, in + (rb + xoa));
            }
            __builtin_amdgcn_sched_barrier(0);
            auto dec = [](uint32_t v) { float4 c; unpack_r11g11b10f(v, c.x, c.y, c.z); c.w = 1.0f; return c; };
#pragma unroll
            for (int k = 0; k < 4; ++k) finish(k, dec(pa[k].x), dec(pa[k].y), dec(pb[k].x), dec(pb[k].y));
        }
    } else if constexpr (IN_FMT == ovrfsr::FMT_R11G11B10F) {
        // a lane on a clamped column: four word loads per row pair, the words kept raw across the fence like the paired form's
        uint32_t w00[4], w10[4], w01[4], w11[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t ra = (uint32_t)clamp0(ty[k].i0, a.v.inH - 1) * a.v.in_pitch, rb = (uint32_t)clamp0(ty[k].i0 + 1, a.v.inH - 1) * a.v.in_pitch;
            w00[k] = *OVRFSR_AT(const uint32_t, in + (ra + xoa)); w10[k] = *OVRFSR_AT(const uint32_t, in + (ra + xob));
            w01[k] = *OVRFSR_AT(const uint32_t, in + (rb + xoa)); w11[k] = *OVRFSR_AT(const uint32_t, in + (rb + xob));
        }
        __builtin_amdgcn_sched_barrier(0);
        auto dec = [](uint32_t v) { float4 c; unpack_r11g11b10f(v, c.x, c.y, c.z); c.w = 1.0f; return c; };
#pragma unroll
        for (int k = 0; k < 4; ++k) finish(k, dec(w00[k]), dec(w10[k]), dec(w01[k]), dec(w11[k]));
    } else {
        float4 c00[4], c10[4], c01[4], c11[4];
        // (RGBA32F texels behind a UNORM8 intermediate -- cfg.reference_formats --: two batches of 8 loads instead of one of 16; with all
        // 48 channel registers live next to the UNORM8 round trip the kernel would pass 64 VGPRs, tests/test_reference_formats.py)
        if constexpr (IN_FMT == ovrfsr::FMT_RGBA32F && MID_FMT == ovrfsr::FMT_RGBA8) {
#pragma unroll
            for (int k0 = 0; k0 < 4; k0 += 2) {
#pragma unroll
                for (int k = k0; k < k0 + 2; ++k) {
                    const uint32_t ra = (uint32_t)clamp0(ty[k].i0, a.v.inH - 1) * a.v.in_pitch, rb = (uint32_t)clamp0(ty[k].i0 + 1, a.v.inH - 1) * a.v.in_pitch;
                    c00[k] = load_unit_off<IN_FMT>(in, ra + xoa); c10[k] = load_unit_off<IN_FMT>(in, ra + xob);
                    c01[k] = load_unit_off<IN_FMT>(in, rb + xoa); c11[k] = load_unit_off<IN_FMT>(in, rb + xob);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = k0; k < k0 + 2; ++k) finish(k, c00[k], c10[k], c01[k], c11[k]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t ra = (uint32_t)clamp0(ty[k].i0, a.v.inH - 1) * a.v.in_pitch, rb = (uint32_t)clamp0(ty[k].i0 + 1, a.v.inH - 1) * a.v.in_pitch;
                c00[k] = load_unit_off<IN_FMT>(in, ra + xoa); c10[k] = load_unit_off<IN_FMT>(in, ra + xob);
                c01[k] = load_unit_off<IN_FMT>(in, rb + xoa); c11[k] = load_unit_off<IN_FMT>(in, rb + xob);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < 4; ++k) finish(k, c00[k], c10[k], c01[k], c11[k]);
        }
    }
}

// Tiles whose four mask groups are all outside the radius, launched from a host-built tile list: no LDS, so
// 8 workgroups per CU instead of 4 for this latency-bound path.
template <int IN_FMT, int OUT_FMT, int MID_FMT = -1>
__global__ __launch_bounds__(256) void easu_outside_kernel(const ovrfsr::EasuArgs a)
{
    const uint32_t img_i = blockIdx.z;
    const uint32_t tile = OVRFSR_TILE_LIST(a)[blockIdx.x];
    uint32_t tileX, tileY;
    tile_xy(tile, a.tilesX, a.tilesXMagic, tileX, tileY);
    OVRFSR_IMAGES(IN_FMT, OUT_FMT);
    const int ox = (int)tileX * ovrfsr::kTileW + (int)(threadIdx.x & 31);
    if (ox >= a.v.outW) return;
    ovrfsr::BilinTap tx;
    fixed8(mad_unfused(div_exact((float)ox, (float)a.v.outW, a.rcpOutW, a.rcpExact != 0u), (float)a.v.inW, -0.5f), tx.i0, tx.frac);
    const int bxa = clampi(tx.i0, 0, a.v.inW - 1), bxb = clampi(tx.i0 + 1, 0, a.v.inW - 1);
    bilinear_column4<IN_FMT, OUT_FMT, MID_FMT>(in, out, a, ox, (int)tileY * ovrfsr::kTileH + (int)(threadIdx.x >> 5), bxa, bxb, tx.frac);
}

// Tiles outside the radius, upscaling only (in <= out in both axes); written for RGBA8 / RGBA16F sources, dispatched
// for RGBA8 ones (see launch_outside_staged).  One 32 x TH tile per
// workgroup of 8*TH threads.  The per-pixel form above issues 4 texel loads and one store per pixel, decodes 12 channels
// and spends an IEEE division per pixel coordinate: at 4-8 B per lane that is instruction-bound (1.8 TB/s on RGBA8).  Here
//   * column and row taps (the only IEEE divisions and sub-texel snaps) come from the host-built tables (BilinTap),
//   * the tile's texel footprint is decoded once into an LDS float4 plane (RGBA8: b/255 correctly rounded); cell (cx,cy)
//     holds texel clamp(X0+cx), clamp(Y0+cy): clamp addressing is resolved at staging time, so tap b is always cell a+1,
//   * every thread blends 4 horizontally adjacent pixels and writes them with 16-byte stores.
// MID_FMT as in bilinear_column4: < 0 = the EASU pass alone (alpha 1); >= 0 = the FINAL pixel, tint(value read back from a
// MID_FMT intermediate); RGBA32F there means "tint the un-rounded value", which is also NIS DirectCopy (TH = 24).
// Wherever a UNORM8 rounding follows, the blend is the same expression, in the same order, on the same unit-domain values
// as bilinear_uv, unfused: 8-bit weights on byte texels land on exact rounding ties very often (5 % of all bytes at scale
// 3/4), and only the as-written evaluation breaks those ties the way the reference does (an exact byte-domain sum, or a
// contracted one, does not).
// LDS layout (round 3): planar and row-interleaved, TEX[row][channel][kOutsidePitch = 40] floats.  A pixel's taps (x, x+1)
// of one channel are adjacent dwords -> one ds_read2_b32 (4 LDS cycles) per channel and row, all six off ONE base VGPR
// with immediate offsets (channel stride 40, row stride 120 dwords: both < 256); consecutive lanes sit 4 pixels = 3 texels
// apart, and with a row stride of 120 = 24 (mod 32) the 8 quads x 4 rows of a 32-lane group fall on 32 distinct banks:
// conflict-free.  Rounds 1-2 kept float4 cells and read them with ds_read_b96 (8 LDS cycles each, lane stride 12 dwords:
// 4-way conflicts, 45 % of the LDS cycles).
// Persistent, software-pipelined (round 3): a tile's work is a chain of dependent memory round trips (tile record ->
// texels and tap tables -> LDS -> pixels) in front of ~230 VALU instructions per thread, and at 8 workgroups per CU the
// one-tile-per-workgroup form left the VALU 45 % idle (4.7 us per workgroup, 2.5 of them issue).  Here a workgroup walks
// tiles blockIdx.x, + gridDim.x, ... of the list; while it blends tile k from LDS, the texels and taps of tile k+1 and the
// record of tile k+2 are already in flight into registers.  The host-built 16-byte record of a list entry (tile origin,
// footprint origin and extent) replaces the tile-index -> tap-table scalar load chain.
struct OutsideRaw { uint32_t t[6]; };           // the texels this thread stages: 5 rows of its column + one of the columns >= 32
struct OutsideTaps { int xs[4]; float fs[4]; int ya; float fy; };

template <int TH, int IN_FMT, int OUT_FMT, int MID_FMT>
__global__ __launch_bounds__(8 * TH) void outside_staged_kernel(const ovrfsr::OutsideArgs a)
{
    static_assert(IN_FMT == ovrfsr::FMT_RGBA8, "staged outside kernel: RGBA8 sources (raw texels wait in registers, one dword each)");
    constexpr int TB = 8 * TH, RSTEP = TB / 32;
    constexpr int P = ovrfsr::kOutsidePitch, RS = 3 * P; // dwords per channel row / per texel row
    static_assert(5 * RSTEP >= TH + 2, "five sweeps cover the footprint rows (in <= out: at most TH + 2)");
    // plane sized by the host to the largest tile footprint of this scale (a.lds_rows x a.lds_cols <= 34 x 36): at scale 3/4
    // 26 rows x 480 B = 12.5 KB
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    OVRFSR_LDS_POISON(smem, a.ldsBytes);
    OVRFSR_PTR(float) TEX = OVRFSR_CARVE(float, reinterpret_cast<float *>(smem), a.lds_rows * RS, 0, K_OUTSIDE_TEX, smem, a.ldsBytes);
    const uint32_t img_i = blockIdx.z;
    OVRFSR_IMAGES(IN_FMT, OUT_FMT);
    const int inW = a.v.inW, inH = a.v.inH, outW = a.v.outW, outH = a.v.outH;
    const int tid = threadIdx.x;
    const int sc = tid & 31, sr = tid >> 5;  // staging: column sc, rows sr + i * RSTEP; columns >= 32: cell (32 + (tid & 3), tid >> 2)
    const int q = tid & 7, row = tid >> 3;   // pixels: (ox0 + 4q .. +3, oy0 + row)
    const uint32_t nT = a.nTiles, G = gridDim.x;
    // a record is 4 dwords, 3 of them used: load exactly those (a dwordx4 load whose 4th, dead destination register the
    // allocator reuses makes the next instruction wait for the load it follows)
    typedef uint32_t u32x4_t __attribute__((ext_vector_type(3), aligned(4)));
    auto load_rec = [&](uint32_t i) { return *OVRFSR_AT_N(const u32x4_t, 12, OVRFSR_TILE_REC(a) + 4u * (size_t)i); };

    struct Rec { int ox0, oy0, X0, Y0, colsN, rowsN; };
    auto unpack = [](u32x4_t r) { // the record is the same for every lane: keep it in SGPRs
        const uint32_t r0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)r.x), r1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)r.y),
                       r2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)r.z);
        Rec o;
        o.ox0 = (int)(r0 & 0xffffu); o.oy0 = (int)(r0 >> 16);
        o.X0 = (int)(r1 & 0xffffu) - 1; o.Y0 = (int)(r1 >> 16) - 1;
        o.colsN = (int)(r2 & 0xffu); o.rowsN = (int)(r2 >> 8);
        return o;
    };
    // issue (do not wait for) the texel loads of a tile: cell (c, r) = texel clamp(X0+c), clamp(Y0+r)
    auto issue_texels = [&](const Rec &t) {
        OutsideRaw w;
        const uint32_t cx = (uint32_t)clampi(t.X0 + sc, 0, inW - 1) * 4u;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int r = sr + i * RSTEP;
            w.t[i] = 0;
            if (sc < t.colsN && r < t.rowsN) w.t[i] = *OVRFSR_AT(const uint32_t, in + ((uint32_t)clampi(t.Y0 + r, 0, inH - 1) * a.v.in_pitch + cx));
        }
        w.t[5] = 0;
        if (t.colsN > 32 && (tid >> 2) < t.rowsN && 32 + (tid & 3) < t.colsN)
            w.t[5] = *OVRFSR_AT(const uint32_t, in + ((uint32_t)clampi(t.Y0 + (tid >> 2), 0, inH - 1) * a.v.in_pitch + (uint32_t)clampi(t.X0 + 32 + (tid & 3), 0, inW - 1) * 4u));
        return w;
    };
    auto issue_taps = [&](const Rec &t) {
        typedef int i32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));
        OVRFSR_PTR(const ovrfsr::BilinTap) bx = OVRFSR_BIL_X(a) + (t.ox0 + 4 * q);
        const i32x4_a8 t01 = *OVRFSR_AT(const i32x4_a8, bx), t23 = *OVRFSR_AT(const i32x4_a8, bx + 2);
        const ovrfsr::BilinTap ty = OVRFSR_BIL_Y(a)[min(t.oy0 + row, outH - 1)];
        OutsideTaps o;
        o.xs[0] = t01.x; o.xs[1] = t01.z; o.xs[2] = t23.x; o.xs[3] = t23.z;
        o.fs[0] = __int_as_float(t01.y); o.fs[1] = __int_as_float(t01.w); o.fs[2] = __int_as_float(t23.y); o.fs[3] = __int_as_float(t23.w);
        o.ya = ty.i0; o.fy = ty.frac;
        return o;
    };
    // decode (b/255 correctly rounded) and write this thread's cells
    auto put = [&](OVRFSR_PTR(float) d, uint32_t v) {
        d[0] = unorm8_to_unit((float)(v & 0xffu)); d[P] = unorm8_to_unit((float)((v >> 8) & 0xffu)); d[2 * P] = unorm8_to_unit((float)((v >> 16) & 0xffu));
    };
    auto stage = [&](const Rec &t, const OutsideRaw &w) {
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int r = sr + i * RSTEP;
            if (sc < t.colsN && r < t.rowsN) put(TEX + r * RS + sc, w.t[i]);
        }
        if (t.colsN > 32 && (tid >> 2) < t.rowsN && 32 + (tid & 3) < t.colsN) put(TEX + (tid >> 2) * RS + 32 + (tid & 3), w.t[5]);
    };
    // UNORM8 encode of a value known to lie in [0,1]: the blend is a convex combination of values in [0,1] whose every
    // partial result is monotone under rounding (products <= their weight, sums of weights exact), so saturate is a no-op
    auto q8 = [](float x) { return (uint32_t)mad_unfused(x, 255.0f, 0.5f); };
    // The debug tint (and, with it, the decode/encode round trip through a UNORM8 intermediate) is wave-uniform: two copies
    // of the pixel block, the common one (debug off) with neither.
    auto blend = [&](const Rec &t, const OutsideTaps &tp4, auto debugTag) {
        constexpr bool kDebug = decltype(debugTag)::value;
        const int ox = t.ox0 + 4 * q, oy = t.oy0 + row;
        if (ox >= outW || oy >= outH) return;
        const float mulG = 1.0f - 0.3f; // 1 - debug*0.3 with debug = 1 (fsr_rcas.hlsl:46, NIS_Upscale.hlsl:88)
        const float fy = tp4.fy, gy = 1.0f - fy;
        const OVRFSR_PTR(float) rowp = TEX + (tp4.ya - t.Y0) * RS - t.X0;
        OVRFSR_PTR(uint8_t) op = out + (size_t)oy * a.v.out_pitch + (size_t)ox * TexelBytes<OUT_FMT>::v; // up to 4 GiB per image (RGBA32F)
        float pr[4], pg[4], pb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const OVRFSR_PTR(float) tp = rowp + tp4.xs[j];
            const float fx = tp4.fs[j], gx = 1.0f - fx;
            const f2_t w0 = mk2(gx * gy, fx * gy), w1 = mk2(gx * fy, fx * fy);
            // the sampler restatement's blend, every product and sum rounded separately (see bilerp_unfused), two products
            // per v_pk_mul_f32
            float r = bilerp_pk_unfused(mk2(tp[0], tp[1]), mk2(tp[RS], tp[RS + 1]), w0, w1);
            float g = bilerp_pk_unfused(mk2(tp[P], tp[P + 1]), mk2(tp[RS + P], tp[RS + P + 1]), w0, w1);
            float b = bilerp_pk_unfused(mk2(tp[2 * P], tp[2 * P + 1]), mk2(tp[RS + 2 * P], tp[RS + 2 * P + 1]), w0, w1);
            if constexpr (MID_FMT == ovrfsr::FMT_RGBA8) {
                // UNORM8 intermediate, then the tinted copy of fsr_rcas.hlsl:46-47.  Into a UNORM8 destination without
                // the tint that is decode + encode of the same byte, i.e. the byte: skipped
                if constexpr (kDebug || OUT_FMT != ovrfsr::FMT_RGBA8) {
                    r = unorm8_to_unit((float)q8(r)); g = unorm8_to_unit((float)q8(g)); b = unorm8_to_unit((float)q8(b));
                }
            } else if constexpr (MID_FMT == ovrfsr::FMT_RGBA16F) {
                r = (float)(half_t)r; g = (float)(half_t)g; b = (float)(half_t)b;
            }
            if constexpr (MID_FMT >= 0 && kDebug) { g *= mulG; b *= mulG; }
            pr[j] = r; pg[j] = g; pb[j] = b;
        }
        if (ox + 3 < outW) {
            typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
            if constexpr (OUT_FMT == ovrfsr::FMT_RGBA8) {
                u32x4_a4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = q8(pr[j]) | (q8(pg[j]) << 8) | (q8(pb[j]) << 16) | 0xff000000u;
                *OVRFSR_AT(u32x4_a4, op) = o;
            } else if constexpr (OUT_FMT == ovrfsr::FMT_RGBA16F) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const half4_t p0 = {(half_t)pr[2 * h], (half_t)pg[2 * h], (half_t)pb[2 * h], (half_t)1.0f};
                    const half4_t p1 = {(half_t)pr[2 * h + 1], (half_t)pg[2 * h + 1], (half_t)pb[2 * h + 1], (half_t)1.0f};
                    u32x4_a4 o;
                    __builtin_memcpy(&o, &p0, 8);
                    __builtin_memcpy(reinterpret_cast<char *>(&o) + 8, &p1, 8);
                    *OVRFSR_AT(u32x4_a4, op + 16 * h) = o;
                }
            } else {
                typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4_a4 o = {pr[j], pg[j], pb[j], 1.0f};
                    *OVRFSR_AT(f32x4_a4, op + 16 * j) = o;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (ox + j < outW) store_unit<OUT_FMT>(out, a.v.out_pitch, ox + j, oy, pr[j], pg[j], pb[j], 1.0f);
        }
    };

    // Pipeline state at the loop head: tile k = (cur, raw, taps: loads in flight), the unpacked record of tile k+1 (nxt, in
    // SGPRs) and the pending record load of tile k+2 (recP).  Records are fetched two tiles ahead and unpacked one tile ahead,
    // right behind the wait the staging writes need anyway -- the loop never waits for a load it has just issued.
    uint32_t idx = blockIdx.x;
    if (idx >= nT) return; // workgroup-uniform
    const u32x4_t rec0 = load_rec(idx), rec1 = load_rec(min(idx + G, nT - 1));
    u32x4_t recP = load_rec(min(idx + 2u * G, nT - 1));
    Rec cur = unpack(rec0), nxt = unpack(rec1);
    OutsideRaw raw = issue_texels(cur);
    OutsideTaps taps = issue_taps(cur);
#pragma unroll 1
    for (;;) {
        stage(cur, raw); // waits for this tile's texels and, in order, for everything issued before them (taps, recP)
        __syncthreads();
        const Rec nn = unpack(recP);
        const bool more = idx + G < nT; // workgroup-uniform
        OutsideRaw rawN = raw;
        OutsideTaps tapsN = taps;
        if (more) {
            recP = load_rec(min(idx + 3u * G, nT - 1));
            rawN = issue_texels(nxt);
            tapsN = issue_taps(nxt);
        }
        if (a.debug) blend(cur, taps, std::true_type{});
        else blend(cur, taps, std::false_type{});
        if (!more) break;
        __syncthreads(); // every wave is done reading the plane
        cur = nxt; nxt = nn; raw = rawN; taps = tapsN; idx += G;
    }
}

