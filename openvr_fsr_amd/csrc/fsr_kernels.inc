// fsr_kernels.inc -- FSR1 EASU and RCAS for gfx950 (CDNA4, wave64), written from scratch.
//
// Included twice by fsr_kernels.hip (after fsr_device.inc):
//   namespace ovrfsr_fast   : OVRFSR_STRICT 0, `#pragma clang fp contract(fast)` -> the product kernels
//   namespace ovrfsr_strict : OVRFSR_STRICT 1, `#pragma clang fp contract(off)`  -> validation build that
//                             evaluates every operator as the HLSL text writes it (bit-identical to the
//                             CPU oracle).
//
// What the kernels compute is fixed by the reference (file:line under /root/reference/src):
//   EASU   fsr/ffx_fsr1.h:239-437 (FsrEasuTapF/SetF/F), entry + radius mask fsr/fsr_easu.hlsl:27-64
//   RCAS   fsr/ffx_fsr1.h:684-769 (FsrRcasF), entry + mask fsr/fsr_rcas.hlsl:23-55
//   approximations fsr/ffx_a.h:1843-1845 (same magic numbers: results depend on them)
// How they compute it is MI355X-first and shares nothing with the HLSL structure:
//   * one 256-thread workgroup per 32x32 output tile; the input footprint (+1/+2 apron) is staged
//     ONCE into LDS, unpacked from RGBA8 once per texel (the D3D texture unit did this per tap);
//   * FsrEasuSetF's direction/length terms depend only on a texel and its 4 neighbours, not on the
//     output position, so they are computed once per input texel in a second LDS pass
//     ("analysis" plane: dirX, dirY, lenX^2, lenY^2) instead of 4x per output pixel;
//   * taps are LDS reads, clamp addressing is folded into the staging pass, stores are
//     row-contiguous (a wave writes 2 rows x 128 B);
//   * the radius mask is evaluated per 16x16 group exactly as the reference does, but a workgroup
//     whose four groups are all outside never touches LDS and resolves bilinear from L2/L1.
// Kernels in this file:
//   easu_kernel / rcas_kernel        reference-order arithmetic, runtime LDS pitch.  These ARE the strict build;
//                                    in the product build easu_kernel only serves footprints wider than 40 cells.
//   easu_fast_kernel                 product build, re-associated for the measured gfx950 VALU classes; 16-byte-load staging
//                                    sweeps, per-row table, lane permutation for conflict-free LDS reads, unmasked specialisation.
//   rcas_dpp_kernel                  product build, RGBA8 sources: side taps from neighbour lanes (DPP); 62 x 32 cells of an unmasked
//                                    frame, or 62-column segments of the runs of tiles touching the radius (mask-sorted form).
//   rcas_direct_kernel               product build, other formats / per-tile masks: every lane loads its own taps.
//   fused_kernel                     EASU -> RCAS in one launch (both builds).
//   easu_outside_kernel / outside_staged_kernel   product build, radius-masked configurations: tiles entirely outside the
//                                    radius from a host-built list, bilinear fallback (+ intermediate rounding + tint =
//                                    the final pixel), per-pixel form (paired wide loads) and LDS-staged 4-pixel form.

// ------------------------------------------------------------------------------------------------
// EASU
// ------------------------------------------------------------------------------------------------
// LDS colour plane: "narrow" = 4 halves per cell (exact for RGBA8 bytes kept as 0..255 and for
// RGBA16F texels), "wide" = float4 unit domain (RGBA32F input, and the strict build).
template <bool WIDE> struct ColorCell;
template <> struct ColorCell<false> { typedef half4_t type; };
template <> struct ColorCell<true> { typedef float4 type; };

template <int IN_FMT> struct EasuTraits {
    static constexpr bool wide = (OVRFSR_STRICT != 0) || (IN_FMT == ovrfsr::FMT_RGBA32F) || (IN_FMT == ovrfsr::FMT_RGB10A2); // k/1023 needs fp32
    static constexpr bool byte_domain = !wide && (IN_FMT == ovrfsr::FMT_RGBA8);
    typedef typename ColorCell<wide>::type cell_t;
};

// BYTES: the cell holds the bytes of an RGBA8 texel as 0..255 (product-build colour plane); the reference's value is b/255,
// correctly rounded (D3D UNORM8 decode)
template <bool BYTES> __device__ __forceinline__ void cell_rgb(const half4_t &c, float &r, float &g, float &b)
{
    r = (float)c.x; g = (float)c.y; b = (float)c.z;
    if constexpr (BYTES) { r = unorm8_to_unit(r); g = unorm8_to_unit(g); b = unorm8_to_unit(b); }
}
template <bool BYTES> __device__ __forceinline__ void cell_rgb(const float4 &c, float &r, float &g, float &b)
{
    if constexpr (BYTES) { r = unorm8_to_unit(c.x); g = unorm8_to_unit(c.y); b = unorm8_to_unit(c.z); }
    else { r = c.x; g = c.y; b = c.z; }
}

// one EASU tap: fsr/ffx_fsr1.h:239-272
__device__ __forceinline__ void easu_tap(float &aR, float &aG, float &aB, float &aW, float offx, float offy, float dirx,
                                         float diry, float lenx, float leny, float lob, float clp, float cr, float cg, float cb)
{
#pragma clang fp contract(off) // every operator rounded as written, in every build (see easu_resolve)
    float vx = (offx * (dirx)) + (offy * diry);
    float vy = (offx * (-diry)) + (offy * dirx);
    vx *= lenx;
    vy *= leny;
    float d2 = vx * vx + vy * vy;
    d2 = fminf(d2, clp);
    float wB = (float)(2.0 / 5.0) * d2 + -1.0f;
    float wA = lob * d2 + -1.0f;
    wB *= wB;
    wA *= wA;
    wB = (float)(25.0 / 16.0) * wB + (float)(-(25.0 / 16.0 - 1.0));
    float w = wB * wA;
    aR += cr * w;
    aG += cg * w;
    aB += cb * w;
    aW += w;
}

// FsrEasuF (fsr/ffx_fsr1.h:315-437) for one output pixel whose 'f' texel is LDS cell `base`
// (pitch = cells per row) and whose sub-texel position is (ppx,ppy), in the reference's operator order with
// every operator rounded separately and an IEEE division -- in EVERY build (the pragma travels with the
// inlined body): the strict build is this function on every pixel; the product build calls it for the
// pixels whose re-associated result lies too close to a rounding boundary of the store format to be
// trusted (near-tie guard, see easu_fast_kernel).  Result in the unit domain.
template <bool BYTES, typename CELL>
__device__ __forceinline__ void easu_resolve(OVRFSR_PTR_RC(CELL) col, OVRFSR_PTR_RC(float4) ana, int base, int pitch,
                                             float ppx, float ppy, float &outR, float &outG, float &outB)
{
#pragma clang fp contract(off)
    // direction/length: bilinear blend of the per-texel analysis of f,g,j,k in the reference's
    // accumulation order (s,t,u,v; x-term then y-term) -- ffx_fsr1.h:383-386 with :295-313 hoisted.
    const float4 aF = ana[base], aG4 = ana[base + 1], aJ = ana[base + pitch], aK = ana[base + pitch + 1];
    float ws = (1.0f - ppx) * (1.0f - ppy), wt = ppx * (1.0f - ppy), wu = (1.0f - ppx) * ppy, wv = ppx * ppy;
    float dirx = 0.0f, diry = 0.0f, len = 0.0f;
    dirx += aF.x * ws;  len += aF.z * ws;  diry += aF.y * ws;  len += aF.w * ws;
    dirx += aG4.x * wt; len += aG4.z * wt; diry += aG4.y * wt; len += aG4.w * wt;
    dirx += aJ.x * wu;  len += aJ.z * wu;  diry += aJ.y * wu;  len += aJ.w * wu;
    dirx += aK.x * wv;  len += aK.z * wv;  diry += aK.y * wv;  len += aK.w * wv;

    float dir2x = dirx * dirx, dir2y = diry * diry;
    float dirR = dir2x + dir2y;
    bool zro = dirR < (float)(1.0 / 32768.0);
    dirR = prx_lo_rsq(dirR);
    dirR = zro ? 1.0f : dirR;
    dirx = zro ? 1.0f : dirx;
    dirx *= dirR;
    diry *= dirR;
    len = len * 0.5f;
    len *= len;
    float stretch = (dirx * dirx + diry * diry) * prx_lo_rcp(fmaxf(fabsf(dirx), fabsf(diry)));
    float len2x = 1.0f + (stretch - 1.0f) * len;
    float len2y = 1.0f + -0.5f * len;
    float lob = 0.5f + (float)((1.0 / 4.0 - 0.04) - 0.5) * len;
    float clp = prx_lo_rcp(lob);

    //    b c
    //  e f g h
    //  i j k l
    //    n o
    float fr, fg, fb, gr, gg, gb, jr, jg, jb, kr, kg, kb, tr, tg, tb;
    cell_rgb<BYTES>(col[base], fr, fg, fb);
    cell_rgb<BYTES>(col[base + 1], gr, gg, gb);
    cell_rgb<BYTES>(col[base + pitch], jr, jg, jb);
    cell_rgb<BYTES>(col[base + pitch + 1], kr, kg, kb);
    float mnR = fminf(fminf(fr, fminf(gr, jr)), kr), mxR = fmaxf(fmaxf(fr, fmaxf(gr, jr)), kr);
    float mnG = fminf(fminf(fg, fminf(gg, jg)), kg), mxG = fmaxf(fmaxf(fg, fmaxf(gg, jg)), kg);
    float mnB = fminf(fminf(fb, fminf(gb, jb)), kb), mxB = fmaxf(fmaxf(fb, fmaxf(gb, jb)), kb);

    float aR = 0.0f, aGc = 0.0f, aB = 0.0f, aW = 0.0f;
#define OVRFSR_TAP(dx, dy, R, G, B) easu_tap(aR, aGc, aB, aW, (float)(dx) - ppx, (float)(dy) - ppy, dirx, diry, len2x, len2y, lob, clp, R, G, B)
#define OVRFSR_TAP_LDS(dx, dy) do { cell_rgb<BYTES>(col[base + (dy) * pitch + (dx)], tr, tg, tb); OVRFSR_TAP(dx, dy, tr, tg, tb); } while (0)
    OVRFSR_TAP_LDS(0, -1);            // b
    OVRFSR_TAP_LDS(1, -1);            // c
    OVRFSR_TAP_LDS(-1, 1);            // i
    OVRFSR_TAP(0, 1, jr, jg, jb);     // j
    OVRFSR_TAP(0, 0, fr, fg, fb);     // f
    OVRFSR_TAP_LDS(-1, 0);            // e
    OVRFSR_TAP(1, 1, kr, kg, kb);     // k
    OVRFSR_TAP_LDS(2, 1);             // l
    OVRFSR_TAP_LDS(2, 0);             // h
    OVRFSR_TAP(1, 0, gr, gg, gb);     // g
    OVRFSR_TAP_LDS(1, 2);             // o
    OVRFSR_TAP_LDS(0, 2);             // n
#undef OVRFSR_TAP_LDS
#undef OVRFSR_TAP
    float rW = 1.0f / aW; // IEEE, correctly rounded (== the oracle's ARcpF1)
    outR = fminf(mxR, fmaxf(mnR, aR * rW));
    outG = fminf(mxG, fmaxf(mnG, aGc * rW));
    outB = fminf(mxB, fmaxf(mnB, aB * rW));
}

// FsrEasuSetF's per-texel part (ffx_fsr1.h:295-313): direction and squared "length" of the luma gradient at a texel C from
// its 4-neighbours (A above, B left, D right, E below).  One expression for every place that evaluates it -- the two staging
// passes and the near-tie fixup kernel -- so that their planes are rounding-identical.
__device__ __forceinline__ float4 easu_analyse(float lA, float lB, float lC, float lD, float lE)
{
    const float dc = lD - lC, cb = lC - lB;
    float lenX = prx_lo_rcp(fmaxf(fabsf(dc), fabsf(cb)));
    const float dirX = lD - lB;
    lenX = sat01(fabsf(dirX) * lenX);
    const float ec = lE - lC, ca = lC - lA;
    float lenY = prx_lo_rcp(fmaxf(fabsf(ec), fabsf(ca)));
    const float dirY = lE - lA;
    lenY = sat01(fabsf(dirY) * lenY);
    return make_float4(dirX, dirY, lenX * lenX, lenY * lenY);
}

// The same function, evaluated by FOUR consecutive lanes per pixel (the near-tie pass of the product kernels lists a dozen
// pixels per tile: one lane each would leave 50 of a wave's 64 lanes idle through ~500 instructions).  Lane q of the quad
// computes the weights of taps 3q .. 3q+2 of the reference's accumulation order (b c i j f e k l h g o n); the twelve
// weights are then broadcast across the quad (DPP quad_perm) and lane c accumulates channel c -- R, G, B, and the weight
// sum in lane 3 -- over all twelve taps IN THAT ORDER, each product and sum rounded separately: every lane performs exactly
// the operations easu_resolve performs for its channel, so the result is the same, bit for bit.  Returns this lane's
// channel (unit domain; lanes 0..2).  Must be called by whole quads.
template <int LANE> __device__ __forceinline__ float quad_bcast(float v) // value of lane LANE of this lane's quad
{
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), LANE * 0x55, 0xf, 0xf, true));
}
__device__ __forceinline__ float quad_bcast(float v, int lane)
{
    return lane == 0 ? quad_bcast<0>(v) : lane == 1 ? quad_bcast<1>(v) : lane == 2 ? quad_bcast<2>(v) : quad_bcast<3>(v);
}
template <bool BYTES, typename COLT = float4>
__device__ __forceinline__ float easu_resolve_quad(OVRFSR_PTR_RC(COLT) col, OVRFSR_PTR_RC(float4) ana, int base, int pitch,
                                                   float ppx, float ppy, int q)
{
#pragma clang fp contract(off)
    // direction / length: as easu_resolve (replicated in the four lanes)
    const float4 aF = ana[base], aG4 = ana[base + 1], aJ = ana[base + pitch], aK = ana[base + pitch + 1];
    float ws = (1.0f - ppx) * (1.0f - ppy), wt = ppx * (1.0f - ppy), wu = (1.0f - ppx) * ppy, wv = ppx * ppy;
    float dirx = 0.0f, diry = 0.0f, len = 0.0f;
    dirx += aF.x * ws;  len += aF.z * ws;  diry += aF.y * ws;  len += aF.w * ws;
    dirx += aG4.x * wt; len += aG4.z * wt; diry += aG4.y * wt; len += aG4.w * wt;
    dirx += aJ.x * wu;  len += aJ.z * wu;  diry += aJ.y * wu;  len += aJ.w * wu;
    dirx += aK.x * wv;  len += aK.z * wv;  diry += aK.y * wv;  len += aK.w * wv;
    float dir2x = dirx * dirx, dir2y = diry * diry;
    float dirR = dir2x + dir2y;
    bool zro = dirR < (float)(1.0 / 32768.0);
    dirR = prx_lo_rsq(dirR);
    dirR = zro ? 1.0f : dirR;
    dirx = zro ? 1.0f : dirx;
    dirx *= dirR;
    diry *= dirR;
    len = len * 0.5f;
    len *= len;
    float stretch = (dirx * dirx + diry * diry) * prx_lo_rcp(fmaxf(fabsf(dirx), fabsf(diry)));
    float len2x = 1.0f + (stretch - 1.0f) * len;
    float len2y = 1.0f + -0.5f * len;
    float lob = 0.5f + (float)((1.0 / 4.0 - 0.04) - 0.5) * len;
    float clp = prx_lo_rcp(lob);

    // taps in accumulation order, 4 bits each: (dx + 1) | (dy + 1) << 2     b    c    i    j    f    e    k    l    h    g    o    n
    constexpr int kDx[12] = {0, 1, -1, 0, 0, -1, 1, 2, 2, 1, 1, 0}, kDy[12] = {-1, -1, 1, 1, 0, 0, 1, 1, 0, 0, 2, 2};
    uint64_t code = 0;
#pragma unroll
    for (int i = 0; i < 12; ++i) code |= (uint64_t)((kDx[i] + 1) | ((kDy[i] + 1) << 2)) << (4 * i);
    float w[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const uint32_t c4 = (uint32_t)(code >> (4 * (3 * q + s))) & 15u;
        const float offx = (float)((int)(c4 & 3u) - 1) - ppx, offy = (float)((int)(c4 >> 2) - 1) - ppy;
        float vx = (offx * (dirx)) + (offy * diry);
        float vy = (offx * (-diry)) + (offy * dirx);
        vx *= len2x;
        vy *= len2y;
        float d2 = vx * vx + vy * vy;
        d2 = fminf(d2, clp);
        float wB = (float)(2.0 / 5.0) * d2 + -1.0f;
        float wA = lob * d2 + -1.0f;
        wB *= wB;
        wA *= wA;
        wB = (float)(25.0 / 16.0) * wB + (float)(-(25.0 / 16.0 - 1.0));
        w[s] = wB * wA;
    }
    // lane c reads component c of every cell: R, G, B, and the plane's constant 1 in lane 3 (1 * w == w: the weight sum).
    // Bytes are decoded b/255 as fma(b, k_hi, b * k_lo) (unorm8_to_unit); lane 3 decodes its 1 with (1, 0): still 1.
    typedef std::conditional_t<std::is_same_v<COLT, float4>, float, half_t> comp_t;
    OVRFSR_PTR(const comp_t) ch = OVRFSR_AS(const comp_t, col + base) + q;
    const float k_hi = (BYTES && q != 3) ? __uint_as_float(0x3b808081u) : 1.0f, k_lo = (BYTES && q != 3) ? __uint_as_float(0xaf7efeffu) : 0.0f;
    float acc = 0.0f, cf = 0.0f, cg = 0.0f, cj = 0.0f, ck = 0.0f;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        float c = (float)ch[4 * (kDy[i] * pitch + kDx[i])];
        if constexpr (BYTES) c = __builtin_fmaf(c, k_hi, c * k_lo);
        const float wi = quad_bcast(w[i % 3], i / 3);
        acc += c * wi;
        if (i == 4) cf = c;
        if (i == 9) cg = c;
        if (i == 3) cj = c;
        if (i == 6) ck = c;
    }
    const float mn = fminf(fminf(cf, fminf(cg, cj)), ck), mx = fmaxf(fmaxf(cf, fmaxf(cg, cj)), ck);
    const float rW = 1.0f / quad_bcast<3>(acc); // IEEE, correctly rounded (== the oracle's ARcpF1)
    return fminf(mx, fmaxf(mn, acc * rW));
}

// Stage the clamped input footprint of one tile into LDS (colour + luma planes), then derive the
// per-texel analysis plane.  tile_x0/tile_y0 = image coordinate of LDS cell (0,0) (may be < 0).
template <int IN_FMT>
__device__ __forceinline__ void easu_stage(OVRFSR_PTR_R(const uint8_t) img, uint32_t pitchB, int inW, int inH, int tile_x0,
                                           int tile_y0, int cellsW, int cellsH, OVRFSR_PTR_R(typename EasuTraits<IN_FMT>::cell_t) col,
                                           OVRFSR_PTR_R(float) lum, OVRFSR_PTR_R(float4) ana)
{
    typedef EasuTraits<IN_FMT> T;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int cy = ty; cy < cellsH; cy += 8) {
        const int sy = clampi(tile_y0 + cy, 0, inH - 1);
        for (int cx = tx; cx < cellsW; cx += 32) {
            const int sx = clampi(tile_x0 + cx, 0, inW - 1);
            const int idx = cy * cellsW + cx;
            if constexpr (T::byte_domain) {
                uint32_t v = *OVRFSR_AT(const uint32_t, img + (size_t)sy * pitchB + (size_t)sx * 4);
                float rb = (float)(v & 0xffu), gb = (float)((v >> 8) & 0xffu), bb = (float)((v >> 16) & 0xffu);
                half4_t h = {(half_t)rb, (half_t)gb, (half_t)bb, (half_t)0.0f};
                col[idx] = h;
                float r = unorm8_to_unit(rb), g = unorm8_to_unit(gb), b = unorm8_to_unit(bb);
                lum[idx] = b * 0.5f + (r * 0.5f + g); // ffx_fsr1.h:363 (x0.5 is exact: fusing cannot change it)
            } else {
                float4 c = load_unit<IN_FMT>(img, pitchB, sx, sy);
                if constexpr (T::wide) col[idx] = c;
                else { half4_t h = {(half_t)c.x, (half_t)c.y, (half_t)c.z, (half_t)0.0f}; col[idx] = h; }
                lum[idx] = c.z * 0.5f + (c.x * 0.5f + c.y);
            }
        }
    }
    __syncthreads();
    // analysis of every cell that can be an f/g/j/k texel: x in [1,cellsW-2], y in [1,cellsH-2]
    for (int cy = 1 + ty; cy < cellsH - 1; cy += 8) {
        for (int cx = 1 + tx; cx < cellsW - 1; cx += 32) {
            const int idx = cy * cellsW + cx;
            ana[idx] = easu_analyse(lum[idx - cellsW], lum[idx - 1], lum[idx], lum[idx + 1], lum[idx + cellsW]);
        }
    }
    __syncthreads();
}

__device__ __forceinline__ size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// EASU pass: grid = (tilesX*tilesY, 1, batch), block = 256.  Dynamic LDS = colour + luma + analysis planes.
template <int IN_FMT, int OUT_FMT>
__global__ __launch_bounds__(256) void easu_kernel(const ovrfsr::EasuArgs a)
{
    typedef EasuTraits<IN_FMT> T;
    typedef typename T::cell_t cell_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    OVRFSR_LDS_POISON(smem, a.ldsBytes);

    const uint32_t img_i = blockIdx.z;
    const uint32_t eye = (a.m.first_eye ^ (img_i & a.m.alternate)) & 1u;
    // mask-sorted launches (product build, footprints wider than the fixed-pitch kernels) hand every block its tile
    const uint32_t tile = a.tileList ? OVRFSR_TILE_LIST(a)[blockIdx.x] : xcd_tile_index(blockIdx.x, a.tilesX * a.tilesY);
    uint32_t tileX, tileY;
    tile_xy(tile, a.tilesX, a.tilesXMagic, tileX, tileY);
    OVRFSR_IMAGES(IN_FMT, OUT_FMT);

    const uint32_t inside_bits = tile_mask_bits(a.m, eye, tileX, tileY);
    const int ox0 = (int)tileX * ovrfsr::kTileW, oy0 = (int)tileY * ovrfsr::kTileH;
    const int lx = threadIdx.x & 31, ly0 = threadIdx.x >> 5;
    const int ox = ox0 + lx;

    // input footprint of the tile: 'f' texel index of its first pixel, minus the 1-texel apron
    const int tile_x0 = (int)floorf(mad_unfused((float)ox0, a.sx, a.cx)) - 1;
    const int tile_y0 = (int)floorf(mad_unfused((float)oy0, a.sy, a.cy)) - 1;

    const size_t ncell = (size_t)a.cellsW * a.cellsH;
    OVRFSR_PTR(cell_t) col = OVRFSR_CARVE(cell_t, reinterpret_cast<cell_t *>(smem), ncell, 0, K_EASU_COL, smem, a.ldsBytes);
    OVRFSR_PTR(float4) ana = OVRFSR_CARVE(float4, reinterpret_cast<float4 *>(smem + align16(ncell * sizeof(cell_t))), ncell, 0, K_EASU_ANA, smem, a.ldsBytes);
    OVRFSR_PTR(float) lum = OVRFSR_CARVE(float, reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(OVRFSR_RAW(ana)) + ncell * sizeof(float4)), ncell, 0, K_EASU_LUM, smem, a.ldsBytes);

    if (inside_bits != 0u) // uniform over the workgroup
        easu_stage<IN_FMT>(in, a.v.in_pitch, a.v.inW, a.v.inH, tile_x0, tile_y0, a.cellsW, a.cellsH, col, lum, ana);

    if (ox >= a.v.outW) return;
    const float ppx_raw = mad_unfused((float)ox, a.sx, a.cx);
    const float fpx = floorf(ppx_raw);
    const float ppx = ppx_raw - fpx;
    const int cellx = (int)fpx - tile_x0;
    const uint32_t gbit_x = (uint32_t)(lx >> 4);

#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const int ly = ly0 + 8 * k;
        const int oy = oy0 + ly;
        if (oy >= a.v.outH) break;
        const bool inside = (inside_bits >> (gbit_x + 2u * (uint32_t)(ly >> 4))) & 1u;
        if (inside) {
            const float ppy_raw = mad_unfused((float)oy, a.sy, a.cy);
            const float fpy = floorf(ppy_raw);
            const float ppy = ppy_raw - fpy;
            const int celly = (int)fpy - tile_y0;
            float r, g, b;
            easu_resolve<T::byte_domain, cell_t>(col, ana, celly * a.cellsW + cellx, a.cellsW, ppx, ppy, r, g, b);
            store_unit<OUT_FMT>(out, a.v.out_pitch, ox, oy, r, g, b, 1.0f);
        } else {
            float4 c = bilinear_global<IN_FMT>(in, a.v.in_pitch, a.v.inW, a.v.inH, ox, oy, (float)a.v.outW, (float)a.v.outH);
            store_unit<OUT_FMT>(out, a.v.out_pitch, ox, oy, c.x, c.y, c.z, 1.0f);
        }
    }
}


#if !OVRFSR_STRICT
// ------------------------------------------------------------------------------------------------
// EASU, product build.  Same function as easu_kernel above (which stays as the strict/generic form),
// re-associated for the gfx950 VALU.  Measured issue cost per wave-instruction (tools/ubench/
// valu_rates.hip): v_fma/mul/add_f32, int add/shift/and/or ~2.7 cycles; v_min/max/med3, every v_pk_*,
// v_cvt_*, v_fma_mix, 3-operand int ops ~4.2; v_rcp 8.2.  So:
//   * colours sit in LDS as fp32 (R,G,B,1) -- one ds_read_b128 per tap, no per-tap conversion, and
//     the constant 1 turns "aW += w" into the high half of a v_pk_fma_f32;
//   * the LDS row pitch is a template constant: all 16 LDS reads of a pixel use one base VGPR plus
//     immediate offsets;
//   * the per-tap rotation/anisotropy  v = (off.x*dir.x + off.y*dir.y, -off.x*dir.y + off.y*dir.x)*len2
//     is linear in the integer tap offset: v(tx,ty) = r(ty) + tx*c0 with two per-pixel column vectors
//     c0, c1 (r(ty) = -ppx*c0 + (ty-ppy)*c1), i.e. one v_pk_add_f32 per tap instead of 6 scalar ops;
//   * the weight polynomial runs on tap PAIRS in v_pk_*_f32;
//   * the weight polynomial is expanded to a quartic in d^2 once per pixel (4 packed FMAs per tap pair);
//   * RGBA8 results are packed with v_cvt_pk_u8_f32 (round-to-nearest-even + clamp; differs from
//     floor(x+0.5) only on exact .5 ties).
// These re-associations change rounding only (measured max-abs vs the oracle: see tests).
// ------------------------------------------------------------------------------------------------
// e2_t: the two-vector type of the product resolve: packed (v_pk_*_f32 on 64-bit register pairs).  (The same expressions on two scalars
// were measured in round 4 -- profiles/r04_easu_scalar_ab.txt: 47 % more instructions, the same time.)
typedef f2_t e2_t;
__device__ __forceinline__ e2_t mke2(float a, float b) { return mk2(a, b); }

// Direction of the product resolve: the bilinear blend of the four per-texel gradient directions, in the REFERENCE's accumulation
// order with every product and every sum rounded separately (ffx_fsr1.h:383-386 through FsrEasuSetF :295-313; easu_resolve), and
// its squared length likewise.  This is the one ill-conditioned step of the filter: the four terms are O(1) and may cancel down to
// |dir|^2 ~ 2^-15 (the zero guard), so a re-associated (FMA) sum differs from the reference's by up to 2^-24 * 1 / 2^-7.5 relative
// -- 1e-5 of the direction, 6e-3 of a byte in the result, three near-tie bands (found by tools/debug/easu_err_search.py, round 4:
// profiles/r04_easu_err_search.txt) -- and a dirR on the other side of the 1/32768 threshold would switch the whole kernel
// shape.  With dir and dirR bit-identical to the reference's, everything downstream is well-conditioned and the re-associations
// of the product build stay inside the band.  3 packed instructions and 1 scalar more than the contracted form.
__device__ __forceinline__ e2_t easu_dir_ref(const float4 &aF, const float4 &aG4, const float4 &aJ, const float4 &aK, float ws, float wt,
                                             float wu, float wv, float &dirR)
{
#pragma clang fp contract(off)
    e2_t dir = mke2(aF.x, aF.y) * ws;
    e2_t t = mke2(aG4.x, aG4.y) * wt;
    dir = dir + t;
    t = mke2(aJ.x, aJ.y) * wu;
    dir = dir + t;
    t = mke2(aK.x, aK.y) * wv;
    dir = dir + t;
    const float dx2 = dir.x * dir.x, dy2 = dir.y * dir.y;
    dirR = dx2 + dy2;
    return dir;
}

// colour-plane cell of the product kernels: float4 (R, G, B, 1).  (A plane of four halves per cell -- exact for the bytes of an RGBA8
// texel and for RGBA16F texels -- was measured for the fused kernel in round 4: profiles/r04_fused_variants.txt.)
__device__ __forceinline__ float4 ldc(OVRFSR_PTR_RC(float4) col, int i) { return col[i]; }
__device__ __forceinline__ void stc(OVRFSR_PTR_R(float4) col, int i, float r, float g, float b) { col[i] = make_float4(r, g, b, 1.0f); }

template <int PITCH, typename COLT = float4>
__device__ __forceinline__ void easu_resolve_fast(OVRFSR_PTR_RC(COLT) col, OVRFSR_PTR_RC(float4) ana, int base,
                                                  float ppx, float ppy, float &outR, float &outG, float &outB)
{
    const float4 aF = ana[base], aG4 = ana[base + 1], aJ = ana[base + PITCH], aK = ana[base + PITCH + 1];
    const float omx = 1.0f - ppx, omy = 1.0f - ppy;
    const float ws = omx * omy, wt = ppx * omy, wu = omx * ppy, wv = ppx * ppy;
    float dirR;
    e2_t dir = easu_dir_ref(aF, aG4, aJ, aK, ws, wt, wu, wv, dirR);
    // (the length terms are all >= 0: no cancellation, the contracted sum is within a few ulp of the reference's)
    e2_t ln2 = mke2(aF.z, aF.w) * ws;
    ln2 = mke2(aG4.z, aG4.w) * wt + ln2;
    ln2 = mke2(aJ.z, aJ.w) * wu + ln2;
    ln2 = mke2(aK.z, aK.w) * wv + ln2;
    float len = ln2.x + ln2.y;

    const bool zro = dirR < (float)(1.0 / 32768.0);
    dirR = prx_lo_rsq(dirR);
    dirR = zro ? 1.0f : dirR;
    dir.x = zro ? 1.0f : dir.x;
    dir = dir * dirR;
    len = len * 0.5f;
    len *= len;
    const float stretch = (dir.x * dir.x + dir.y * dir.y) * prx_lo_rcp(fmaxf(fabsf(dir.x), fabsf(dir.y)));
    const float len2x = 1.0f + (stretch - 1.0f) * len;
    const float len2y = 1.0f + -0.5f * len;
    const float lob = 0.5f + (float)((1.0 / 4.0 - 0.04) - 0.5) * len;
    const float clp = prx_lo_rcp(lob);
    // The window clamp min(d2, clp) becomes the free [0,1] saturate of the instruction that produces d2 when distances are
    // measured in units of sqrt(clp): u = d2/clp.  One v_rsq per pixel and two multiplies replace twelve v_min (slow class).
    const float q = __builtin_amdgcn_rsqf(clp);
    const float sx = len2x * q, sy = len2y * q;

    // v(tx,ty) = (tx-ppx)*c0 + (ty-ppy)*c1
    const e2_t c0 = mke2(dir.x * sx, -dir.y * sy);
    const e2_t c1 = mke2(dir.y * sx, dir.x * sy);
    const e2_t rm = c0 * (-ppx) + c1 * (-1.0f - ppy); // row ty = -1, tx = 0
    const e2_t r0 = rm + c1, r1 = r0 + c1, r2 = r1 + c1;
    const e2_t c02 = c0 + c0;

    e2_t accRG = mke2(0.0f, 0.0f), accBW = mke2(0.0f, 0.0f);
    // one pair of taps: distances (saturated = window clamp), weights (packed), accumulate.
    // w(d) = (25/16*(2/5*d-1)^2 - 9/16) * (lob*d-1)^2  (ffx_fsr1.h:265-270).  The first factor is a difference of squares:
    // 25/16*(2/5*d-1)^2 - 9/16 = 1/4 (d-4)(d-1) = 1 - 5/4 d + 1/4 d^2, so with d = clp*u (u = the saturated |v|^2):
    //   w = P(u) * Q(u)^2,   P = 1 + u*(p1 + u*p2),  p1 = -5/4 clp, p2 = 1/4 clp^2,   Q = (lob*clp)*u - 1
    // 5 packed ops per tap pair and 5 scalar ops per pixel.  (Rounds 1-2 expanded w to ONE quartic in u, 4 packed ops per
    // pair and 13 per pixel: the same cycles, but it cancels terms of magnitude ~10 down to w ~ 0.01 at the window edge --
    // where the colours are farthest from the result -- and that was most of the product build's distance from the
    // reference-order evaluation: 3.1e-3 of a byte at worst against 6e-4 in this form, profiles/r03_easu_err.txt.)
    const float pL = lob * clp, p1 = -1.25f * clp, p2 = (0.5f * clp) * (0.5f * clp);
#define OVRFSR_PAIR(VA, CA, VB, CB)                                                                       \
    do {                                                                                                  \
        const e2_t va = (VA), vb = (VB);                                                                  \
        const e2_t d2 = mke2(__builtin_amdgcn_fmed3f(__builtin_fmaf(va.y, va.y, va.x * va.x), 0.0f, 1.0f), \
                            __builtin_amdgcn_fmed3f(__builtin_fmaf(vb.y, vb.y, vb.x * vb.x), 0.0f, 1.0f)); \
        e2_t wp = d2 * p2 + p1;                                                                           \
        wp = wp * d2 + 1.0f;                                                                              \
        const e2_t wq = d2 * pL + -1.0f;                                                                  \
        const e2_t w = wp * (wq * wq);                                                                    \
        accRG = mke2((CA).x, (CA).y) * w.x + accRG;                                                         \
        accBW = mke2((CA).z, (CA).w) * w.x + accBW;                                                         \
        accRG = mke2((CB).x, (CB).y) * w.y + accRG;                                                         \
        accBW = mke2((CB).z, (CB).w) * w.y + accBW;                                                         \
    } while (0)

    const float4 cf = ldc(col, base), cg = ldc(col, base + 1), cj = ldc(col, base + PITCH), ck = ldc(col, base + PITCH + 1);
    {
        const float4 cb = ldc(col, base - PITCH), cc = ldc(col, base - PITCH + 1);
        OVRFSR_PAIR(rm, cb, rm + c0, cc);                 // b c
    }
    {
        const float4 ce = ldc(col, base - 1);
        OVRFSR_PAIR(r0 - c0, ce, r0, cf);                 // e f
    }
    {
        const float4 ch = ldc(col, base + 2);
        OVRFSR_PAIR(r0 + c0, cg, r0 + c02, ch);           // g h
    }
    {
        const float4 ci = ldc(col, base + PITCH - 1);
        OVRFSR_PAIR(r1 - c0, ci, r1, cj);                 // i j
    }
    {
        const float4 cl = ldc(col, base + PITCH + 2);
        OVRFSR_PAIR(r1 + c0, ck, r1 + c02, cl);           // k l
    }
    {
        const float4 cn = ldc(col, base + 2 * PITCH), co = ldc(col, base + 2 * PITCH + 1);
        OVRFSR_PAIR(r2, cn, r2 + c0, co);                 // n o
    }
#undef OVRFSR_PAIR
    const float rW = __builtin_amdgcn_rcpf(accBW.y);
    const float mnR = raw_min(raw_min3(cf.x, cg.x, cj.x), ck.x), mxR = raw_max(raw_max3(cf.x, cg.x, cj.x), ck.x);
    const float mnG = raw_min(raw_min3(cf.y, cg.y, cj.y), ck.y), mxG = raw_max(raw_max3(cf.y, cg.y, cj.y), ck.y);
    const float mnB = raw_min(raw_min3(cf.z, cg.z, cj.z), ck.z), mxB = raw_max(raw_max3(cf.z, cg.z, cj.z), ck.z);
    // min(max4, max(min4, x)) == med3(x, min4, max4) for min4 <= max4 (NaN x -> min4 either way)
    outR = __builtin_amdgcn_fmed3f(accRG.x * rW, mnR, mxR);
    outG = __builtin_amdgcn_fmed3f(accRG.y * rW, mnG, mxG);
    outB = __builtin_amdgcn_fmed3f(accBW.x * rW, mnB, mxB);
}

// ------------------------------------------------------------------------------------------------
// Two vertically adjacent output pixels A (row oy) and B (row oy+1) of one column, resolved together (round 3).
// When upscaling, B's 'f' texel is A's (DIFF = 0) or the one below it (DIFF = 1): the two 12-tap footprints share 12 / 8 of
// their colour cells and 4 / 2 of their analysis cells, so the pair reads 16 / 22 LDS cells instead of 32 -- the kernel's
// LDS reads are what co-limits it (DESIGN.md "Which roof").  The arithmetic per (pixel, tap) is easu_resolve_fast's; a
// packed operation now carries the SAME cell for the two pixels (or one A-only and one B-only cell) instead of two cells
// of one pixel, with the per-pixel polynomial coefficients as packed operands -- the same number of VALU instructions.
// ------------------------------------------------------------------------------------------------
struct EasuPx { e2_t c0, c1, rm; float p1, p2, pL; }; // tap vector of cell (x, y) relative to 'f': rm + x*c0 + (y+1)*c1

__device__ __forceinline__ EasuPx easu_px_setup(const float4 &aF, const float4 &aG4, const float4 &aJ, const float4 &aK, float ppx, float ppy)
{
    const float omx = 1.0f - ppx, omy = 1.0f - ppy;
    const float ws = omx * omy, wt = ppx * omy, wu = omx * ppy, wv = ppx * ppy;
    float dirR;
    e2_t dir = easu_dir_ref(aF, aG4, aJ, aK, ws, wt, wu, wv, dirR); // reference order, unfused: the ill-conditioned step
    e2_t ln2 = mke2(aF.z, aF.w) * ws;
    ln2 = mke2(aG4.z, aG4.w) * wt + ln2;
    ln2 = mke2(aJ.z, aJ.w) * wu + ln2;
    ln2 = mke2(aK.z, aK.w) * wv + ln2;
    float len = ln2.x + ln2.y;
    const bool zro = dirR < (float)(1.0 / 32768.0);
    dirR = prx_lo_rsq(dirR);
    dirR = zro ? 1.0f : dirR;
    dir.x = zro ? 1.0f : dir.x;
    dir = dir * dirR;
    len = len * 0.5f;
    len *= len;
    const float stretch = (dir.x * dir.x + dir.y * dir.y) * prx_lo_rcp(fmaxf(fabsf(dir.x), fabsf(dir.y)));
    const float len2x = 1.0f + (stretch - 1.0f) * len;
    const float len2y = 1.0f + -0.5f * len;
    const float lob = 0.5f + (float)((1.0 / 4.0 - 0.04) - 0.5) * len;
    const float clp = prx_lo_rcp(lob);
    const float q = __builtin_amdgcn_rsqf(clp); // distances in units of sqrt(clp): the window clamp is a [0,1] saturate
    const float sx = len2x * q, sy = len2y * q;
    EasuPx o;
    o.c0 = mke2(dir.x * sx, -dir.y * sy);
    o.c1 = mke2(dir.y * sx, dir.x * sy);
    o.rm = o.c0 * (-ppx) + o.c1 * (-1.0f - ppy);
    o.pL = lob * clp; o.p1 = -1.25f * clp; o.p2 = (0.5f * clp) * (0.5f * clp);
    return o;
}

template <int PITCH, int DIFF>
__device__ __forceinline__ void easu_resolve_fast2(OVRFSR_PTR_RC(float4) col, OVRFSR_PTR_RC(float4) ana, int base, float ppx,
                                                   float ppyA, float ppyB, float &aR, float &aG, float &aB, float &bR, float &bG, float &bB)
{
    static_assert(DIFF == 0 || DIFF == 1, "B's f texel is A's or the one below");
    const float4 n00 = ana[base], n10 = ana[base + 1], n01 = ana[base + PITCH], n11 = ana[base + PITCH + 1];
    const EasuPx A = easu_px_setup(n00, n10, n01, n11, ppx, ppyA);
    EasuPx B;
    if constexpr (DIFF == 0) {
        B = easu_px_setup(n00, n10, n01, n11, ppx, ppyB);
    } else {
        const float4 n02 = ana[base + 2 * PITCH], n12 = ana[base + 2 * PITCH + 1];
        B = easu_px_setup(n01, n11, n02, n12, ppx, ppyB);
    }
    const e2_t P2 = mke2(A.p2, B.p2), P1 = mke2(A.p1, B.p1), PL = mke2(A.pL, B.pL);
    e2_t aRG = mke2(0.0f, 0.0f), aBW = mke2(0.0f, 0.0f), bRG = mke2(0.0f, 0.0f), bBW = mke2(0.0f, 0.0f);
    // weights of one cell for A (vector va) and one cell for B (vector vb): w = P(u) * Q(u)^2 (see easu_resolve_fast)
    auto weights = [&](e2_t va, e2_t vb) {
        const e2_t d2 = mke2(__builtin_amdgcn_fmed3f(__builtin_fmaf(va.y, va.y, va.x * va.x), 0.0f, 1.0f),
                            __builtin_amdgcn_fmed3f(__builtin_fmaf(vb.y, vb.y, vb.x * vb.x), 0.0f, 1.0f));
        e2_t wp = d2 * P2 + P1;
        wp = wp * d2 + 1.0f;
        const e2_t wq = d2 * PL + -1.0f;
        return wp * (wq * wq);
    };
    auto accA = [&](const float4 &c, float w) { aRG = mke2(c.x, c.y) * w + aRG; aBW = mke2(c.z, c.w) * w + aBW; };
    auto accB = [&](const float4 &c, float w) { bRG = mke2(c.x, c.y) * w + bRG; bBW = mke2(c.z, c.w) * w + bBW; };
    auto both = [&](const float4 &c, e2_t va, e2_t vb) { const e2_t w = weights(va, vb); accA(c, w.x); accB(c, w.y); };
    // row vectors (x = 0): A's rows -1..2 of its footprint are cell rows -1..2; B's are cell rows DIFF-1..DIFF+2
    const e2_t rA0 = A.rm, rA1 = rA0 + A.c1, rA2 = rA1 + A.c1, rA3 = rA2 + A.c1;
    const e2_t rB0 = B.rm, rB1 = rB0 + B.c1, rB2 = rB1 + B.c1, rB3 = rB2 + B.c1;
    const e2_t cA = A.c0, cB = B.c0, cA2 = cA + cA, cB2 = cB + cB;
    float mnR, mxR, mnG, mxG, mnB, mxB, nnR, nxR, nnG, nxG, nnB, nxB;
    if constexpr (DIFF == 0) {
        // identical footprints: every cell serves both pixels
        const float4 c00 = col[base], c10 = col[base + 1], c01 = col[base + PITCH], c11 = col[base + PITCH + 1];
        { const float4 c = col[base - PITCH]; both(c, rA0, rB0); }
        { const float4 c = col[base - PITCH + 1]; both(c, rA0 + cA, rB0 + cB); }
        { const float4 c = col[base - 1]; both(c, rA1 - cA, rB1 - cB); }
        both(c00, rA1, rB1);
        both(c10, rA1 + cA, rB1 + cB);
        { const float4 c = col[base + 2]; both(c, rA1 + cA2, rB1 + cB2); }
        { const float4 c = col[base + PITCH - 1]; both(c, rA2 - cA, rB2 - cB); }
        both(c01, rA2, rB2);
        both(c11, rA2 + cA, rB2 + cB);
        { const float4 c = col[base + PITCH + 2]; both(c, rA2 + cA2, rB2 + cB2); }
        { const float4 c = col[base + 2 * PITCH]; both(c, rA3, rB3); }
        { const float4 c = col[base + 2 * PITCH + 1]; both(c, rA3 + cA, rB3 + cB); }
        mnR = raw_min(raw_min3(c00.x, c10.x, c01.x), c11.x); mxR = raw_max(raw_max3(c00.x, c10.x, c01.x), c11.x);
        mnG = raw_min(raw_min3(c00.y, c10.y, c01.y), c11.y); mxG = raw_max(raw_max3(c00.y, c10.y, c01.y), c11.y);
        mnB = raw_min(raw_min3(c00.z, c10.z, c01.z), c11.z); mxB = raw_max(raw_max3(c00.z, c10.z, c01.z), c11.z);
        nnR = mnR; nxR = mxR; nnG = mnG; nxG = mxG; nnB = mnB; nxB = mxB;
    } else {
        // B's footprint is A's moved down one cell row: cell rows 0..2 are shared (8 cells), row -1 and the outer cells of
        // row 0 are A's alone, the outer cells of row 2 and row 3 are B's alone; an A-only and a B-only cell share a packed
        // weight evaluation.  B's row r of ITS footprint is cell row r + 1.
        const float4 c00 = col[base], c10 = col[base + 1], c01 = col[base + PITCH], c11 = col[base + PITCH + 1];
        const float4 c02 = col[base + 2 * PITCH], c12 = col[base + 2 * PITCH + 1];
        { const float4 ca = col[base - PITCH], cb = col[base + 3 * PITCH]; const e2_t w = weights(rA0, rB3); accA(ca, w.x); accB(cb, w.y); }                   // A b | B n
        { const float4 ca = col[base - PITCH + 1], cb = col[base + 3 * PITCH + 1]; const e2_t w = weights(rA0 + cA, rB3 + cB); accA(ca, w.x); accB(cb, w.y); } // A c | B o
        { const float4 ca = col[base - 1], cb = col[base + 2 * PITCH - 1]; const e2_t w = weights(rA1 - cA, rB2 - cB); accA(ca, w.x); accB(cb, w.y); }         // A e | B i
        { const float4 ca = col[base + 2], cb = col[base + 2 * PITCH + 2]; const e2_t w = weights(rA1 + cA2, rB2 + cB2); accA(ca, w.x); accB(cb, w.y); }       // A h | B l
        both(c00, rA1, rB0);                 // A f | B b
        both(c10, rA1 + cA, rB0 + cB);       // A g | B c
        { const float4 c = col[base + PITCH - 1]; both(c, rA2 - cA, rB1 - cB); }     // A i | B e
        both(c01, rA2, rB1);                 // A j | B f
        both(c11, rA2 + cA, rB1 + cB);       // A k | B g
        { const float4 c = col[base + PITCH + 2]; both(c, rA2 + cA2, rB1 + cB2); }   // A l | B h
        both(c02, rA3, rB2);                 // A n | B j
        both(c12, rA3 + cA, rB2 + cB);       // A o | B k
        // the dering boxes of A (c00 c10 c01 c11) and B (c01 c11 c02 c12) share cells c01 and c11: their extrema once (18 min/max for 24)
        const float loR = raw_min(c01.x, c11.x), hiR = raw_max(c01.x, c11.x);
        const float loG = raw_min(c01.y, c11.y), hiG = raw_max(c01.y, c11.y);
        const float loB = raw_min(c01.z, c11.z), hiB = raw_max(c01.z, c11.z);
        mnR = raw_min3(c00.x, c10.x, loR); mxR = raw_max3(c00.x, c10.x, hiR);
        mnG = raw_min3(c00.y, c10.y, loG); mxG = raw_max3(c00.y, c10.y, hiG);
        mnB = raw_min3(c00.z, c10.z, loB); mxB = raw_max3(c00.z, c10.z, hiB);
        nnR = raw_min3(loR, c02.x, c12.x); nxR = raw_max3(hiR, c02.x, c12.x);
        nnG = raw_min3(loG, c02.y, c12.y); nxG = raw_max3(hiG, c02.y, c12.y);
        nnB = raw_min3(loB, c02.z, c12.z); nxB = raw_max3(hiB, c02.z, c12.z);
    }
    const float rWA = __builtin_amdgcn_rcpf(aBW.y), rWB = __builtin_amdgcn_rcpf(bBW.y);
    aR = __builtin_amdgcn_fmed3f(aRG.x * rWA, mnR, mxR);
    aG = __builtin_amdgcn_fmed3f(aRG.y * rWA, mnG, mxG);
    aB = __builtin_amdgcn_fmed3f(aBW.x * rWA, mnB, mxB);
    bR = __builtin_amdgcn_fmed3f(bRG.x * rWB, nnR, nxR);
    bG = __builtin_amdgcn_fmed3f(bRG.y * rWB, nnG, nxG);
    bB = __builtin_amdgcn_fmed3f(bBW.x * rWB, nnB, nxB);
}

// staging for the product build: colour plane float4 (R,G,B,1) [bytes 0..255 for RGBA8 input, unit
// otherwise], luma plane, analysis plane (dirX, dirY, lenX^2, lenY^2), all with row pitch PITCH (a multiple of 4).
// The per-thread setup of this pass is amortised over few cells (a 32x32 tile at scale 3/4 stages 28x28 = 784 cells with
// 256 threads), so both sweeps give every lane FOUR horizontally adjacent cells:
//   * RGBA8 tiles whose footprint lies inside the image (all but the border tiles; workgroup-uniform test): one 16-byte
//     load = 4 texels, no clamps, no per-cell index split or 64-bit address arithmetic, one 16-byte store of the 4 lumas;
//     border tiles and the other formats keep the per-texel sweep with clamp addressing;
//   * analysis: a lane takes 4 VERTICALLY adjacent cells of one column: 14 luma reads per 4 cells instead of 20, the
//     vertical differences l[i+1]-l[i] shared by neighbouring cells, and consecutive lanes write consecutive cells.  (Four
//     horizontally adjacent cells per lane cost the same VALU work but their ds_write_b128 are 4-way bank-conflicted --
//     64-byte lane stride --, which the fused kernel at 3 workgroups per CU pays for: C5 12.0 k -> 9.6 k pairs/s.)
//     The last group reads up to ovrfsr::kLumPadRows rows past the luma plane: the launchers allocate them.
// (round 1: 34 + 18 VALU instructions per output pixel for the two sweeps; this form: 17 + 14.)
typedef uint32_t u32x4_a4_t __attribute__((ext_vector_type(4), aligned(4)));

// tmax (optional, LDS, zeroed by the caller before the call): receives the bit pattern of the largest |channel| of the staged footprint
// -- what the half near-tie guard scales its band with on HDR tiles (near_tie_half3_hdr); only float sources compute it.
template <int IN_FMT, int PITCH, int NT = ovrfsr::kThreads, typename COLT = float4>
__device__ __forceinline__ void easu_stage_fast(OVRFSR_PTR_R(const uint8_t) img, uint32_t pitchB, int inW, int inH, int tile_x0,
                                                int tile_y0, int cellsH, OVRFSR_PTR_R(COLT) col, OVRFSR_PTR_R(float) lum,
                                                OVRFSR_PTR_R(float4) ana, uint32_t *__restrict__ tmax = nullptr)
{
    constexpr bool kFloatSrc = IN_FMT == ovrfsr::FMT_RGBA16F || IN_FMT == ovrfsr::FMT_RGBA32F || IN_FMT == ovrfsr::FMT_R11G11B10F;
    [[maybe_unused]] float lmax = 0.0f; // this lane's largest |channel|
    static_assert(PITCH % 4 == 0, "quad sweeps need a row pitch that is a multiple of 4 cells");
    constexpr int SEGS = PITCH / 4;
    const int ncell = PITCH * cellsH;
    bool quad = false;
    if constexpr (IN_FMT == ovrfsr::FMT_RGBA8 || IN_FMT == ovrfsr::FMT_RGBA16F || IN_FMT == ovrfsr::FMT_RGBA8_MS4 || IN_FMT == ovrfsr::FMT_R11G11B10F)
        quad = tile_x0 >= 0 && tile_y0 >= 0 && tile_x0 + PITCH <= inW && tile_y0 + cellsH <= inH; // pad columns are loaded too
    if (quad) {
        if constexpr (IN_FMT == ovrfsr::FMT_RGBA8 || IN_FMT == ovrfsr::FMT_RGBA16F || IN_FMT == ovrfsr::FMT_RGBA8_MS4 || IN_FMT == ovrfsr::FMT_R11G11B10F) {
            constexpr uint32_t TB = TexelBytes<IN_FMT>::v;
            OVRFSR_PTR_R(const uint8_t) base = img + ((size_t)tile_y0 * pitchB + (size_t)tile_x0 * TB); // uniform
            // (no loop vectorisation / interleaving in these sweeps: packing across iterations costs more in register
            // shuffles, separate |x| and saturate instructions than the packed operations save)
#pragma clang loop vectorize(disable) interleave(disable)
#pragma unroll 1
            for (int t = threadIdx.x; t < SEGS * cellsH; t += NT) {
                const int row = t / SEGS, seg = t - row * SEGS;
                OVRFSR_PTR(const uint8_t) src = base + ((uint32_t)row * pitchB + (uint32_t)seg * (4u * TB)); // footprint rows x row pitch < 4 GiB
                const int idx = row * PITCH + 4 * seg;
                float l[4];
                if constexpr (IN_FMT == ovrfsr::FMT_RGBA8) {
                    const u32x4_a4_t v = *OVRFSR_AT(const u32x4_a4_t, src);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float rb = (float)(v[j] & 0xffu), gb = (float)((v[j] >> 8) & 0xffu), bb = (float)((v[j] >> 16) & 0xffu);
                        stc(col, idx + j, rb, gb, bb);
                        const float r = unorm8_to_unit(rb), g = unorm8_to_unit(gb), b = unorm8_to_unit(bb);
                        l[j] = b * 0.5f + (r * 0.5f + g); // ffx_fsr1.h:363 on the exact b/255 (see DESIGN "A parity lesson")
                    }
                } else if constexpr (IN_FMT == ovrfsr::FMT_RGBA8_MS4) {
                    // 4-sample RGBA8: one 16-byte load per texel (its 4 samples), resolved before anything is staged -- then the RGBA8 body
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const u32x4_a4_t q = *OVRFSR_AT(const u32x4_a4_t, src + 16 * j);
                        const uint32_t s4[4] = {q[0], q[1], q[2], q[3]};
                        const uint32_t v = resolve_unorm8<4>(s4);
                        const float rb = (float)(v & 0xffu), gb = (float)((v >> 8) & 0xffu), bb = (float)((v >> 16) & 0xffu);
                        stc(col, idx + j, rb, gb, bb);
                        const float r = unorm8_to_unit(rb), g = unorm8_to_unit(gb), b = unorm8_to_unit(bb);
                        l[j] = b * 0.5f + (r * 0.5f + g);
                    }
                } else if constexpr (IN_FMT == ovrfsr::FMT_R11G11B10F) {
                    // packed float words: one 16-byte load = 4 texels (rows are only 4-byte aligned, as RGBA8's), decoded to the fp32 values
                    // the RGBA16F copy of the resolve pass holds -- then the RGBA16F body
                    const u32x4_a4_t v = *OVRFSR_AT(const u32x4_a4_t, src);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float r, g, b;
                        unpack_r11g11b10f(v[j], r, g, b);
                        if (tmax) lmax = fmaxf(lmax, fmaxf(fabsf(r), fmaxf(fabsf(g), fabsf(b))));
                        stc(col, idx + j, r, g, b);
                        l[j] = b * 0.5f + (r * 0.5f + g);
                    }
                } else {
                    typedef half4_t half4_a8_t __attribute__((aligned(8)));
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const half4_t h = *OVRFSR_AT(const half4_a8_t, src + 8 * j);
                        const float r = (float)h.x, g = (float)h.y, b = (float)h.z;
                        if (tmax) lmax = fmaxf(lmax, fmaxf(fabsf(r), fmaxf(fabsf(g), fabsf(b))));
                        stc(col, idx + j, r, g, b);
                        l[j] = b * 0.5f + (r * 0.5f + g);
                    }
                }
                *OVRFSR_AT(float4, lum + idx) = make_float4(l[0], l[1], l[2], l[3]);
            }
        }
    } else {
        // flat sweep over all PITCH x cellsH cells (pad columns load a clamped texel too: harmless, never read)
        for (int idx = threadIdx.x; idx < ncell; idx += NT) {
            const int cy = idx / PITCH, cx = idx - cy * PITCH;
            const int sy = clampi(tile_y0 + cy, 0, inH - 1);
            const int sx = clampi(tile_x0 + cx, 0, inW - 1);
            if constexpr (IN_FMT == ovrfsr::FMT_RGBA8) {
                const uint32_t off = (uint32_t)sy * pitchB + (uint32_t)sx * 4u; // images are < 4 GiB (16384^2 x 4 B)
                const uint32_t v = *OVRFSR_AT(const uint32_t, img + off);
                const float rb = (float)(v & 0xffu), gb = (float)((v >> 8) & 0xffu), bb = (float)((v >> 16) & 0xffu);
                stc(col, idx, rb, gb, bb);
                const float r = unorm8_to_unit(rb), g = unorm8_to_unit(gb), b = unorm8_to_unit(bb);
                lum[idx] = b * 0.5f + (r * 0.5f + g);
            } else if constexpr (IN_FMT == ovrfsr::FMT_RGBA8_MS4) {
                const uint32_t off = (uint32_t)sy * pitchB + (uint32_t)sx * 16u; // the multisampled image spans <= 4 GiB (CheckImage)
                const u32x4_a4_t q = *OVRFSR_AT(const u32x4_a4_t, img + off);
                const uint32_t s4[4] = {q[0], q[1], q[2], q[3]};
                const uint32_t v = resolve_unorm8<4>(s4);
                const float rb = (float)(v & 0xffu), gb = (float)((v >> 8) & 0xffu), bb = (float)((v >> 16) & 0xffu);
                stc(col, idx, rb, gb, bb);
                const float r = unorm8_to_unit(rb), g = unorm8_to_unit(gb), b = unorm8_to_unit(bb);
                lum[idx] = b * 0.5f + (r * 0.5f + g);
            } else if constexpr (IN_FMT == ovrfsr::FMT_R11G11B10F) {
                const uint32_t off = (uint32_t)sy * pitchB + (uint32_t)sx * 4u; // images span <= 4 GiB (CheckImage)
                float r, g, b;
                unpack_r11g11b10f(*OVRFSR_AT(const uint32_t, img + off), r, g, b);
                if (tmax) lmax = fmaxf(lmax, fmaxf(fabsf(r), fmaxf(fabsf(g), fabsf(b))));
                stc(col, idx, r, g, b);
                lum[idx] = b * 0.5f + (r * 0.5f + g);
            } else {
                const float4 c = load_unit<IN_FMT>(img, pitchB, sx, sy);
                if constexpr (kFloatSrc) { if (tmax) lmax = fmaxf(lmax, fmaxf(fabsf(c.x), fmaxf(fabsf(c.y), fabsf(c.z)))); }
                stc(col, idx, c.x, c.y, c.z);
                lum[idx] = c.z * 0.5f + (c.x * 0.5f + c.y);
            }
        }
    }
    __syncthreads();
    if constexpr (kFloatSrc) {
        // (behind the barrier: the caller's zero of *tmax is visible; published by the barrier that ends this function.)  |x| >= 0: the bit
        // patterns order like the values.  A NaN texel never gets here -- fmaxf drops NaN operands, so lmax is the largest FINITE-or-inf
        // channel -- and needs no band: every pixel its taps reach is NaN in both builds, whatever is listed
        if (tmax && lmax > 1.0f) atomicMax(tmax, __float_as_uint(lmax)); // unit-range footprints (the common case) issue no atomic
    }
    // analysis of rows 1..cellsH-2, every column; a lane owns 4 vertically adjacent cells.  Border columns take their missing
    // neighbour from the adjacent row, and the last group reads up to ovrfsr::kLumPadRows rows past the plane: finite-or-not garbage
    // that only reaches cells which are never an f/g/j/k texel, or results that are not stored.
    const int groups = (cellsH - 2 + 3) >> 2;
#pragma clang loop vectorize(disable) interleave(disable)
#pragma unroll 1
    for (int t = threadIdx.x; t < PITCH * groups; t += NT) {
        const int g = t / PITCH, cx = t - g * PITCH;
        const int row = 1 + 4 * g;
        const int idx = row * PITCH + cx;
        const int nrows = min(4, cellsH - 1 - row);
        float V[6], Lf[4], Rt[4];
#pragma unroll
        for (int i = 0; i < 6; ++i) V[i] = lum[idx + (i - 1) * PITCH];
#pragma unroll
        for (int j = 0; j < 4; ++j) { Lf[j] = lum[idx + j * PITCH - 1]; Rt[j] = lum[idx + j * PITCH + 1]; }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 an = easu_analyse(V[j], Lf[j], V[j + 1], Rt[j], V[j + 2]);
            if (j < nrows) ana[idx + j * PITCH] = an;
        }
    }
    __syncthreads();
}

// RGBA8 store of byte-domain RGB (already inside [min4,max4] of byte values), alpha = 255
__device__ __forceinline__ uint32_t pack_bytes_rne(float r, float g, float b)
{
    uint32_t v = 0xff000000u;
    v = __builtin_amdgcn_cvt_pk_u8_f32(r, 0, v);
    v = __builtin_amdgcn_cvt_pk_u8_f32(g, 1, v);
    v = __builtin_amdgcn_cvt_pk_u8_f32(b, 2, v);
    return v;
}

#ifdef OVRFSR_TIE_AUDIT
// Audit of one product-resolved pixel (see g_ovrfsr_tie_audit in fsr_kernels.hip).  (r, g, b): the product resolve's result in the domain it is
// stored from (bytes 0..255 for UNORM8 stores of RGBA8 input; unit domain for half stores); `listed`: the near-tie guard took the pixel.
// UNIT8: the UNORM8 store of a FLOAT source (unit domain, store_unit on both sides); xmin then carries the pixel's band in bytes, and the
// distance is recorded as a FRACTION OF THAT BAND in slot [5] (the band varies with the tile: a distance in bytes would not compare) --
// the campaign that audits such stores runs nothing else, so the slot is not shared with half spacings.
template <bool BYTES, bool HALF_STORE, bool UNIT8 = false>
__device__ __forceinline__ void tie_audit_px(OVRFSR_PTR_RC(float4) col, OVRFSR_PTR_RC(float4) ana, int base, int pitch, float ppx, float ppy,
                                             float r, float g, float b, bool listed, float xmin)
{
    float sr, sg, sb; // the strict build's value, unit domain
    easu_resolve<BYTES, float4>(col, ana, base, pitch, ppx, ppy, sr, sg, sb);
    bool flip = false, small = false;
    float dist = 0.0f;
    if constexpr (UNIT8) {
        const uint32_t pv = unit_to_unorm8(r) | (unit_to_unorm8(g) << 8) | (unit_to_unorm8(b) << 16);
        const uint32_t sv = unit_to_unorm8(sr) | (unit_to_unorm8(sg) << 8) | (unit_to_unorm8(sb) << 16);
        flip = pv != sv;
        // distance between the values as stored from: sat(x) * 255, in bands
        dist = fmaxf(fabsf(sat01(r) - sat01(sr)), fmaxf(fabsf(sat01(g) - sat01(sg)), fabsf(sat01(b) - sat01(sb)))) * 255.0f / xmin;
    } else if constexpr (!HALF_STORE) {
        // product: v_cvt_pk_u8_f32 of the byte-domain value; strict: floor(sat(x) * 255 + 0.5)
        const uint32_t pv = pack_bytes_rne(r, g, b);
        const uint32_t sv = unit_to_unorm8(sr) | (unit_to_unorm8(sg) << 8) | (unit_to_unorm8(sb) << 16) | 0xff000000u;
        flip = pv != sv;
        dist = fmaxf(fabsf(r - sr * 255.0f), fmaxf(fabsf(g - sg * 255.0f), fabsf(b - sb * 255.0f)));
    } else {
        const float p[3] = {r, g, b}, q[3] = {sr, sg, sb};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const half_t hp = (half_t)p[c], hq = (half_t)q[c];
            const bool differ = __builtin_bit_cast(unsigned short, hp) != __builtin_bit_cast(unsigned short, hq);
            const bool guarded = fmaxf(p[c], q[c]) >= xmin; // the contract covers channels >= xmin
            flip |= differ && guarded;
            small |= differ && !guarded;
            // distance in half spacings of the strict value's binade (2^-10 of the binade's base; subnormals: 2^-24)
            const float spacing = fmaxf(__uint_as_float((__float_as_uint(fabsf(q[c])) & 0x7f800000u)) * (1.0f / 1024.0f), 5.9604645e-8f);
            if (guarded) dist = fmaxf(dist, fabsf(p[c] - q[c]) / spacing); // (channels under xmin: tiny spacings, outside the contract)
        }
    }
    atomicAdd(&g_ovrfsr_tie_audit[0], 1ull);
    if (listed) atomicAdd(&g_ovrfsr_tie_audit[1], 1ull);
    if (flip && !listed) atomicAdd(&g_ovrfsr_tie_audit[2], 1ull);
    if (small && !listed) atomicAdd(&g_ovrfsr_tie_audit[3], 1ull);
    atomicMax(&g_ovrfsr_tie_audit[(HALF_STORE || UNIT8) ? 5 : 4], (unsigned long long)__float_as_uint(dist)); // dist >= 0: the bit pattern orders like the value
}
#endif

#include "fsr_outside.inc" // bilinear_column4, easu_outside_kernel, outside_staged_kernel

// MASKED = false: every 16x16 group of every image is inside the radius (radius 2.0 "mask off", or a radius that covers
// the frame): no mask test, no bilinear fallback, nothing of either hoisted into the prologue the 4 pixels of a thread share.
// (Round 5 measured 16-row tiles for small launches -- one eye image per call is 4.3 rounds of the 5 x 256 resident workgroups --: 41.3
// instead of 40.7 us per eye.  This kernel is VALU-bound: the CUs of the partly filled last round run their fewer workgroups faster,
// and half-height tiles stage 14 % more cells per pixel.  profiles/r05_frame.txt.)
template <int IN_FMT, int OUT_FMT, int PITCH, bool MASKED>
__global__ __launch_bounds__(256) void easu_fast_kernel(const ovrfsr::EasuArgs a)
{
    constexpr int TH = ovrfsr::kTileH;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    OVRFSR_LDS_POISON(smem, a.ldsBytes);
    // per output row of the tile: sub-texel position ppy and the LDS cell index of the row of its 'f' texel.  Both are the
    // same for the 32 pixels of a row: 32 lanes compute them once (9 VALU) instead of every pixel.
    OVRFSR_LDS_ARRAY(float2, rowinfo, TH, K_EASU_ROWINFO);
    constexpr bool byte_domain = IN_FMT == ovrfsr::FMT_RGBA8 || IN_FMT == ovrfsr::FMT_RGBA8_MS4; // (MS4: resolved to RGBA8 as it is staged)

    const uint32_t img_i = blockIdx.z;
    const uint32_t tile = a.tileList ? OVRFSR_TILE_LIST(a)[blockIdx.x] : xcd_tile_index(blockIdx.x, a.tilesX * a.tilesY);
    uint32_t tileX, tileY;
    tile_xy(tile, a.tilesX, a.tilesXMagic, tileX, tileY);
    OVRFSR_IMAGES(IN_FMT, OUT_FMT);

    uint32_t inside_bits = 0xfu;
    if constexpr (MASKED) inside_bits = tile_mask_bits(a.m, (a.m.first_eye ^ (img_i & a.m.alternate)) & 1u, tileX, tileY);
    const int ox0 = (int)tileX * ovrfsr::kTileW, oy0 = (int)tileY * TH;
    const int l5 = threadIdx.x & 31, ly0 = threadIdx.x >> 5;
    // conflict-free ds_read_b128 groups; only with 4-byte output texels, where a row of 32 pixels is one 128-byte line in any
    // lane order (wider texels: the permuted 16-lane store groups would straddle lines)
    const int lx = TexelBytes<OUT_FMT>::v == 4 ? lane32_to_pos(l5) : l5;
    const int ox = ox0 + lx;
    const int tile_x0 = (int)floorf(mad_unfused((float)ox0, a.sx, a.cx)) - 1;
    const int tile_y0 = (int)floorf(mad_unfused((float)oy0, a.sy, a.cy)) - 1;

    const int ncell = PITCH * a.cellsH;
    OVRFSR_PTR(float4) col = OVRFSR_CARVE(float4, reinterpret_cast<float4 *>(smem), ncell, 0, K_EASU_COL, smem, a.ldsBytes);
    OVRFSR_PTR(float4) ana = OVRFSR_CARVE(float4, OVRFSR_RAW(col) + ncell, ncell, 0, K_EASU_ANA, smem, a.ldsBytes);
    OVRFSR_PTR(float) lum = OVRFSR_CARVE(float, reinterpret_cast<float *>(OVRFSR_RAW(ana) + ncell), ncell, PITCH * ovrfsr::kLumPadRows, K_EASU_LUM, smem, a.ldsBytes);

    // which stores the near-tie guard (below) covers
    constexpr bool kGuardU8 = byte_domain && OUT_FMT == ovrfsr::FMT_RGBA8, kGuardH = OUT_FMT == ovrfsr::FMT_RGBA16F;
    // UNORM8 stores of float sources (cfg.reference_formats): guarded in the unit domain (near_tie_unorm8_unit), and only where the host
    // switches the guard on -- a.tieHalfMin, which this instantiation has no other use for: +inf = off (the stores of every earlier
    // release, bit for bit), finite = on
    constexpr bool kGuardF8 = !byte_domain && OUT_FMT == ovrfsr::FMT_RGBA8;
    constexpr bool kGuard = kGuardU8 || kGuardH || kGuardF8;
    // half and UNORM8 stores of float sources: the largest |channel| of the staged footprint (HDR tiles widen the guard's band, near_tie_half3_hdr)
    constexpr bool kTmax = (kGuardH || kGuardF8) && !byte_domain;
    __shared__ uint32_t tile_tmax;

    if (inside_bits != 0u) {
        if (threadIdx.x < (unsigned)TH) {
            const float ppy_raw = mad_unfused((float)(oy0 + (int)threadIdx.x), a.sy, a.cy);
            const float fpy = floorf(ppy_raw);
            rowinfo[threadIdx.x] = make_float2(ppy_raw - fpy, __int_as_float(((int)fpy - tile_y0) * PITCH));
        }
        if (kTmax && threadIdx.x == 0) tile_tmax = 0u;
        easu_stage_fast<IN_FMT, PITCH>(in, a.v.in_pitch, a.v.inW, a.v.inH, tile_x0, tile_y0, a.cellsH, col, lum, ana, kTmax ? &tile_tmax : nullptr);
    }
    // (workgroup-uniform: one LDS read into an SGPR; meaningful only where something was staged -- elsewhere the word is uninitialised and unused)
    [[maybe_unused]] const float tmax_v = kTmax ? __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)tile_tmax)) : 1.0f;
    // (kGuardF8: the band in bytes, workgroup-uniform; 0 = guard off.  A band of half a byte or more -- tmax >= 256 -- lists every pixel
    // of the tile: a wave's list holds all of its 256 pixels, and the one-lane-per-pixel pass below then resolves the whole tile in reference order)
    [[maybe_unused]] const float band_f8 = (kGuardF8 && a.tieHalfMin < __builtin_inff()) ? (1.0f / (float)(1 << kTieBits)) * fmaxf(tmax_v, 1.0f) : 0.0f;

    // Near-tie guard.  The re-associated resolve differs from the reference-order one by rounding noise (<= 6.5e-4 of a
    // byte measured over 1e8 values, adversarial content included: profiles/r03_easu_err.txt); where its result lies that
    // close to k + 0.5 the UNORM8 store could round the other way, and RCAS amplifies such a flipped intermediate byte up to
    // 4x.  A pixel with a channel within 2^-TIE_BITS of a boundary (2^(1-TIE_BITS) of the values: ~1.2 % of the pixels at
    // the default 9) is not stored; it is listed in LDS -- per wave, ranked with mbcnt, no atomics -- and after the pixel
    // loop the workgroup re-resolves its list in the reference's operator order from the same LDS planes (the luma and
    // analysis planes are rounding-identical to the strict build's; bytes are decoded b/255), one lane per listed pixel.
    // The stored image is then bit-identical to the strict build's / the oracle's.
    // (Measured alternative, profiles/r03_guard_variants.txt: recording the pixels in global memory and re-resolving them
    // densely in a second kernel.  Its 12-texel gathers -- one unrelated address per lane -- run at 12 G pixels/s whatever
    // the load width or the batch grouping: 0.16-0.19 ms per 32 eyes against 0.12 ms for this in-kernel pass.)
    // RGBA16F destinations (the half intermediate of a half-float pipeline) are guarded the same way, on the half rounding
    // boundaries of the values large enough for a flipped half-ulp to matter behind RCAS (near_tie_half3).
    OVRFSR_LDS_ARRAY(uint16_t, tie_list, (kGuard ? 4 * 256 : 4), K_TIE_LIST);
    OVRFSR_LDS_ARRAY(uint32_t, tie_cnt, 4, K_TIE_CNT);
    [[maybe_unused]] const uint32_t wave = threadIdx.x >> 6;
    [[maybe_unused]] uint32_t tie_n = 0; // wave-uniform: near-tie pixels this wave has listed

    const bool active = ox < a.v.outW;
    if constexpr (MASKED) {
        if (inside_bits == 0u) { // workgroup-uniform: nothing staged
            if (a.ringStrips) {
                // Ring tile of the mask-sorted form (an outside tile 4-adjacent to a tile touching the radius; its final
                // pixels come from the outside-tile kernel).  This intermediate is read by nothing but the b/d/f/h taps of
                // RCAS in the inside neighbours, which reach ONE pixel across the tile edge: write, per 16-pixel half edge
                // whose neighbouring group is inside the radius, that line of pixels -- at most 124 of the 1024.
                // (Rounds 1-3 wrote the whole tile: 7-11 us per 16 eyes at C2r, 3 % of the step.)
                if (threadIdx.x < 128u) {
                    const uint32_t eye = (a.m.first_eye ^ (img_i & a.m.alternate)) & 1u;
                    const int e = (int)(threadIdx.x >> 5), i = (int)(threadIdx.x & 31u); // e: left / right column, top / bottom row
                    const int px = e == 0 ? 0 : e == 1 ? ovrfsr::kTileW - 1 : i, py = e == 2 ? 0 : e == 3 ? ovrfsr::kTileH - 1 : i;
                    const int gx = 2 * (int)tileX + (e == 0 ? -1 : e == 1 ? 2 : (i >> 4)), gy = 2 * (int)tileY + (e == 2 ? -1 : e == 3 ? 2 : (i >> 4));
                    const int x = ox0 + px, y = oy0 + py;
                    if (gx >= 0 && gy >= 0 && x < a.v.outW && y < a.v.outH && group_inside((uint32_t)gx, (uint32_t)gy, a.m.centre[eye], a.m.r2)) {
                        const float4 c = bilinear_global<IN_FMT>(in, a.v.in_pitch, a.v.inW, a.v.inH, x, y, (float)a.v.outW, (float)a.v.outH);
                        store_unit<OUT_FMT>(out, a.v.out_pitch, x, y, c.x, c.y, c.z, 1.0f);
                    }
                }
                return;
            }
            if (active) {
                const ovrfsr::BilinTap tx = OVRFSR_BIL_X(a)[ox];
                bilinear_column4<IN_FMT, OUT_FMT>(in, out, a, ox, oy0 + ly0, clampi(tx.i0, 0, a.v.inW - 1), clampi(tx.i0 + 1, 0, a.v.inW - 1), tx.frac);
            }
            return;
        }
    }
    const float ppx_raw = mad_unfused((float)ox, a.sx, a.cx);
    const float fpx = floorf(ppx_raw);
    const float ppx = ppx_raw - fpx;
    const int cellx = (int)fpx - tile_x0;

    // stores the resolved pixel (lx, ly) of the tile, unless it is a near-tie (returns true: the caller lists it)
    auto put_px = [&](int ly, float r, float g, float b) -> bool {
        const int oy = oy0 + ly;
        if constexpr (byte_domain && OUT_FMT == ovrfsr::FMT_RGBA8) {
            if (kGuardU8 && ((int)near_tie_byte(r) | (int)near_tie_byte(g) | (int)near_tie_byte(b))) return true;
            // an RGBA8 image spans < 4 GiB (CheckImage): 32-bit byte offset from the uniform image base
            *OVRFSR_AT(uint32_t, out + ((uint32_t)oy * a.v.out_pitch + (uint32_t)ox * 4u)) = pack_bytes_rne(r, g, b);
        } else if constexpr (kGuardH) {
            if constexpr (byte_domain) { const float s = 1.0f / 255.0f; r *= s; g *= s; b *= s; }
            const half4_t h = {(half_t)r, (half_t)g, (half_t)b, (half_t)1.0f};
            if (near_tie_half3_hdr(r, g, b, a.tieHalfMin, tmax_v)) return true;
            *OVRFSR_AT(half4_t, out + (size_t)oy * a.v.out_pitch + (size_t)ox * 8) = h;
        } else if constexpr (kGuardF8) {
            if (near_tie_unorm8_unit3(r, g, b, band_f8)) return true;
            store_unit<OUT_FMT>(out, a.v.out_pitch, ox, oy, r, g, b, 1.0f);
        } else if constexpr (byte_domain) {
            const float s = 1.0f / 255.0f;
            store_unit<OUT_FMT>(out, a.v.out_pitch, ox, oy, r * s, g * s, b * s, 1.0f);
        } else {
            store_unit<OUT_FMT>(out, a.v.out_pitch, ox, oy, r, g, b, 1.0f);
        }
        return false;
    };
    // Resolves the vertically adjacent pixels (lx, ly) and (lx, ly + 1), ly even, of the tile.  Whether their footprints
    // coincide or B's sits one cell row lower depends on the row pair only; a wave covers two row pairs, and the shared
    // forms are taken when every lane agrees (always at scale 3/4, where every even-aligned pair has DIFF = 1).
    auto easu_pair = [&](int ly, bool &tieA, bool &tieB) {
        tieA = tieB = false;
        if (!active) return;
        const float2 riA = rowinfo[ly], riB = rowinfo[ly + 1];
        const int base = __float_as_int(riA.y) + cellx, drow = __float_as_int(riB.y) - __float_as_int(riA.y);
        float r0, g0, b0, r1, g1, b1;
        const bool all1 = __builtin_amdgcn_ballot_w64(drow != PITCH) == 0, all0 = __builtin_amdgcn_ballot_w64(drow != 0) == 0;
        if (all1) {
            easu_resolve_fast2<PITCH, 1>(col, ana, base, ppx, riA.x, riB.x, r0, g0, b0, r1, g1, b1);
        } else if (all0) {
            easu_resolve_fast2<PITCH, 0>(col, ana, base, ppx, riA.x, riB.x, r0, g0, b0, r1, g1, b1);
        } else {
            easu_resolve_fast<PITCH>(col, ana, base, ppx, riA.x, r0, g0, b0);
            easu_resolve_fast<PITCH>(col, ana, base + drow, ppx, riB.x, r1, g1, b1);
        }
        tieA = put_px(ly, r0, g0, b0);
        if (oy0 + ly + 1 < a.v.outH) tieB = put_px(ly + 1, r1, g1, b1);
#ifdef OVRFSR_TIE_AUDIT
        if constexpr (kGuardF8) { // audited where the guard is on (off: the unguarded stores of earlier releases, no contract)
            if (band_f8 > 0.0f) {
                tie_audit_px<false, false, true>(col, ana, base, PITCH, ppx, riA.x, r0, g0, b0, tieA, band_f8);
                if (oy0 + ly + 1 < a.v.outH) tie_audit_px<false, false, true>(col, ana, base + drow, PITCH, ppx, riB.x, r1, g1, b1, tieB, band_f8);
            }
        } else if constexpr (kGuard) {
            constexpr float us = (byte_domain && kGuardH) ? 1.0f / 255.0f : 1.0f; // put_px brings byte-domain results to the unit domain before a half store
            tie_audit_px<byte_domain, kGuardH>(col, ana, base, PITCH, ppx, riA.x, r0 * us, g0 * us, b0 * us, tieA, a.tieHalfMin);
            if (oy0 + ly + 1 < a.v.outH) tie_audit_px<byte_domain, kGuardH>(col, ana, base + drow, PITCH, ppx, riB.x, r1 * us, g1 * us, b1 * us, tieB, a.tieHalfMin);
        }
#endif
    };
    // called by the whole wave (converged): list the lanes whose pixel of row ly is a near-tie
    auto tie_append = [&](bool tie, int ly) {
        if constexpr (kGuard) {
            const uint64_t m = __builtin_amdgcn_ballot_w64(tie);
            if (tie) {
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                tie_list[wave * 256u + tie_n + rank] = (uint16_t)((ly << 5) | lx);
            }
            tie_n += (uint32_t)__builtin_popcountll(m);
        }
    };

    if (inside_bits == 0xfu) {
        // the common case gets its own loop: otherwise the compiler hoists the bilinear fallback's x-dependent
        // setup (the tap-table load, clamps, 64-bit addressing: ~45 VALU) above the loop
#pragma unroll 1
        for (int k = 0; k < TH / 16; ++k) {
            const int ly = 2 * ly0 + 16 * k; // this thread's rows: (ly, ly + 1), even-aligned, inside one 16-row mask group
            if (oy0 + ly >= a.v.outH) break;
            bool tieA, tieB;
            easu_pair(ly, tieA, tieB);
            tie_append(tieA, ly);
            tie_append(tieB, ly + 1);
        }
    } else if constexpr (MASKED) {
        const uint32_t gbit_x = (uint32_t)(lx >> 4);
        const ovrfsr::BilinTap tx = OVRFSR_BIL_X(a)[active ? ox : 0];
        const float bfx = tx.frac;
#pragma unroll 1
        for (int k = 0; k < 2; ++k) {
            const int ly = 2 * ly0 + 16 * k;
            if (oy0 + ly >= a.v.outH) break;
            const bool inside = (inside_bits >> (gbit_x + 2u * (uint32_t)(ly >> 4))) & 1u;
            bool tieA = false, tieB = false;
            if (inside) {
                easu_pair(ly, tieA, tieB);
            } else if (active) {
                // bilinear fallback of the groups outside the radius in a tile that touches it: taps from the host-built
                // column/row tables, texels from the LDS colour plane -- the fallback samples at pos/outSize, half an output
                // pixel left/up of EASU's mapping, so its 2x2 footprint lies inside the staged one (clamp addressing was
                // resolved at staging time); the bytes are decoded b/255 and blended unfused exactly as bilinear_uv does.
                // (Rounds 1-2 fetched the four texels from global memory per pixel: such tiles cost twice a full-EASU tile.)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int oy = oy0 + ly + j;
                    if (oy >= a.v.outH) break;
                    const ovrfsr::BilinTap ty = OVRFSR_BIL_Y(a)[oy];
                    const OVRFSR_PTR(float4) cp = col + (ty.i0 - tile_y0) * PITCH + (tx.i0 - tile_x0);
                    float4 c00 = cp[0], c10 = cp[1], c01 = cp[PITCH], c11 = cp[PITCH + 1];
                    if constexpr (byte_domain) {
                        auto dec = [](float4 &c) { c.x = unorm8_to_unit(c.x); c.y = unorm8_to_unit(c.y); c.z = unorm8_to_unit(c.z); };
                        dec(c00); dec(c10); dec(c01); dec(c11);
                    }
                    const float fy = ty.frac;
                    const float w00 = (1.0f - bfx) * (1.0f - fy), w10 = bfx * (1.0f - fy), w01 = (1.0f - bfx) * fy, w11 = bfx * fy;
                    store_unit<OUT_FMT>(out, a.v.out_pitch, ox, oy, bilerp_unfused(c00.x, c10.x, c01.x, c11.x, w00, w10, w01, w11),
                                        bilerp_unfused(c00.y, c10.y, c01.y, c11.y, w00, w10, w01, w11),
                                        bilerp_unfused(c00.z, c10.z, c01.z, c11.z, w00, w10, w01, w11), 1.0f);
                }
            }
            tie_append(tieA, ly);
            tie_append(tieB, ly + 1);
        }
    }
    if constexpr (kGuard) {
        if ((threadIdx.x & 63u) == 0u) tie_cnt[wave] = tie_n;
        __syncthreads();
        const uint32_t n0 = tie_cnt[0], n1 = tie_cnt[1], n2 = tie_cnt[2], total = n0 + n1 + n2 + tie_cnt[3];
        // The wave that takes the first entries rotates with the tile so that the pass does not always land on the same SIMD.
        const uint32_t rot = (threadIdx.x + 64u * (tile & 3u)) & 255u;
        auto entry = [&](uint32_t t, int &fox, int &foy, int &base, float &fppx, float &fppy) {
            uint32_t w = 0, off = t;
            if (off >= n0) { off -= n0; w = 1; if (off >= n1) { off -= n1; w = 2; if (off >= n2) { off -= n2; w = 3; } } }
            const uint32_t e = tie_list[w * 256u + off];
            const int fly = (int)(e >> 5);
            fox = ox0 + (int)(e & 31u); foy = oy0 + fly;
            const float px_raw = mad_unfused((float)fox, a.sx, a.cx);
            const float px_f = floorf(px_raw);
            const float2 ri = rowinfo[fly];
            base = __float_as_int(ri.y) + ((int)px_f - tile_x0); fppx = px_raw - px_f; fppy = ri.x;
        };
        if (total <= 32u) { // workgroup-uniform
            // the usual case (a dozen pixels): four lanes per listed pixel (easu_resolve_quad), 16 pixels per wave -- 253
            // instructions for the tile instead of 515 with one lane per pixel and 50 lanes idle (C2 +3 %)
            const int q = (int)(threadIdx.x & 3u);
#pragma unroll 1
            for (uint32_t t = rot >> 2; t < total; t += 64u) {
                int fox, foy, base; float fppx, fppy;
                entry(t, fox, foy, base, fppx, fppy);
                const float v = easu_resolve_quad<byte_domain>(col, ana, base, PITCH, fppx, fppy, q);
                // lane c holds channel c; lane 0 collects G and B and writes the texel exactly as the strict build's store_unit does
                if constexpr (OUT_FMT == ovrfsr::FMT_RGBA8) {
                    const uint32_t me = unit_to_unorm8(v);
                    const uint32_t g8 = (uint32_t)__builtin_amdgcn_mov_dpp((int)me, 1 * 0x55, 0xf, 0xf, true), b8 = (uint32_t)__builtin_amdgcn_mov_dpp((int)me, 2 * 0x55, 0xf, 0xf, true);
                    if (q == 0) *OVRFSR_AT(uint32_t, out + ((uint32_t)foy * a.v.out_pitch + (uint32_t)fox * 4u)) = me | (g8 << 8) | (b8 << 16) | 0xff000000u;
                } else {
                    const float g = quad_bcast<1>(v), b = quad_bcast<2>(v);
                    if (q == 0) store_unit<OUT_FMT>(out, a.v.out_pitch, fox, foy, v, g, b, 1.0f);
                }
            }
        } else {
            // many near-ties (dense content): one lane per listed pixel keeps the lanes full
#pragma unroll 1
            for (uint32_t t = rot; t < total; t += 256u) {
                int fox, foy, base; float fppx, fppy, r, g, b;
                entry(t, fox, foy, base, fppx, fppy);
                easu_resolve<byte_domain, float4>(col, ana, base, PITCH, fppx, fppy, r, g, b);
                store_unit<OUT_FMT>(out, a.v.out_pitch, fox, foy, r, g, b, 1.0f); // the strict build's store: UNORM8 floor(x*255+0.5) / half RNE
            }
        }
    }
}
#endif // !OVRFSR_STRICT

// ------------------------------------------------------------------------------------------------
// RCAS
// ------------------------------------------------------------------------------------------------

// FsrRcasF, fsr/ffx_fsr1.h:684-769, on unit-domain taps (FSR_RCAS_DENOISE undefined: the nz term is dead)
__device__ __forceinline__ void rcas_resolve(const float4 &b, const float4 &d, const float4 &e, const float4 &f, const float4 &h,
                                             float sharp, float &pr, float &pg, float &pb)
{
    float mn4R = fminf(fminf(b.x, fminf(d.x, f.x)), h.x), mx4R = fmaxf(fmaxf(b.x, fmaxf(d.x, f.x)), h.x);
    float mn4G = fminf(fminf(b.y, fminf(d.y, f.y)), h.y), mx4G = fmaxf(fmaxf(b.y, fmaxf(d.y, f.y)), h.y);
    float mn4B = fminf(fminf(b.z, fminf(d.z, f.z)), h.z), mx4B = fmaxf(fmaxf(b.z, fmaxf(d.z, f.z)), h.z);
    float hitMinR = mn4R * rcp_f(4.0f * mx4R), hitMinG = mn4G * rcp_f(4.0f * mx4G), hitMinB = mn4B * rcp_f(4.0f * mx4B);
    float hitMaxR = (1.0f - mx4R) * rcp_f(4.0f * mn4R + -4.0f);
    float hitMaxG = (1.0f - mx4G) * rcp_f(4.0f * mn4G + -4.0f);
    float hitMaxB = (1.0f - mx4B) * rcp_f(4.0f * mn4B + -4.0f);
    float lobeR = fmaxf(-hitMinR, hitMaxR), lobeG = fmaxf(-hitMinG, hitMaxG), lobeB = fmaxf(-hitMinB, hitMaxB);
    float lobe = fmaxf(-OVRFSR_RCAS_LIMIT, fminf(fmaxf(lobeR, fmaxf(lobeG, lobeB)), 0.0f)) * sharp;
    float rcpL = prx_med_rcp(4.0f * lobe + 1.0f);
    pr = (lobe * b.x + lobe * d.x + lobe * h.x + lobe * f.x + e.x) * rcpL;
    pg = (lobe * b.y + lobe * d.y + lobe * h.y + lobe * f.y + e.y) * rcpL;
    pb = (lobe * b.z + lobe * d.z + lobe * h.z + lobe * f.z + e.z) * rcpL;
}

// RCAS pass: grid = (tilesX*tilesY, 1, batch), block = 256, 32x32 tile + 1-texel ring in LDS
// (float4, unit domain; Texture2D.Load semantics: out-of-image taps read 0).
template <int IN_FMT, int OUT_FMT>
__global__ __launch_bounds__(256) void rcas_kernel(const ovrfsr::RcasArgs a)
{
    constexpr int LW = ovrfsr::kTileW + 2, LH = ovrfsr::kTileH + 2;
    OVRFSR_LDS_ARRAY(float4, tile_px, LW * LH, K_RCAS_TILE);

    const uint32_t img_i = blockIdx.z;
    const uint32_t eye = (a.m.first_eye ^ (img_i & a.m.alternate)) & 1u;
    const uint32_t tile = xcd_tile_index(blockIdx.x, a.tilesX * a.tilesY);
    uint32_t tileX, tileY;
    tile_xy(tile, a.tilesX, a.tilesXMagic, tileX, tileY);
    OVRFSR_IMAGES(IN_FMT, OUT_FMT);
    const int W = a.v.outW, H = a.v.outH;

    const uint32_t inside_bits = tile_mask_bits(a.m, eye, tileX, tileY);
    const int ox0 = (int)tileX * ovrfsr::kTileW, oy0 = (int)tileY * ovrfsr::kTileH;

    if (inside_bits != 0u) {
        for (int i = threadIdx.x; i < LW * LH; i += ovrfsr::kThreads) {
            int cy = i / LW, cx = i - cy * LW;
            int sx = ox0 - 1 + cx, sy = oy0 - 1 + cy;
            float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (sx >= 0 && sy >= 0 && sx < W && sy < H) c = load_unit<IN_FMT>(in, a.v.in_pitch, sx, sy);
            tile_px[i] = c;
        }
        __syncthreads();
    }

    const int lx = threadIdx.x & 31, ly0 = threadIdx.x >> 5;
    const int ox = ox0 + lx;
    if (ox >= W) return;
    const uint32_t gbit_x = (uint32_t)(lx >> 4);
    const float dbg = (float)a.debug;
    const float mulG = 1.0f - dbg * 0.3f; // fsr_rcas.hlsl:46: mul = 1 - debug*(0,.3,.3,0)
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const int ly = ly0 + 8 * k;
        const int oy = oy0 + ly;
        if (oy >= H) break;
        const bool inside = (inside_bits >> (gbit_x + 2u * (uint32_t)(ly >> 4))) & 1u;
        if (inside) {
            const int c = (ly + 1) * LW + (lx + 1);
            float r, g, b;
            rcas_resolve(tile_px[c - LW], tile_px[c - 1], tile_px[c], tile_px[c + 1], tile_px[c + LW], a.sharp, r, g, b);
            store_unit<OUT_FMT>(out, a.v.out_pitch, ox, oy, r, g, b, 1.0f);
        } else {
            float4 s = load_unit<IN_FMT>(in, a.v.in_pitch, ox, oy);
            store_unit<OUT_FMT>(out, a.v.out_pitch, ox, oy, s.x * (1.0f - dbg * 0.0f), s.y * mulG, s.z * mulG, s.w * (1.0f - dbg * 0.0f));
        }
    }
}


#if !OVRFSR_STRICT
// ------------------------------------------------------------------------------------------------
// RCAS, product build, without LDS.  FsrRcasF is homogeneous of degree 1 in the colour scale once the peak
// constant follows the scale: with taps in the 0..255 byte domain hitMin = mn/(4mx) is unchanged and
// hitMax = (255-mx)/(4mn-1020); lobe is dimensionless; pix comes out in bytes.  So an RGBA8 source is unpacked
// with one v_cvt_f32_ubyteN per channel (no b/255) and the result packed with v_cvt_pk_u8_f32 (clamps like the
// UNORM store; RNE instead of floor(x+.5): exact ties only).  PEAK = 255 for RGBA8 input, 1 otherwise.
// A thread resolves 4 vertically adjacent pixels of one column: the 6
// centre-column texels and the 4+4 left/right texels are loaded from L1/L2 once each and unpacked once
// (14 loads, 42 v_cvt per 4 pixels) -- versus a staging pass (4.5 texels per thread through LDS with bounds
// tests, integer division and a barrier) plus 20 LDS reads.  Lanes of a half-wave cover 32 consecutive x, so
// every load instruction is two 128-byte row segments.  Taps outside the image read 0 (Texture2D.Load): only
// workgroups that touch the image border take the predicated path.
// ------------------------------------------------------------------------------------------------
template <int IN_FMT, bool CHECKED>
__device__ __forceinline__ float4 rcas_tap(OVRFSR_PTR_R(const uint8_t) in, uint32_t pitch, int x, int y, int W, int H)
{
    if constexpr (CHECKED) {
        if ((unsigned)x >= (unsigned)W || (unsigned)y >= (unsigned)H) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    if constexpr (IN_FMT == ovrfsr::FMT_RGBA8) {
        const uint32_t v = *OVRFSR_AT(const uint32_t, in + (uint32_t)y * pitch + (uint32_t)x * 4u);
        return make_float4((float)(v & 0xffu), (float)((v >> 8) & 0xffu), (float)((v >> 16) & 0xffu), 0.0f);
    } else {
        return load_unit<IN_FMT>(in, pitch, x, y);
    }
}

// FsrRcasF on taps in the domain PEAK (255: bytes of an RGBA8 source, 1: unit) -- see the block comment above
template <bool BYTES>
__device__ __forceinline__ void rcas_resolve_bytes(const float4 &b, const float4 &d, const float4 &e, const float4 &f, const float4 &h,
                                                   float sharp, float &pr, float &pg, float &pb)
{
    constexpr float PEAK = BYTES ? 255.0f : 1.0f;
    const float mnR = raw_min(raw_min3(b.x, d.x, f.x), h.x), mxR = raw_max(raw_max3(b.x, d.x, f.x), h.x);
    const float mnG = raw_min(raw_min3(b.y, d.y, f.y), h.y), mxG = raw_max(raw_max3(b.y, d.y, f.y), h.y);
    const float mnB = raw_min(raw_min3(b.z, d.z, f.z), h.z), mxB = raw_max(raw_max3(b.z, d.z, f.z), h.z);
    float lobe;
    if constexpr (BYTES) {
        lobe = rcas_lobe_bytes(mnR, mxR, mnG, mxG, mnB, mxB, sharp); // one quotient per channel: exact on integers 0..255 only
    } else {
        const float hitMinR = mnR * __builtin_amdgcn_rcpf(4.0f * mxR);
        const float hitMinG = mnG * __builtin_amdgcn_rcpf(4.0f * mxG);
        const float hitMinB = mnB * __builtin_amdgcn_rcpf(4.0f * mxB);
        const float hitMaxR = (PEAK - mxR) * __builtin_amdgcn_rcpf(4.0f * mnR + -4.0f * PEAK);
        const float hitMaxG = (PEAK - mxG) * __builtin_amdgcn_rcpf(4.0f * mnG + -4.0f * PEAK);
        const float hitMaxB = (PEAK - mxB) * __builtin_amdgcn_rcpf(4.0f * mnB + -4.0f * PEAK);
        const float lobeR = fmaxf(-hitMinR, hitMaxR), lobeG = fmaxf(-hitMinG, hitMaxG), lobeB = fmaxf(-hitMinB, hitMaxB);
        lobe = __builtin_amdgcn_fmed3f(fmaxf(lobeR, fmaxf(lobeG, lobeB)), -OVRFSR_RCAS_LIMIT, 0.0f) * sharp;
    }
    const float rcpL = prx_med_rcp(4.0f * lobe + 1.0f);
    pr = (lobe * ((b.x + d.x) + (h.x + f.x)) + e.x) * rcpL;
    pg = (lobe * ((b.y + d.y) + (h.y + f.y)) + e.y) * rcpL;
    pb = (lobe * ((b.z + d.z) + (h.z + f.z)) + e.z) * rcpL;
}

// ------------------------------------------------------------------------------------------------
// Exact stores (OVRFSR_PRECISION_FP32_EXACT): the RGBA8 -> RGBA8 instances of the two kernels below with a near-tie guard on the FINAL
// byte, as easu_fast_kernel has one on the intermediate byte.  The product arithmetic above (one quotient per channel, v_rcp_f32, contracted
// sums, the byte domain, RNE pack) differs from the reference-order evaluation by 1.4e-4 byte at most (measured); a pixel with a channel within
// 2^-kRcasTieBits byte of a rounding boundary k + 1/2 is evaluated a second time exactly as ovrfsr_strict::rcas_kernel evaluates it and
// stored through unit_to_unorm8 (floor(x * 255 + 1/2): exact ties, which RNE rounds the other way half of the time, are inside the band).
// Every other pixel keeps the product value, whose byte is then the strict build's.  The band and the measurement behind it:
// profiles/exact_stores.txt (audit build, tools/debug/tie_audit.py --rcas).
//   Shape: a per-lane branch.  The taps of the pixel are live in registers where the test runs, and the kernels have no LDS to compact a
// list through.  0.3 % of the pixels of uniform-random content are listed, so one wave-row in six runs the second evaluation for all 64
// lanes: the guarded RCAS launch takes 14.0 instead of 10.2 us per eye at C2's size, a C2 step 8.5 % more (profiles/exact_stores.txt).
// rcas_dpp_kernel's neighbour-lane moves sit in front of the branch, where every lane is active.
// ------------------------------------------------------------------------------------------------
// Measured (audit build, tools/debug/tie_audit.py --rcas 1.0: 1.96e9 pixels, structured / uniform-random / natural / tie-rich content, sharpness
// 0 .. 1, every kernel form): largest |product - reference-order| 1.373e-4 byte; 3 x that = 4.12e-4 <= 2^-11 = 4.88e-4 byte.
constexpr int kRcasTieBits = 11;
// FsrRcasF in the reference's operator order on the byte taps of an RGBA8 source: what ovrfsr_strict::rcas_kernel computes (rcas_resolve
// with OVRFSR_STRICT's rcp_f, behind load_unit), restated here because this namespace's helpers are contracted: b/255 decode, both
// quotients per channel, unit domain, IEEE division, every operator rounded on its own.  Unit-domain result.
__device__ __forceinline__ void rcas_resolve_ref(const float4 &bB, const float4 &dB, const float4 &eB, const float4 &fB, const float4 &hB,
                                                 float sharp, float &pr, float &pg, float &pb)
{
#pragma clang fp contract(off)
    const float bx = unorm8_to_unit(bB.x), by = unorm8_to_unit(bB.y), bz = unorm8_to_unit(bB.z);
    const float dx = unorm8_to_unit(dB.x), dy = unorm8_to_unit(dB.y), dz = unorm8_to_unit(dB.z);
    const float ex = unorm8_to_unit(eB.x), ey = unorm8_to_unit(eB.y), ez = unorm8_to_unit(eB.z);
    const float fx = unorm8_to_unit(fB.x), fy = unorm8_to_unit(fB.y), fz = unorm8_to_unit(fB.z);
    const float hx = unorm8_to_unit(hB.x), hy = unorm8_to_unit(hB.y), hz = unorm8_to_unit(hB.z);
    const float mn4R = fminf(fminf(bx, fminf(dx, fx)), hx), mx4R = fmaxf(fmaxf(bx, fmaxf(dx, fx)), hx);
    const float mn4G = fminf(fminf(by, fminf(dy, fy)), hy), mx4G = fmaxf(fmaxf(by, fmaxf(dy, fy)), hy);
    const float mn4B = fminf(fminf(bz, fminf(dz, fz)), hz), mx4B = fmaxf(fmaxf(bz, fmaxf(dz, fz)), hz);
    const float hitMinR = mn4R * (1.0f / (4.0f * mx4R)), hitMinG = mn4G * (1.0f / (4.0f * mx4G)), hitMinB = mn4B * (1.0f / (4.0f * mx4B));
    const float hitMaxR = (1.0f - mx4R) * (1.0f / (4.0f * mn4R + -4.0f));
    const float hitMaxG = (1.0f - mx4G) * (1.0f / (4.0f * mn4G + -4.0f));
    const float hitMaxB = (1.0f - mx4B) * (1.0f / (4.0f * mn4B + -4.0f));
    const float lobeR = fmaxf(-hitMinR, hitMaxR), lobeG = fmaxf(-hitMinG, hitMaxG), lobeB = fmaxf(-hitMinB, hitMaxB);
    const float lobe = fmaxf(-OVRFSR_RCAS_LIMIT, fminf(fmaxf(lobeR, fmaxf(lobeG, lobeB)), 0.0f)) * sharp;
    const float ra = 4.0f * lobe + 1.0f;
    const float rb = __uint_as_float(0x7ef19fffu - __float_as_uint(ra)); // prx_med_rcp, unfused
    const float rcpL = rb * (-rb * ra + 2.0f);
    pr = (lobe * bx + lobe * dx + lobe * hx + lobe * fx + ex) * rcpL;
    pg = (lobe * by + lobe * dy + lobe * hy + lobe * fy + ey) * rcpL;
    pb = (lobe * bz + lobe * dz + lobe * hz + lobe * fz + ez) * rcpL;
    __asm__ volatile("" : "+v"(pr), "+v"(pg), "+v"(pb)); // round to fp32 here: nothing of the store folds into the products (store_unit)
}

// The RGBA8 word an exact-stores instance writes for a pixel whose product resolve gave (pr, pg, pb) in bytes.  `counted` (audit build):
// the pixel is stored, so it counts.
__device__ __forceinline__ uint32_t rcas_exact_bytes(const float4 &b, const float4 &d, const float4 &e, const float4 &f, const float4 &h,
                                                     float sharp, float pr, float pg, float pb, [[maybe_unused]] bool counted)
{
    uint32_t v = pack_bytes_rne(pr, pg, pb);
    const bool tie = (int)near_tie_byte<kRcasTieBits>(pr) | (int)near_tie_byte<kRcasTieBits>(pg) | (int)near_tie_byte<kRcasTieBits>(pb);
#ifdef OVRFSR_TIE_AUDIT
    // audit build: every stored pixel in reference order; counters g_ovrfsr_tie_audit_rcas (fsr_kernels.hip)
    float sr, sg, sb;
    rcas_resolve_ref(b, d, e, f, h, sharp, sr, sg, sb);
    const uint32_t sv = unit_to_unorm8(sr) | (unit_to_unorm8(sg) << 8) | (unit_to_unorm8(sb) << 16) | 0xff000000u;
    if (counted) {
        // the distance between the values the two stores round: the product's bytes clamped as its pack clamps them, sat(x) * 255 of the reference
        auto clampb = [](float x) { return fminf(fmaxf(x, 0.0f), 255.0f); };
        const float dist = fmaxf(fabsf(clampb(pr) - sat01(sr) * 255.0f), fmaxf(fabsf(clampb(pg) - sat01(sg) * 255.0f), fabsf(clampb(pb) - sat01(sb) * 255.0f)));
        atomicAdd(&g_ovrfsr_tie_audit_rcas[0], 1ull);
        if (tie) atomicAdd(&g_ovrfsr_tie_audit_rcas[1], 1ull);
        if (!tie && v != sv) atomicAdd(&g_ovrfsr_tie_audit_rcas[2], 1ull);
        atomicMax(&g_ovrfsr_tie_audit_rcas[3], (unsigned long long)__float_as_uint(dist));
    }
    if (tie) v = sv;
#else
    if (tie) {
        float sr, sg, sb;
        rcas_resolve_ref(b, d, e, f, h, sharp, sr, sg, sb);
        v = unit_to_unorm8(sr) | (unit_to_unorm8(sg) << 8) | (unit_to_unorm8(sb) << 16) | 0xff000000u;
    }
#endif
    return v;
}

template <int IN_FMT, int OUT_FMT, bool CHECKED, bool EXACT = false>
__device__ __forceinline__ void rcas_column4(OVRFSR_PTR_R(const uint8_t) in, OVRFSR_PTR_R(uint8_t) out, const ovrfsr::RcasArgs &a,
                                             int ox, int oy, int W, int H)
{
    constexpr bool byte_domain = IN_FMT == ovrfsr::FMT_RGBA8;
    [[maybe_unused]] constexpr float PEAK = byte_domain ? 255.0f : 1.0f;
    float4 c[6], l[4], r[4];
    if constexpr (IN_FMT == ovrfsr::FMT_RGBA8 && !CHECKED) {
        // interior workgroups: left, centre and right tap of a row are three adjacent texels: one 12-byte load instead of three
        // 4-byte ones (6 vector-memory loads per thread instead of 14; the kernel is co-limited by that path, see rcas_dpp_kernel)
        typedef uint32_t u32x3_a4_t __attribute__((ext_vector_type(3), aligned(4)));
        auto dec = [](uint32_t v) { return make_float4((float)(v & 0xffu), (float)((v >> 8) & 0xffu), (float)((v >> 16) & 0xffu), 0.0f); };
        c[0] = rcas_tap<IN_FMT, false>(in, a.v.in_pitch, ox, oy - 1, W, H);
        c[5] = rcas_tap<IN_FMT, false>(in, a.v.in_pitch, ox, oy + 4, W, H);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const u32x3_a4_t t = *OVRFSR_AT_N(const u32x3_a4_t, 12, in + ((uint32_t)(oy + i) * a.v.in_pitch + (uint32_t)(ox - 1) * 4u));
            l[i] = dec(t.x); c[i + 1] = dec(t.y); r[i] = dec(t.z);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 6; ++i) c[i] = rcas_tap<IN_FMT, CHECKED>(in, a.v.in_pitch, ox, oy - 1 + i, W, H);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            l[i] = rcas_tap<IN_FMT, CHECKED>(in, a.v.in_pitch, ox - 1, oy + i, W, H);
            r[i] = rcas_tap<IN_FMT, CHECKED>(in, a.v.in_pitch, ox + 1, oy + i, W, H);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (CHECKED && oy + i >= H) break;
        float pr, pg, pb;
        rcas_resolve_bytes<byte_domain>(c[i], l[i], c[i + 1], r[i], c[i + 2], a.sharp, pr, pg, pb);
        if constexpr (byte_domain && OUT_FMT == ovrfsr::FMT_RGBA8 && EXACT) {
            *OVRFSR_AT(uint32_t, out + (size_t)(oy + i) * a.v.out_pitch + (size_t)ox * 4) =
                rcas_exact_bytes(c[i], l[i], c[i + 1], r[i], c[i + 2], a.sharp, pr, pg, pb, true);
        } else if constexpr (byte_domain && OUT_FMT == ovrfsr::FMT_RGBA8) {
            *OVRFSR_AT(uint32_t, out + (size_t)(oy + i) * a.v.out_pitch + (size_t)ox * 4) = pack_bytes_rne(pr, pg, pb);
        } else if constexpr (byte_domain) {
            const float s = 1.0f / 255.0f;
            store_unit<OUT_FMT>(out, a.v.out_pitch, ox, oy + i, pr * s, pg * s, pb * s, 1.0f);
        } else {
            store_unit<OUT_FMT>(out, a.v.out_pitch, ox, oy + i, pr, pg, pb, 1.0f);
        }
    }
}

template <int IN_FMT, int OUT_FMT, bool EXACT>
__device__ __forceinline__ void rcas_direct_body(const ovrfsr::RcasArgs a)
{
    const uint32_t img_i = blockIdx.z;
    const uint32_t eye = (a.m.first_eye ^ (img_i & a.m.alternate)) & 1u;
    const uint32_t tile = a.tileList ? OVRFSR_TILE_LIST(a)[blockIdx.x] : xcd_tile_index(blockIdx.x, a.tilesX * a.tilesY);
    uint32_t tileX, tileY;
    tile_xy(tile, a.tilesX, a.tilesXMagic, tileX, tileY);
    OVRFSR_IMAGES(IN_FMT, OUT_FMT);
    const int W = a.v.outW, H = a.v.outH;
    const uint32_t inside_bits = tile_mask_bits(a.m, eye, tileX, tileY);
    const int lx = threadIdx.x & 31, ly = (int)(threadIdx.x >> 5) * 4; // 4 consecutive rows, inside one 16-row group
    const int ox = (int)tileX * ovrfsr::kTileW + lx, oy = (int)tileY * ovrfsr::kTileH + ly;
    if (ox >= W || oy >= H) return;
    const bool inside = (inside_bits >> ((uint32_t)(lx >> 4) + 2u * (uint32_t)(ly >> 4))) & 1u;
    if (inside) {
        // wave-uniform: does any tap of this 32x32 tile fall outside the image?
        const bool border = tileX == 0 || tileY == 0 || (int)(tileX + 1) * ovrfsr::kTileW + 1 > W || (int)(tileY + 1) * ovrfsr::kTileH + 1 > H;
        if (border) rcas_column4<IN_FMT, OUT_FMT, true, EXACT>(in, out, a, ox, oy, W, H);
        else rcas_column4<IN_FMT, OUT_FMT, false, EXACT>(in, out, a, ox, oy, W, H);
    } else {
        const float dbg = (float)a.debug;
        const float mulG = 1.0f - dbg * 0.3f;
        for (int i = 0; i < 4 && oy + i < H; ++i) {
            const float4 s = load_unit<IN_FMT>(in, a.v.in_pitch, ox, oy + i);
            store_unit<OUT_FMT>(out, a.v.out_pitch, ox, oy + i, s.x, s.y * mulG, s.z * mulG, s.w);
        }
    }
}
template <int IN_FMT, int OUT_FMT>
__global__ __launch_bounds__(256) void rcas_direct_kernel(const ovrfsr::RcasArgs a) { rcas_direct_body<IN_FMT, OUT_FMT, false>(a); }
// exact stores: RGBA8 -> RGBA8 only (the copy / tint outside the radius is the reference's evaluation already)
#ifndef OVRFSR_PACKED_TU /* not a template: defined once, in fsr_kernels.hip */
__global__ __launch_bounds__(256) void rcas_direct_exact_kernel(const ovrfsr::RcasArgs a) { rcas_direct_body<ovrfsr::FMT_RGBA8, ovrfsr::FMT_RGBA8, true>(a); }
#endif
// ------------------------------------------------------------------------------------------------
// RCAS, product build, unmasked RGBA8 source: neighbour reuse across lanes (north_star: "wave64 shuffles for neighbour
// reuse").  FsrRcasF's side taps d and f (ffx_fsr1.h:698-707) are the centre taps e of the pixels to the left and right,
// so a wave that covers 64 CONSECUTIVE columns of 4 rows lets every lane load and unpack only its own 6 centre-column
// texels and take the 24 side values from lanes -1 / +1 with v_mov_b32_dpp wave_shr:1 / wave_shl:1.  Lanes 0 and 63 have no
// neighbour on one side: they are halo lanes (load, unpack, store nothing), so a wave yields 62 columns.  Measured against
// the 14-loads-per-lane form above on the same arithmetic (tools/ubench/rcas_dpp_ab.hip, profiles/r02_rcas_dpp_ab.txt): the
// same VALU instruction count (94.7 vs 94.4 per 64 px -- a DPP move issues like the v_cvt it replaces, and 2 of 64 lanes
// idle) but 1.6 instead of 3.6 vector-memory loads per 64 px, and 16 % less time: 11.8 vs 14.0 us per eye.  Round 1 argued
// this could not pay because the kernel is VALU-issue-bound; the measurement says the texture-address path was co-limiting.
// Out-of-image taps read 0 (Texture2D.Load): halo lanes outside the image and rows outside it hold zeros, resolved only in
// workgroups that touch the image border.  Masked configurations keep rcas_direct_kernel (16x16 mask groups, tile lists).
// ------------------------------------------------------------------------------------------------
// bound_ctrl = 1: the lane without a source (lane 0 / 63, halo lanes) reads 0 and every lane is written, so the destination
// needs no initialising v_mov (6 fewer VALU instructions per pixel than the "old value" form)
__device__ __forceinline__ float dpp_from_left(float v) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x138, 0xf, 0xf, true)); }   // wave_shr:1
__device__ __forceinline__ float dpp_from_right(float v) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x130, 0xf, 0xf, true)); }  // wave_shl:1

// SPANS (round 3): the same kernel on a masked frame.  The tiles touching the radius form, per 32-row band, runs of
// adjacent tiles; the host cuts every run into 62-column segments (RcasArgs::spanRec) and a workgroup takes one segment
// instead of one cell of the regular 62 x 32 grid.  A lane whose 16x16 mask group lies outside the radius stores the
// reference's fallback instead -- the intermediate texel times (1 - debug*(0,.3,.3,0)), fsr_rcas.hlsl:46-47 -- evaluated as
// rcas_direct_kernel does (decode b/255, scale, re-encode).  A wave's 8 rows sit inside one 16-row group, so the test is one
// per lane.  Taps beyond the run are the ring tiles' bilinear intermediate (written by the EASU launch) or, where a
// lane's own group is outside, unused.
// TH (round 5): rows per workgroup, 4 waves x TH / 4 rows per lane.  32 for batches; a SMALL launch -- one eye image per call, the
// reference's own call pattern -- is 2 886 workgroups of TH = 32 on 2 048 resident slots: 1.41 rounds, the second one 41 % full.  With
// TH = 16 the same image is 2.8 rounds of half the length (launch_rcas picks the height from the grid size: profiles/r05_frame.txt).
// The body is fsr_rcas_dpp.inc, included as text by both kernels: the exact-stores instances add a template flag's worth of code, and a
// kernel's name carries its template arguments -- a flag on rcas_dpp_kernel itself would rename every shipped instance
// (profiles/r06_isa_fingerprint_r06.json), and a shared __device__ body, though always inlined, is scheduled differently.
template <int OUT_FMT, bool SPANS = false, int TH = ovrfsr::kRcasDppTileH>
__global__ __launch_bounds__(256) void rcas_dpp_kernel(const ovrfsr::RcasArgs a)
{
    constexpr bool EXACT = false;
#include "fsr_rcas_dpp.inc"
}
// exact stores: the RGBA8 destination only, in the three forms launch_rcas takes (32 rows, 16 rows, span records)
template <bool SPANS, int TH>
__global__ __launch_bounds__(256) void rcas_dpp_exact_kernel(const ovrfsr::RcasArgs a)
{
    constexpr int OUT_FMT = ovrfsr::FMT_RGBA8;
    constexpr bool EXACT = true;
#include "fsr_rcas_dpp.inc"
}
#endif // !OVRFSR_STRICT

// ------------------------------------------------------------------------------------------------
// Fused EASU -> RCAS (SURVEY.md 8f rank 1): one launch, the intermediate image never leaves the CU.
// A workgroup produces a 32x32 output tile.  RCAS needs the EASU result of the tile plus a 1-pixel
// ring, so EASU is evaluated on 34x34 pixels (13 % recompute) into an LDS plane; pixels outside the
// image are 0 there, which is what Texture2D.Load returns to the reference's RCAS.  The plane holds
// exactly what the second pass of the two-kernel path would read back from its intermediate
// texture, i.e. the value after that texture's format rounding (MID_FMT: RGBA8 = reference-faithful
// UNORM8 store, RGBA16F, RGBA32F = none) -- so fused and two-pass outputs are identical for the same
// build.  The radius mask is per 16x16 group for both stages; ring pixels take the EASU/bilinear
// branch of the neighbouring group they belong to.
// HBM traffic drops from 4*(in + 3*out) to 4*(in + out) bytes per eye (x2.3 at C2); on this chip the
// kernels are VALU-bound, so the recompute makes the fused form slightly slower -- see DESIGN.md.
// ------------------------------------------------------------------------------------------------
// The product build's register budget is part of the design (profiles/r03_fused_threads.txt, tests/test_kernel_resources.py):
// beside the outside-tile kernel of a masked half-float frame a SIMD hosts three fused waves and five outside waves only if both
// stay at <= 64 VGPRs -- ask the register allocator for 8 waves per SIMD.
#undef OVRFSR_FUSED_OCC
#if OVRFSR_STRICT || defined(OVRFSR_TIE_AUDIT) /* (the audit build re-resolves every pixel: no register budget) */
#define OVRFSR_FUSED_OCC
#else
#define OVRFSR_FUSED_OCC __attribute__((amdgpu_waves_per_eu(8, 8)))
#endif
// cell of the fused kernel's LDS intermediate plane
__device__ __forceinline__ float4 ldm(OVRFSR_PTR_RC(float4) mid, int i) { return mid[i]; }
__device__ __forceinline__ void stm(OVRFSR_PTR_R(float4) mid, int i, const float4 &v) { mid[i] = v; }
__device__ __forceinline__ void stm_comp(OVRFSR_PTR_R(float4) mid, int i, int q, float v) { OVRFSR_AS(float, mid + i)[q] = v; }

template <int IN_FMT, int MID_FMT, int OUT_FMT, int PITCH, int NT = ovrfsr::kThreads>
__global__ __launch_bounds__(NT) OVRFSR_FUSED_OCC void fused_kernel(const ovrfsr::FusedArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    OVRFSR_LDS_POISON(smem, a.ldsBytes);
    constexpr int MW = ovrfsr::kTileW + 2, MH = ovrfsr::kTileH + 2;
#if OVRFSR_STRICT
    typedef EasuTraits<IN_FMT> T;
    typedef typename T::cell_t cell_t;
    [[maybe_unused]] constexpr bool easu_bytes = false;
#else
    constexpr bool easu_bytes = IN_FMT == ovrfsr::FMT_RGBA8; // easu_resolve_fast returns 0..255 for RGBA8 input
#endif
    // domain of the LDS intermediate plane = domain the RCAS stage computes in
    constexpr bool mid_bytes = (OVRFSR_STRICT == 0) && MID_FMT == ovrfsr::FMT_RGBA8;
    constexpr float PEAK = mid_bytes ? 255.0f : 1.0f;

    const uint32_t img_i = blockIdx.z;
    const uint32_t eye = (a.m.first_eye ^ (img_i & a.m.alternate)) & 1u;
    const uint32_t tile = a.tileList ? OVRFSR_TILE_LIST(a)[blockIdx.x] : xcd_tile_index(blockIdx.x, a.tilesX * a.tilesY);
    uint32_t tileX, tileY;
    tile_xy(tile, a.tilesX, a.tilesXMagic, tileX, tileY);
    OVRFSR_IMAGES(IN_FMT, OUT_FMT);
    const int outW = a.v.outW, outH = a.v.outH;

    // mask bits of the 4x4 groups around the tile: bit (gy+1)*4 + (gx+1), gx,gy in -1..2
    uint32_t gbits = 0;
    {
        const uint32_t mode = a.m.mode[eye];
        if (mode == ovrfsr::MASK_ALL_INSIDE) gbits = 0xffffu;
        else if (mode == ovrfsr::MASK_MIXED) {
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int gx = 2 * (int)tileX + (g & 3) - 1, gy = 2 * (int)tileY + (g >> 2) - 1;
                // groups left of / above the image are never sampled (their pixels are outside -> 0)
                const bool in_g = gx >= 0 && gy >= 0 && group_inside((uint32_t)gx, (uint32_t)gy, a.m.centre[eye], a.m.r2);
                gbits |= (in_g ? 1u : 0u) << g;
            }
        }
    }
    // half intermediate of a float source: the footprint's largest |channel| (HDR tiles widen the guard's band, near_tie_half3_hdr)
    constexpr bool kTmax = (OVRFSR_STRICT == 0) && MID_FMT == ovrfsr::FMT_RGBA16F && IN_FMT != ovrfsr::FMT_RGBA8;
    __shared__ uint32_t tile_tmax;
    if (kTmax && threadIdx.x == 0) tile_tmax = 0u;
    const int ox0 = (int)tileX * ovrfsr::kTileW, oy0 = (int)tileY * ovrfsr::kTileH;
    // EASU footprint of the 34x34 block starting at (ox0-1, oy0-1)
    const int tile_x0 = (int)floorf(mad_unfused((float)(ox0 - 1), a.sx, a.cx)) - 1;
    const int tile_y0 = (int)floorf(mad_unfused((float)(oy0 - 1), a.sy, a.cy)) - 1;

#if OVRFSR_STRICT
    const size_t ncell = (size_t)a.cellsW * a.cellsH;
    OVRFSR_PTR(cell_t) col = OVRFSR_CARVE(cell_t, reinterpret_cast<cell_t *>(smem), ncell, 0, K_EASU_COL, smem, a.ldsBytes);
    OVRFSR_PTR(float4) ana = OVRFSR_CARVE(float4, reinterpret_cast<float4 *>(smem + align16(ncell * sizeof(cell_t))), ncell, 0, K_EASU_ANA, smem, a.ldsBytes);
    OVRFSR_PTR(float) lum = OVRFSR_CARVE(float, reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(OVRFSR_RAW(ana)) + ncell * sizeof(float4)), ncell, 0, K_EASU_LUM, smem, a.ldsBytes);
    typedef float4 mid_t;
    typedef cell_t col_t;
    OVRFSR_PTR(mid_t) mid = OVRFSR_CARVE(mid_t, reinterpret_cast<mid_t *>(reinterpret_cast<unsigned char *>(OVRFSR_RAW(lum)) + align16(ncell * sizeof(float))), MW * MH, 0, K_FUSED_MID, smem, a.ldsBytes);
    const int pitch = a.cellsW;
    if (gbits != 0u) easu_stage<IN_FMT>(in, a.v.in_pitch, a.v.inW, a.v.inH, tile_x0, tile_y0, a.cellsW, a.cellsH, col, lum, ana);
#else
    typedef float4 col_t;
    typedef float4 mid_t;
    const int ncell = PITCH * a.cellsH;
    OVRFSR_PTR(col_t) col = OVRFSR_CARVE(col_t, reinterpret_cast<col_t *>(smem), ncell, 0, K_EASU_COL, smem, a.ldsBytes);
    OVRFSR_PTR(float4) ana = OVRFSR_CARVE(float4, reinterpret_cast<float4 *>(OVRFSR_RAW(col) + ncell), ncell, 0, K_EASU_ANA, smem, a.ldsBytes);
    // (the kLumPadRows rows behind the luma plane that the analysis sweep may read are the head of the intermediate plane here --
    // bytes of this workgroup's own allocation, written only after the sweep's barrier)
    OVRFSR_PTR(float) lum = OVRFSR_CARVE(float, reinterpret_cast<float *>(OVRFSR_RAW(ana) + ncell), ncell, PITCH * ovrfsr::kLumPadRows, K_EASU_LUM, smem, a.ldsBytes);
    // (the luma plane doubles as the near-tie list region of stage 1: at least kFusedTieListBytes)
    OVRFSR_PTR(mid_t) mid = OVRFSR_CARVE(mid_t, reinterpret_cast<mid_t *>(OVRFSR_RAW(lum) + max(ncell, (int)(ovrfsr::kFusedTieListBytes / sizeof(float)))), MW * MH, 0, K_FUSED_MID, smem, a.ldsBytes);
    constexpr int pitch = PITCH;
    if (gbits != 0u) easu_stage_fast<IN_FMT, PITCH, NT, col_t>(in, a.v.in_pitch, a.v.inW, a.v.inH, tile_x0, tile_y0, a.cellsH, col, lum, ana, kTmax ? &tile_tmax : nullptr);
#endif
    // (workgroup-uniform: one LDS read into an SGPR; meaningful only where something was staged, and only read for EASU pixels)
    [[maybe_unused]] const float tmax_v = kTmax ? __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)tile_tmax)) : 1.0f;

    // ---- stage 1: EASU (or its bilinear fallback) on the 34x34 block -> LDS, with the intermediate format's rounding
    // Near-tie guard of the product build (see easu_fast_kernel): with a UNORM8 intermediate, a pixel whose re-associated EASU
    // result lies within 2^-TIE_BITS of a byte boundary is listed (per wave, ranked with mbcnt) and re-resolved in the
    // reference's operator order from the same LDS planes before the RCAS stage reads the plane: the intermediate is then
    // the oracle's, bit for bit, like the two-kernel path's.
    // A half intermediate is guarded on its half rounding boundaries (near_tie_half3).
    constexpr bool kGuardU8 = (OVRFSR_STRICT == 0) && easu_bytes && MID_FMT == ovrfsr::FMT_RGBA8;
    constexpr bool kGuardH = (OVRFSR_STRICT == 0) && MID_FMT == ovrfsr::FMT_RGBA16F;
    constexpr bool kGuard = kGuardU8 || kGuardH;
    constexpr int NW = NT / 64, kIters = (MW * MH + NT - 1) / NT, kWaveList = kIters * 64;
    // The lists live in the luma plane, which nothing reads once the analysis plane exists (the launcher makes that region
    // at least kFusedTieListBytes large): static LDS for them would take this kernel from 3 workgroups per CU to 2
    static_assert(NW * kWaveList * sizeof(uint16_t) <= ovrfsr::kFusedTieListBytes, "list region");
    [[maybe_unused]] OVRFSR_PTR(uint16_t) tie_list = OVRFSR_CARVE(uint16_t, reinterpret_cast<uint16_t *>(OVRFSR_RAW(lum)), NW * kWaveList, 0, K_TIE_LIST, smem, a.ldsBytes);
    OVRFSR_LDS_ARRAY(uint32_t, tie_cnt, NW, K_TIE_CNT);
    [[maybe_unused]] uint32_t tie_n = 0; // wave-uniform
    // The block as a linear sweep of 1156 pixels, every pixel from scratch (both builds; the strict build resolves in reference order)
#pragma unroll 1
    for (int it = 0; it < kIters; ++it) {
        const int i = threadIdx.x + it * NT;
        bool tie = false;
        if (i < MW * MH) {
        const int py = i / MW, px = i - py * MW;
        const int ox = ox0 - 1 + px, oy = oy0 - 1 + py;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f); // outside the image: Load returns 0
        if ((unsigned)ox < (unsigned)outW && (unsigned)oy < (unsigned)outH) {
            const int g = (((oy >> 4) - 2 * (int)tileY + 1) << 2) + ((ox >> 4) - 2 * (int)tileX + 1);
            float r, gg, b; // unit domain unless easu_bytes
            bool bytes = false;
            [[maybe_unused]] bool easu_px = false;
#ifdef OVRFSR_TIE_AUDIT
            [[maybe_unused]] int audit_base = 0;
            [[maybe_unused]] float audit_ppx = 0.0f, audit_ppy = 0.0f;
#endif
            if ((gbits >> g) & 1u) {
                const float ppx_raw = mad_unfused((float)ox, a.sx, a.cx), ppy_raw = mad_unfused((float)oy, a.sy, a.cy);
                const float fpx = floorf(ppx_raw), fpy = floorf(ppy_raw);
                const int base = ((int)fpy - tile_y0) * pitch + ((int)fpx - tile_x0);
#if OVRFSR_STRICT
                easu_resolve<false, cell_t>(col, ana, base, pitch, ppx_raw - fpx, ppy_raw - fpy, r, gg, b);
#else
                easu_resolve_fast<PITCH, col_t>(col, ana, base, ppx_raw - fpx, ppy_raw - fpy, r, gg, b);
                bytes = easu_bytes;
                easu_px = true;
                if constexpr (kGuardU8) tie = (int)near_tie_byte(r) | (int)near_tie_byte(gg) | (int)near_tie_byte(b);
#ifdef OVRFSR_TIE_AUDIT
                audit_base = base; audit_ppx = ppx_raw - fpx; audit_ppy = ppy_raw - fpy;
#endif
#endif
            } else {
                const float4 c = bilinear_global<IN_FMT>(in, a.v.in_pitch, a.v.inW, a.v.inH, ox, oy, (float)outW, (float)outH);
                r = c.x; gg = c.y; b = c.z;
            }
            // what the RCAS pass reads back from a MID_FMT texture, expressed in the RCAS stage's domain
            if constexpr (MID_FMT == ovrfsr::FMT_RGBA8) {
                float qr, qg, qb; // rounded byte values
                if (bytes) { qr = __builtin_rintf(r); qg = __builtin_rintf(gg); qb = __builtin_rintf(b); } // == v_cvt_pk_u8_f32 in range
                else { qr = (float)unit_to_unorm8(r); qg = (float)unit_to_unorm8(gg); qb = (float)unit_to_unorm8(b); }
                if constexpr (mid_bytes) v = make_float4(qr, qg, qb, 255.0f);
                else v = make_float4(unorm8_to_unit(qr), unorm8_to_unit(qg), unorm8_to_unit(qb), 1.0f);
            } else {
                if (bytes) { const float s = 1.0f / 255.0f; r *= s; gg *= s; b *= s; }
                if constexpr (MID_FMT == ovrfsr::FMT_RGBA16F) {
#if OVRFSR_STRICT
                    __asm__ volatile("" : "+v"(r), "+v"(gg), "+v"(b));
#endif
                    v = make_float4((float)(half_t)r, (float)(half_t)gg, (float)(half_t)b, 1.0f);
                    if constexpr (kGuardH)
                        tie = easu_px && near_tie_half3_hdr(r, gg, b, a.tieHalfMin, tmax_v);
                } else {
                    v = make_float4(r, gg, b, 1.0f);
                }
            }
#if defined(OVRFSR_TIE_AUDIT) && !OVRFSR_STRICT
            if constexpr (kGuard) {
                if (easu_px) tie_audit_px<easu_bytes, kGuardH>(col, ana, audit_base, pitch, audit_ppx, audit_ppy, r, gg, b, tie, a.tieHalfMin);
            }
#endif
        }
        stm(mid, i, v);
        }
        if constexpr (kGuard) { // whole wave, converged
            const uint64_t m = __builtin_amdgcn_ballot_w64(tie);
            if (tie) tie_list[(threadIdx.x >> 6) * kWaveList + tie_n + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = (uint16_t)i;
            tie_n += (uint32_t)__builtin_popcountll(m);
        }
    }
    if constexpr (kGuard) {
        if ((threadIdx.x & 63u) == 0u) tie_cnt[threadIdx.x >> 6] = tie_n;
        __syncthreads();
        uint32_t total = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) total += tie_cnt[w];
        const uint32_t rot = (threadIdx.x + 64u * (tile & 3u)) & (uint32_t)(NT - 1);
        auto entry = [&](uint32_t t, int &i, int &base, float &fppx, float &fppy) {
            uint32_t w = 0, off = t; // t-th entry of the concatenated per-wave lists (counts re-read from LDS: no registers held)
            while (w < (uint32_t)(NW - 1) && off >= tie_cnt[w]) off -= tie_cnt[w++];
            i = tie_list[w * kWaveList + off];
            const int py = i / MW, px = i - py * MW;
            const float ppx_raw = mad_unfused((float)(ox0 - 1 + px), a.sx, a.cx), ppy_raw = mad_unfused((float)(oy0 - 1 + py), a.sy, a.cy);
            const float fpx = floorf(ppx_raw), fpy = floorf(ppy_raw);
            base = ((int)fpy - tile_y0) * pitch + ((int)fpx - tile_x0); fppx = ppx_raw - fpx; fppy = ppy_raw - fpy;
        };
        if (total <= (uint32_t)(NT / 8)) { // workgroup-uniform: few pixels -> four lanes per pixel (easu_resolve_quad), each writes its component
            const int q = (int)(threadIdx.x & 3u);
#pragma unroll 1
            for (uint32_t t = rot >> 2; t < total; t += (uint32_t)(NT / 4)) {
                int i, base; float fppx, fppy;
                entry(t, i, base, fppx, fppy);
                const float v = easu_resolve_quad<easu_bytes, col_t>(col, ana, base, pitch, fppx, fppy, q);
                float o = kGuardU8 ? (float)unit_to_unorm8(v) : (float)(half_t)v;
                if (q == 3) o = kGuardU8 ? 255.0f : 1.0f;
                stm_comp(mid, i, q, o);
            }
        } else {
#pragma unroll 1
            for (uint32_t t = rot; t < total; t += (uint32_t)NT) { // one lane per listed pixel
                int i, base; float fppx, fppy, r, gg, b;
                entry(t, i, base, fppx, fppy);
                easu_resolve<easu_bytes, col_t>(col, ana, base, pitch, fppx, fppy, r, gg, b);
                if constexpr (kGuardU8) stm(mid, i, make_float4((float)unit_to_unorm8(r), (float)unit_to_unorm8(gg), (float)unit_to_unorm8(b), 255.0f)); // => mid_bytes
                else stm(mid, i, make_float4((float)(half_t)r, (float)(half_t)gg, (float)(half_t)b, 1.0f));
            }
        }
    }
    __syncthreads();

    // ---- stage 2: RCAS on the 32x32 tile from the LDS plane
    // (lane32_to_pos was measured here too: no gain on RGBA8 pipelines, and with 8-byte output texels the permuted lanes
    // spread each 16-lane store group over two 128-byte lines: C5 12.2 k -> 10.1 k pairs/s)
    const int lx = threadIdx.x & 31, ly0 = threadIdx.x >> 5;
    const int ox = ox0 + lx;
    if (ox >= outW) return;
    const float dbg = (float)a.debug;
    const float mulG = 1.0f - dbg * 0.3f;
    constexpr int ROWS = NT / 32; // tile rows per sweep
#pragma unroll 1
    for (int k = 0; k < ovrfsr::kTileH / ROWS; ++k) {
        const int ly = ly0 + ROWS * k;
        const int oy = oy0 + ly;
        if (oy >= outH) break;
        const int g = (((ly >> 4) + 1) << 2) + ((lx >> 4) + 1);
        const int c = (ly + 1) * MW + (lx + 1);
        float pr, pg, pb, pa;
        if ((gbits >> g) & 1u) {
            const float4 b = ldm(mid, c - MW), d = ldm(mid, c - 1), e = ldm(mid, c), f = ldm(mid, c + 1), h = ldm(mid, c + MW);
#if OVRFSR_STRICT
            rcas_resolve(b, d, e, f, h, a.sharp, pr, pg, pb);
#else
            if constexpr (mid_bytes) {
                rcas_resolve_bytes<true>(b, d, e, f, h, a.sharp, pr, pg, pb); // the RCAS kernels' one-quotient form: one helper, so the two cannot drift
            } else {
                const float mnR = raw_min(raw_min3(b.x, d.x, f.x), h.x), mxR = raw_max(raw_max3(b.x, d.x, f.x), h.x);
                const float mnG = raw_min(raw_min3(b.y, d.y, f.y), h.y), mxG = raw_max(raw_max3(b.y, d.y, f.y), h.y);
                const float mnB = raw_min(raw_min3(b.z, d.z, f.z), h.z), mxB = raw_max(raw_max3(b.z, d.z, f.z), h.z);
                const float hitMinR = mnR * __builtin_amdgcn_rcpf(4.0f * mxR);
                const float hitMinG = mnG * __builtin_amdgcn_rcpf(4.0f * mxG);
                const float hitMinB = mnB * __builtin_amdgcn_rcpf(4.0f * mxB);
                const float hitMaxR = (PEAK - mxR) * __builtin_amdgcn_rcpf(4.0f * mnR + -4.0f * PEAK);
                const float hitMaxG = (PEAK - mxG) * __builtin_amdgcn_rcpf(4.0f * mnG + -4.0f * PEAK);
                const float hitMaxB = (PEAK - mxB) * __builtin_amdgcn_rcpf(4.0f * mnB + -4.0f * PEAK);
                const float lobeR = fmaxf(-hitMinR, hitMaxR), lobeG = fmaxf(-hitMinG, hitMaxG), lobeB = fmaxf(-hitMinB, hitMaxB);
                const float lobe = __builtin_amdgcn_fmed3f(fmaxf(lobeR, fmaxf(lobeG, lobeB)), -OVRFSR_RCAS_LIMIT, 0.0f) * a.sharp;
                const float rcpL = prx_med_rcp(4.0f * lobe + 1.0f);
                pr = (lobe * ((b.x + d.x) + (h.x + f.x)) + e.x) * rcpL;
                pg = (lobe * ((b.y + d.y) + (h.y + f.y)) + e.y) * rcpL;
                pb = (lobe * ((b.z + d.z) + (h.z + f.z)) + e.z) * rcpL;
            }
#endif
            pa = PEAK;
        } else {
            const float4 s = ldm(mid, c);
            if constexpr (mid_bytes) {
                // tinted copy of a UNORM8 intermediate texel (fsr_rcas.hlsl:46-47), evaluated as the reference does --
                // decode b/255, scale, re-encode -- and brought back to the byte domain of this stage (exact integers)
                pr = s.x; pa = s.w;
                pg = a.debug ? (float)unit_to_unorm8(unorm8_to_unit(s.y) * mulG) : s.y;
                pb = a.debug ? (float)unit_to_unorm8(unorm8_to_unit(s.z) * mulG) : s.z;
                if constexpr (OUT_FMT != ovrfsr::FMT_RGBA8) {
                    // float / half destination: the un-rounded tinted value, stored directly
                    store_unit<OUT_FMT>(out, a.v.out_pitch, ox, oy, unorm8_to_unit(s.x), unorm8_to_unit(s.y) * mulG, unorm8_to_unit(s.z) * mulG, unorm8_to_unit(s.w));
                    continue;
                }
            } else {
                pr = s.x * (1.0f - dbg * 0.0f); pg = s.y * mulG; pb = s.z * mulG; pa = s.w * (1.0f - dbg * 0.0f);
            }
        }
        if constexpr (mid_bytes) {
            if constexpr (OUT_FMT == ovrfsr::FMT_RGBA8) {
                uint32_t v = 0;
                v = __builtin_amdgcn_cvt_pk_u8_f32(pr, 0, v);
                v = __builtin_amdgcn_cvt_pk_u8_f32(pg, 1, v);
                v = __builtin_amdgcn_cvt_pk_u8_f32(pb, 2, v);
                v = __builtin_amdgcn_cvt_pk_u8_f32(pa, 3, v);
                *OVRFSR_AT(uint32_t, out + (size_t)oy * a.v.out_pitch + (size_t)ox * 4) = v;
            } else {
                const float s = 1.0f / 255.0f;
                store_unit<OUT_FMT>(out, a.v.out_pitch, ox, oy, pr * s, pg * s, pb * s, pa * s);
            }
        } else {
            store_unit<OUT_FMT>(out, a.v.out_pitch, ox, oy, pr, pg, pb, pa);
        }
    }
}
