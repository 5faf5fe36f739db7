// fsr_rcas_dpp.inc -- the body of rcas_dpp_kernel and rcas_dpp_exact_kernel (fsr_kernels.inc), included inside each.
// In scope: a (RcasArgs), OUT_FMT, SPANS, TH, EXACT (exact stores: the final byte guarded, rcas_exact_bytes).
    constexpr int TW = ovrfsr::kRcasDppTileW, R = TH / 4; // 62 stored columns per wave, 4 waves x R rows
    static_assert(!SPANS || TH == ovrfsr::kRcasDppTileH, "the host cuts its span records for 32-row bands");
    static_assert(TH == 32 || TH == 16, "a wave's R rows must sit inside one 16-row mask group");
    // (8 rows per lane: 10 loads per 8 pixels and half the per-thread prologue of the 4-row form: RCAS-only +2.7 % on batches)
    const uint32_t img_i = blockIdx.z;
    const int W = a.v.outW, H = a.v.outH;
    OVRFSR_IMAGES(ovrfsr::FMT_RGBA8, OUT_FMT);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x, y, xEnd;
    bool border;
    if constexpr (SPANS) {
        const uint32_t r0 = OVRFSR_SPAN_REC(a)[2 * blockIdx.x], r1 = OVRFSR_SPAN_REC(a)[2 * blockIdx.x + 1]; // uniform
        const int x0 = (int)(r0 & 0xffffu), tileY = (int)(r0 >> 16);
        xEnd = (int)r1;
        x = x0 + lane - 1; y = tileY * TH + wave * R;
        border = x0 == 0 || x0 + TW + 1 > W || tileY == 0 || (tileY + 1) * TH + 1 > H;
    } else {
        const uint32_t tilesX = (uint32_t)(W + TW - 1) / TW, tilesY = (uint32_t)(H + TH - 1) / TH;
        const uint32_t tile = xcd_tile_index(blockIdx.x, tilesX * tilesY);
        uint32_t tileX, tileY;
        tile_xy(tile, tilesX, a.dppTilesXMagic, tileX, tileY);
        x = (int)tileX * TW + lane - 1; y = (int)tileY * TH + wave * R;
        xEnd = W;
        // workgroup-uniform: does any tap of this block (columns -1..62, rows -1..16 of the tile) fall outside the image?
        border = tileX == 0 || (int)(tileX + 1) * TW + 1 > W || tileY == 0 || (int)(tileY + 1) * TH + 1 > H;
    }
    if (y >= H) return; // wave-uniform
    float4 c[R + 2];
    if (border) {
#pragma unroll
        for (int i = 0; i < R + 2; ++i) c[i] = rcas_tap<ovrfsr::FMT_RGBA8, true>(in, a.v.in_pitch, x, y - 1 + i, W, H);
    } else {
#pragma unroll
        for (int i = 0; i < R + 2; ++i) c[i] = rcas_tap<ovrfsr::FMT_RGBA8, false>(in, a.v.in_pitch, x, y - 1 + i, W, H);
    }
    const bool store = lane >= 1 && lane <= TW && x < xEnd;
    [[maybe_unused]] bool inside = true;
    if constexpr (SPANS) {
        const uint32_t eye = (a.m.first_eye ^ (img_i & a.m.alternate)) & 1u;
        const uint32_t mode = a.m.mode[eye];
        inside = mode == ovrfsr::MASK_ALL_INSIDE ||
                 (mode == ovrfsr::MASK_MIXED && x >= 0 && group_inside((uint32_t)x >> 4, (uint32_t)y >> 4, a.m.centre[eye], a.m.r2));
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const float4 e = c[i + 1];
        const float4 d = make_float4(dpp_from_left(e.x), dpp_from_left(e.y), dpp_from_left(e.z), 0.0f);
        const float4 f = make_float4(dpp_from_right(e.x), dpp_from_right(e.y), dpp_from_right(e.z), 0.0f);
        float pr, pg, pb;
        rcas_resolve_bytes<true>(c[i], d, e, f, c[i + 2], a.sharp, pr, pg, pb);
        if constexpr (SPANS) {
            if (!inside) { // byte domain: decode, tint, re-encode (identity without the debug tint)
                const float mulG = 1.0f - 0.3f;
                pr = e.x;
                pg = a.debug ? (float)unit_to_unorm8(unorm8_to_unit(e.y) * mulG) : e.y;
                pb = a.debug ? (float)unit_to_unorm8(unorm8_to_unit(e.z) * mulG) : e.z;
            }
        }
        if (store && y + i < H) {
            if constexpr (OUT_FMT == ovrfsr::FMT_RGBA8 && EXACT) {
                // (SPANS && !inside: pr, pg, pb are the copied / tinted bytes, whole numbers -- exact already, outside the guard)
                const uint32_t v = SPANS && !inside ? pack_bytes_rne(pr, pg, pb) : rcas_exact_bytes(c[i], d, e, f, c[i + 2], a.sharp, pr, pg, pb, true);
                *OVRFSR_AT(uint32_t, out + ((uint32_t)(y + i) * a.v.out_pitch + (uint32_t)x * 4u)) = v;
            } else if constexpr (OUT_FMT == ovrfsr::FMT_RGBA8) {
                *OVRFSR_AT(uint32_t, out + ((uint32_t)(y + i) * a.v.out_pitch + (uint32_t)x * 4u)) = pack_bytes_rne(pr, pg, pb);
            } else {
                const float s = 1.0f / 255.0f;
                if (SPANS && !inside) { // the un-rounded tinted texel, as rcas_direct_kernel stores it
                    const float mulG = 1.0f - (float)a.debug * 0.3f;
                    store_unit<OUT_FMT>(out, a.v.out_pitch, x, y + i, unorm8_to_unit(e.x), unorm8_to_unit(e.y) * mulG, unorm8_to_unit(e.z) * mulG, 1.0f);
                } else {
                    store_unit<OUT_FMT>(out, a.v.out_pitch, x, y + i, pr * s, pg * s, pb * s, 1.0f);
                }
            }
        }
    }
