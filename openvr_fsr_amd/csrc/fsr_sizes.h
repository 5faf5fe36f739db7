// fsr_sizes.h -- the size rules of the kernels: LDS pitches, LDS bytes, and which kernel a shape may take.  Host only, inline, no HIP call:
// the pipeline planner (pipeline_plan.cpp) decides by them and the launchers (fsr_kernels.hip, fsr_packed_kernels.hip, nis_kernels.hip) launch by them, so that
// what the planner accepts is what the launchers can run.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "fsr_formats.h"
#include "fsr_params.h"

namespace ovrfsr {

// LDS row pitch (cells) of the product-build EASU kernel; 0 = footprint too wide, use the generic kernel
inline int easu_fast_pitch(int cellsW) { return cellsW <= 32 ? 32 : cellsW <= 40 ? 40 : 0; }
// the EASU-only kernel also has a 28-cell pitch: exactly the footprint of a 32-pixel tile at scale 3/4
inline int easu_kernel_pitch(int cellsW) { return cellsW <= 28 ? 28 : easu_fast_pitch(cellsW); }

// (in_fmt FMT_R11G11B10F -- words decoded in staging, product build, fixed pitches only -- sizes like the RGBA16F texels it decodes to)
inline size_t easu_lds_bytes(int prec, int in_fmt, int cellsW, int cellsH)
{
    if (prec != PREC_FP32_STRICT && easu_fast_pitch(cellsW) != 0)
        return (size_t)easu_fast_pitch(cellsW) * cellsH * (16 + 16 + 4) + (size_t)easu_fast_pitch(cellsW) * kLumPadRows * 4; // pitch 32/40 (the fused kernel's; 28 fits inside) + kLumPadRows
    const bool wide = (prec == PREC_FP32_STRICT) || (in_fmt == FMT_RGBA32F) || (in_fmt == FMT_RGB10A2);
    const size_t ncell = (size_t)cellsW * cellsH;
    const size_t col = (ncell * (wide ? 16 : 8) + 15) & ~(size_t)15;
    return col + ncell * 16 + ncell * 4;
}

// LDS of the fused kernel: EASU planes + 34x34 intermediate (float4 cells)
inline size_t fused_lds_bytes(int prec, int in_fmt, int mid_fmt, int cellsW, int cellsH)
{
    size_t e = easu_lds_bytes(prec, in_fmt, cellsW, cellsH);
    e = (e + 15) & ~(size_t)15;
    size_t midCell = 16;
    if (prec != PREC_FP32_STRICT && easu_fast_pitch(cellsW) != 0) {
        const size_t ncell = (size_t)easu_fast_pitch(cellsW) * cellsH;
        // the luma plane doubles as the near-tie list region (fused_kernel) and is at least that large
        if (ncell * 4 < kFusedTieListBytes) e += kFusedTieListBytes;
    }
    (void)mid_fmt;
    return e + (size_t)(kTileW + 2) * (kTileH + 2) * midCell;
}

// NVScaler: LDS row pitch (cells) of a 32x24 group's footprint; 0 = too wide
inline int nis_pitch(int cellsW) { return cellsW <= 32 ? 32 : cellsW <= 40 ? 40 : 0; }
inline size_t nis_scaler_lds_bytes(int cellsW, int cellsH) { return (size_t)nis_pitch(cellsW) * cellsH * (4 + 4 + 16 + 4) + 2 * 512 * 4; } // Yu, Y255, E, raw texel

// LDS-staged outside-tile kernel (outside_staged_kernel): upscaling only, RGBA8 sources (any destination format).
// RGBA16F sources stay on the per-pixel kernel: stand-alone the staged form is 11 % faster there too (C5: 1020 -> 904 us),
// but its 20 KB of LDS per workgroup cannot co-reside with three 52 KB fused-kernel workgroups per CU, and the overlapped
// step gets 20 % slower.
inline bool outside_staged_ok(const BatchView &v, int in_fmt) { return v.inW <= v.outW && v.inH <= v.outH && in_fmt == FMT_RGBA8; }

// 4-sample RGBA8 input resolved inside easu_fast_kernel's staging sweep (in_fmt FMT_RGBA8_MS4 of launch_easu): product build, unmasked,
// UNORM8 destination (the pipeline's intermediate or an EASU-only output), a fixed LDS pitch
inline bool easu_msaa_fused_ok(int prec, int out_fmt, int cellsW)
{
    return prec == PREC_FP32 && out_fmt == FMT_RGBA8 && easu_kernel_pitch(cellsW) != 0;
}

// rcas_dpp_kernel's grid for an unmasked launch: tiles of 62 stored columns by `rows` (kRcasDppTileH = 32, or 16) rows
inline uint32_t rcas_dpp_tiles_x(int outW) { return (uint32_t)(outW + kRcasDppTileW - 1) / kRcasDppTileW; }
inline uint32_t rcas_dpp_tiles_y(int outH, int rows) { return (uint32_t)(outH + rows - 1) / rows; }
// ... and its height for such a launch of `batch` images: true = the 16-row form.  Small launches: the grid is r = workgroups /
// kRcasResident rounds of the resident workgroups, the last one partly filled; half-height workgroups run ceil(2r) rounds of half the
// length (3 % more work per pixel).  One C2 eye image: r = 1.41, 2 rounds against 3 half rounds = 1.5 (14.4 instead of 15.5 us,
// profiles/r05_frame.txt); a batch: no difference, the 8-row form wins
inline bool rcas_dpp_small(int outW, int outH, uint32_t batch)
{
    const uint64_t wgs = (uint64_t)rcas_dpp_tiles_x(outW) * rcas_dpp_tiles_y(outH, kRcasDppTileH) * batch;
    const uint64_t full = (wgs + kRcasResident - 1) / kRcasResident, half = (2 * wgs + kRcasResident - 1) / kRcasResident;
    return wgs < 16 * kRcasResident && 103 * half < 200 * full;
}

// rows of the resolve pass's destination: texels of the format the pipeline sees (R11G11B10F: 4-byte words in, RGBA16F out), padded to 16 bytes
inline uint32_t resolve_pitch(int fmt, uint32_t w)
{
    return (w * texel_bytes(pipeline_format((uint32_t)fmt)) + 15u) & ~15u;
}

// The launch manager's own copies of its input, and the bytes of ONE image of each for a submission of (fmt, w, h) -- 64-bit: the mapped
// copy of a 16384 x 16384 image is 4 GiB.  The build (at the maximum input size) and the per-call path size the copies by this and nothing else.
enum class InputCopy {
    Resolved,  // the resolve / unpack pass's destination: single-sample texels of pipeline_format, rows of resolve_pitch
    Reordered, // the BGRA8 re-order's destination: RGBA8, tight
    Mapped     // the HDR domain's forward map: RGBA32F, tight
};
inline uint64_t input_copy_bytes(InputCopy copy, uint32_t fmt, uint32_t w, uint32_t h)
{
    return copy == InputCopy::Resolved  ? (uint64_t)resolve_pitch((int)base_format(fmt), w) * h
         : copy == InputCopy::Reordered ? (uint64_t)w * h * texel_bytes(OVRFSR_FORMAT_RGBA8_UNORM)
                                        : (uint64_t)w * h * 16u;
}

} // namespace ovrfsr
