// fsr_launch.h -- the typed launchers the host launch manager calls: declarations only.  They are implemented in the kernel units
// (fsr_kernels.hip, fsr_packed_kernels.hip, nis_kernels.hip), out of the pieces in fsr_launch_impl.h; every one of them clears the thread's
// pending HIP error before it launches (launch_fresh there), so what it returns is its own launch's.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include "fsr_params.h"
#include "fsr_sizes.h" // the size rules the launchers go by (and the pipeline planner decides by)

namespace ovrfsr {
hipError_t launch_easu(int prec, int in_fmt, int out_fmt, const EasuArgs &a, uint32_t batch, hipStream_t s, uint32_t nTiles = 0);
hipError_t launch_easu_outside(int in_fmt, int mid_fmt, int out_fmt, const EasuArgs &a, uint32_t nTiles, uint32_t batch, hipStream_t s);
hipError_t launch_fused(int prec, int in_fmt, int mid_fmt, int out_fmt, const FusedArgs &a, uint32_t batch, hipStream_t s, uint32_t nTiles = 0);
hipError_t launch_rcas(int prec, int in_fmt, int out_fmt, const RcasArgs &a, uint32_t batch, hipStream_t s, uint32_t nTiles = 0);
hipError_t launch_nis_scaler(int prec, int in_fmt, int out_fmt, const NisArgs &a, uint32_t batch, hipStream_t s, uint32_t nGroups = 0);
hipError_t launch_bgra_to_rgba(const uint8_t *src, uint32_t srcPitch, uint64_t srcStride, uint8_t *dst, uint32_t w, uint32_t h,
                              uint32_t batch, hipStream_t s);
// multisampled input (OVRFSR_FORMAT_MS) -> single-sample image of the base format (BGRA8 -> RGBA8): image i of the batch at
// dst + i * h * resolve_pitch(fmt, w), rows resolve_pitch(fmt, w) bytes apart (the row bytes rounded up to 16)
// fmt FMT_R11G11B10F (samples 1, 2, 4 or 8): 4-byte packed texels in, RGBA16F texels out -- the one source whose destination texel
// has another size: resolve_pitch(FMT_R11G11B10F, w) is the pitch of the 8-byte copy
// launch_easu, launch_fused and launch_easu_outside also take in_fmt FMT_R11G11B10F as it is: single-sample words decoded where the kernels
// stage or load their texels (product build, fixed LDS pitches; hipErrorInvalidValue for the strict build and wider footprints).  Those
// instances live in a translation unit of their own (fsr_packed_kernels.hip), so in a code object of their own: the runtime loads a code
// object at the first launch from it, and a host that never submits the format never loads theirs -- what the other kernels' code object
// costs to load and hold stays what it was.  The three launchers hand over to these (`a` complete, tilesXMagic included):
hipError_t launch_easu_packed(int out_fmt, const EasuArgs &a, dim3 grid, hipStream_t s);
hipError_t launch_fused_packed(int mid_fmt, int out_fmt, const FusedArgs &a, dim3 grid, size_t lds, hipStream_t s);
hipError_t launch_easu_outside_packed(int mid_fmt, int out_fmt, const EasuArgs &a, dim3 grid, hipStream_t s);
hipError_t tie_audit_read_packed(unsigned long long out[6], bool reset); // that unit's counters (-DOVRFSR_TIE_AUDIT; zeros otherwise)
hipError_t bounds_read_packed(unsigned long long *out, bool reset);      // ... and its checked-accessor counters (-DOVRFSR_BOUNDS)
// (resolve_pitch, easu_msaa_fused_ok -- FMT_RGBA8_MS4 resolved inside easu_fast_kernel's staging sweep -- and outside_staged_ok: fsr_sizes.h)
hipError_t launch_resolve(int fmt, int samples, const uint8_t *src, uint32_t srcPitch, uint64_t srcStride, uint8_t *dst, uint32_t w, uint32_t h,
                          uint32_t batch, hipStream_t s);
// OVRFSR_HDR_DOMAIN_SRTM (fsr_hdr_domain.inc): fmt RGBA16F / RGBA32F pipeline input -> tight RGBA32F copy, mapped; and that layout back into an RGBA8 / RGBA16F / RGBA32F destination, un-mapped
hipError_t launch_hdr_forward(int fmt, const uint8_t *src, uint32_t srcPitch, uint64_t srcStride, uint8_t *dst, uint32_t w, uint32_t h, uint32_t batch, hipStream_t s);
hipError_t launch_hdr_back(int fmt, const uint8_t *src, uint8_t *dst, uint32_t dstPitch, uint64_t dstStride, uint32_t w, uint32_t h, uint32_t batch, hipStream_t s);
// the 16-byte records of the first a.n[eye] entries of both list regions (fsr_tile_records.inc); no launch where both are empty
hipError_t launch_tile_records(const TileRecordsArgs &a, hipStream_t s);
// the column taps, their padding copies and the row taps for the two sizes of `a`, in place (fsr_tap_tables.inc)
hipError_t launch_tap_tables(const TapTablesArgs &a, hipStream_t s);
// the mask-feather pass over tilesW x tilesH tiles of `batch` images, in place on a.v.out (fsr_mask_feather.inc)
hipError_t launch_mask_feather(const FeatherArgs &a, uint32_t tilesW, uint32_t tilesH, uint32_t batch, hipStream_t s);
hipError_t launch_outside_staged(int tileH, int in_fmt, int mid_fmt, int out_fmt, const OutsideArgs &a, uint32_t nTiles, uint32_t batch, hipStream_t s);
hipError_t launch_nis_outside(int in_fmt, int out_fmt, const NisArgs &a, uint32_t nGroups, uint32_t batch, hipStream_t s);
hipError_t launch_nis_sharpen(int prec, int in_fmt, int out_fmt, const NisArgs &a, uint32_t batch, hipStream_t s);
hipError_t tie_audit_read(unsigned long long out[6], bool reset); // -DOVRFSR_TIE_AUDIT builds only (fsr_kernels.hip)
hipError_t tie_audit_read_rcas(unsigned long long out[5], bool reset); // the same for the exact-stores RCAS instances ([4]: the band's bit count)
// -DOVRFSR_BOUNDS builds only (fsr_bounds.h): the checked accessors' counters of the current device, one array per kernel translation
// unit (fsr_kernels.hip / nis_kernels.hip), ADDED into out[ovrfsr_chk::kSlots] (the first-hit record: copied if out has none yet);
// and a launch that drives the accessors through every kind of violation once (fsr_kernels.hip)
hipError_t bounds_read_fsr(unsigned long long *out, bool reset);
hipError_t bounds_read_nis(unsigned long long *out, bool reset);
hipError_t bounds_selftest();
} // namespace ovrfsr
