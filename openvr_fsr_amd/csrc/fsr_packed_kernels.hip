// fsr_packed_kernels.hip -- the product-build instances that read single-sample R11G11B10F words themselves (input format 6 of
// easu_fast_kernel, fused_kernel and easu_outside_kernel: the word is decoded where the kernel stages or loads its texels, fsr_device.inc
// unpack_r11g11b10f), and their launchers.  A translation unit of its own is a code object of its own: the runtime loads a code object at
// the first launch from it, so a process that never submits the format never loads this one, and fsr_kernels.hip's code object -- what it
// costs to load, to hold and to tear down at exit -- is what it was before these instances existed.  The kernel text is fsr_kernels.inc's,
// included once more (product namespace only: no strict instance reads the word); nothing but the instances named below is emitted.
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdlib>
#include <type_traits>
#include "fsr_params.h"
#include "fsr_launch.h"
#include "fsr_formats.h"
#include "fsr_bounds.h"

#define OVRFSR_PACKED_TU 1
#ifdef OVRFSR_TIE_AUDIT
// this unit's own audit counters (layout: fsr_kernels.hip); tie_audit_read adds them to its own.  (The RCAS array is named by kernel text
// that is never instantiated here.)
static __device__ unsigned long long g_ovrfsr_tie_audit[6];
static __device__ unsigned long long g_ovrfsr_tie_audit_rcas[4];
#endif

namespace ovrfsr_fast {
#define OVRFSR_STRICT 0
#pragma clang fp contract(fast)
#include "fsr_device.inc"
#include "fsr_kernels.inc"
#undef OVRFSR_STRICT
} // namespace ovrfsr_fast
#pragma clang fp contract(on)

// The launchers: fsr_kernels.hip's pieces (fsr_launch_impl.h) on this unit's instances.  The order in which they name the kernels is the
// order of the kernels in this code object (see there).
#define OVRFSR_LAUNCH_FSR 1
#include "fsr_launch_impl.h"

namespace ovrfsr {

template <int I, int O>
static hipError_t easu_packed(const EasuArgs &a, dim3 grid, hipStream_t s)
{
    const int pitch = easu_kernel_pitch(a.cellsW);
    if (pitch == 0) return hipErrorInvalidValue; // wider footprints have no instance: the launch manager sends them through the resolve pass
    return is_masked(a.m) ? easu_fast_go<I, O, true>(pitch, a, grid, s) : easu_fast_go<I, O, false>(pitch, a, grid, s);
}

// the words decode to RGBA16F texels: a half or a float intermediate, as for an RGBA16F input
template <int I, int O>
static hipError_t fused_packed(int mid_fmt, const FusedArgs &a, dim3 grid, size_t lds, hipStream_t s)
{
    return fused_go<FusedFast, I, O, FMT_RGBA8, FMT_RGBA16F, FMT_RGBA32F>(mid_fmt, a, grid, lds, s);
}
// ... and behind them, under cfg.reference_formats, a UNORM8 one (the outside-tile kernel only)
template <int I, int O>
static hipError_t easu_outside_packed(int mid_fmt, const EasuArgs &a, dim3 grid, hipStream_t s)
{
    return easu_outside_go<I, O, -1, FMT_RGBA16F, FMT_RGBA32F, FMT_RGBA8>(mid_fmt, a, grid, s);
}

// the destination of a launch from packed words: RGBA8, RGBA16F or RGBA32F
#define OVRFSR_PACKED_OUT(FN, ...) OVRFSR_DISPATCH_OUT(FMT_R11G11B10F, FN, __VA_ARGS__) return hipErrorInvalidValue;

hipError_t launch_easu_packed(int out_fmt, const EasuArgs &a, dim3 grid, hipStream_t s) { OVRFSR_PACKED_OUT(easu_packed, a, grid, s) }
hipError_t launch_fused_packed(int mid_fmt, int out_fmt, const FusedArgs &a, dim3 grid, size_t lds, hipStream_t s) { OVRFSR_PACKED_OUT(fused_packed, mid_fmt, a, grid, lds, s) }
hipError_t launch_easu_outside_packed(int mid_fmt, int out_fmt, const EasuArgs &a, dim3 grid, hipStream_t s) { OVRFSR_PACKED_OUT(easu_outside_packed, mid_fmt, a, grid, s) }

hipError_t tie_audit_read_packed(unsigned long long out[6], bool reset)
{
#ifdef OVRFSR_TIE_AUDIT
    return read_counters(HIP_SYMBOL(g_ovrfsr_tie_audit), out, 6, reset);
#else
    for (int i = 0; i < 6; ++i) out[i] = 0;
    (void)reset;
    return hipSuccess;
#endif
}

#ifdef OVRFSR_BOUNDS
hipError_t bounds_read_packed(unsigned long long *out, bool reset) { return ovrfsr_chk::read_counts(out, reset); }
#else
hipError_t bounds_read_packed(unsigned long long *, bool) { return hipErrorNotSupported; }
#endif

} // namespace ovrfsr
