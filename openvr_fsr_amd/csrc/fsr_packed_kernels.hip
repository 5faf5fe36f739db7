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

namespace ovrfsr {

constexpr int I = FMT_R11G11B10F;

template <int O, bool M>
static void easu_packed_go(int pitch, const EasuArgs &a, dim3 grid, hipStream_t s)
{
    const size_t lds = (size_t)pitch * a.cellsH * 36 + (size_t)pitch * kLumPadRows * 4; // colour + analysis (float4) + luma planes + pad rows
    if (pitch == 28) hipLaunchKernelGGL((ovrfsr_fast::easu_fast_kernel<I, O, 28, M>), grid, dim3(kThreads), lds, s, with_lds(a, lds));
    else if (pitch == 32) hipLaunchKernelGGL((ovrfsr_fast::easu_fast_kernel<I, O, 32, M>), grid, dim3(kThreads), lds, s, with_lds(a, lds));
    else hipLaunchKernelGGL((ovrfsr_fast::easu_fast_kernel<I, O, 40, M>), grid, dim3(kThreads), lds, s, with_lds(a, lds));
}
template <int O>
static hipError_t easu_packed(const EasuArgs &a, dim3 grid, hipStream_t s)
{
    const int pitch = easu_kernel_pitch(a.cellsW);
    if (pitch == 0) return hipErrorInvalidValue; // wider footprints have no instance: the launch manager sends them through the resolve pass
    if (a.m.mode[0] != MASK_ALL_INSIDE || a.m.mode[1] != MASK_ALL_INSIDE) easu_packed_go<O, true>(pitch, a, grid, s);
    else easu_packed_go<O, false>(pitch, a, grid, s);
    return hipGetLastError();
}

// (the dynamic-LDS cap is raised per kernel instantiation and device: fused_go3, fsr_kernels.hip)
template <int M, int O, int PITCH>
static hipError_t fused_packed_go(const FusedArgs &a, dim3 grid, size_t lds, hipStream_t s)
{
    static std::atomic<uint64_t> done{0};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const uint64_t bit = 1ull << (dev & 63);
    if (!(done.load(std::memory_order_acquire) & bit)) {
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(&ovrfsr_fast::fused_kernel<I, M, O, PITCH, kFusedThreads>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFusedLdsMax);
        if (e != hipSuccess) return e;
        done.fetch_or(bit, std::memory_order_release);
    }
    hipLaunchKernelGGL((ovrfsr_fast::fused_kernel<I, M, O, PITCH, kFusedThreads>), grid, dim3(kFusedThreads), lds, s, with_lds(a, lds));
    return hipGetLastError();
}
// the words decode to RGBA16F texels: a half or a float intermediate, as for an RGBA16F input
template <int O>
static hipError_t fused_packed(int mid_fmt, const FusedArgs &a, dim3 grid, size_t lds, hipStream_t s)
{
    const int pitch = easu_fast_pitch(a.cellsW);
    if (pitch == 0) return hipErrorInvalidValue;
    if (mid_fmt == FMT_RGBA16F) return pitch == 32 ? fused_packed_go<FMT_RGBA16F, O, 32>(a, grid, lds, s) : fused_packed_go<FMT_RGBA16F, O, 40>(a, grid, lds, s);
    if (mid_fmt == FMT_RGBA32F) return pitch == 32 ? fused_packed_go<FMT_RGBA32F, O, 32>(a, grid, lds, s) : fused_packed_go<FMT_RGBA32F, O, 40>(a, grid, lds, s);
    return hipErrorInvalidValue;
}

// ... and behind them, under cfg.reference_formats, a UNORM8 one (the outside-tile kernel only)
template <int O>
static hipError_t easu_outside_packed(int mid_fmt, const EasuArgs &a, dim3 grid, hipStream_t s)
{
    if (mid_fmt < 0) hipLaunchKernelGGL((ovrfsr_fast::easu_outside_kernel<I, O, -1>), grid, dim3(kThreads), 0, s, a);
    else if (mid_fmt == FMT_RGBA16F) hipLaunchKernelGGL((ovrfsr_fast::easu_outside_kernel<I, O, FMT_RGBA16F>), grid, dim3(kThreads), 0, s, a);
    else if (mid_fmt == FMT_RGBA32F) hipLaunchKernelGGL((ovrfsr_fast::easu_outside_kernel<I, O, FMT_RGBA32F>), grid, dim3(kThreads), 0, s, a);
    else if (mid_fmt == FMT_RGBA8) hipLaunchKernelGGL((ovrfsr_fast::easu_outside_kernel<I, O, FMT_RGBA8>), grid, dim3(kThreads), 0, s, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// the destination of a launch from packed words: RGBA8, RGBA16F or RGBA32F
#define OVRFSR_PACKED_OUT(FN, ...)                                  \
    switch (out_fmt) {                                              \
    case FMT_RGBA8: return FN<FMT_RGBA8>(__VA_ARGS__);              \
    case FMT_RGBA16F: return FN<FMT_RGBA16F>(__VA_ARGS__);          \
    case FMT_RGBA32F: return FN<FMT_RGBA32F>(__VA_ARGS__);          \
    default: return hipErrorInvalidValue;                           \
    }

hipError_t launch_easu_packed(int out_fmt, const EasuArgs &a, dim3 grid, hipStream_t s) { OVRFSR_PACKED_OUT(easu_packed, a, grid, s) }
hipError_t launch_fused_packed(int mid_fmt, int out_fmt, const FusedArgs &a, dim3 grid, size_t lds, hipStream_t s) { OVRFSR_PACKED_OUT(fused_packed, mid_fmt, a, grid, lds, s) }
hipError_t launch_easu_outside_packed(int mid_fmt, int out_fmt, const EasuArgs &a, dim3 grid, hipStream_t s) { OVRFSR_PACKED_OUT(easu_outside_packed, mid_fmt, a, grid, s) }

hipError_t tie_audit_read_packed(unsigned long long out[6], bool reset)
{
#ifdef OVRFSR_TIE_AUDIT
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ovrfsr_tie_audit), 6 * sizeof(unsigned long long));
    if (e == hipSuccess && reset) {
        const unsigned long long z[6] = {0, 0, 0, 0, 0, 0};
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_ovrfsr_tie_audit), z, sizeof z);
    }
    return e;
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
