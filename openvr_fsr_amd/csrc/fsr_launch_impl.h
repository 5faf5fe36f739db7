// fsr_launch_impl.h -- what the launchers of the three kernel units (fsr_kernels.hip, fsr_packed_kernels.hip, nis_kernels.hip) are made of:
// the one launch site, the dynamic-LDS cap latch, the run-time format switches and the small pieces every launch_* shares.  Host only,
// templates and inline functions only, included by those units BEHIND their kernel text and by nothing else.  A unit holding the FSR kernel
// text (fsr_kernels.inc) defines OVRFSR_LAUNCH_FSR first and gets the launchers that name those kernels too.
// Nothing here may change a code object: a kernel is emitted where a launcher first names it, so the ORDER in which the launchers below (and
// the units' own) name their kernels is the order of the kernels in the code object, and the byte comparison of the code objects against
// the parent's (profiles/launch_layer.txt) is what holds it.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include "fsr_params.h"
#include "fsr_launch.h"
#include "fsr_formats.h"

namespace ovrfsr {

// HIP keeps a host thread's last error until somebody reads it, and a kernel launch reports its failure only there.  Every launch_*
// reads (= clears) it BEFORE launching, so that what it returns afterwards is its own launch's -- not an error the HOST's code left behind:
// a failed hipMalloc of the caller's, handled through its return value, used to fail the next frame as "EASU launch: out of memory"
// (tests/debug/stale_error.c, round 6).
inline void launch_fresh() { (void)hipGetLastError(); }

// a kernel argument as launched: checked builds put the launch's dynamic LDS size into the argument blocks that carry the field
#ifdef OVRFSR_BOUNDS
template <typename A, typename = decltype(A::ldsBytes)> inline A with_lds(A a, size_t lds, int) { a.ldsBytes = (uint32_t)lds; return a; }
template <typename A> inline const A &with_lds(const A &a, size_t, long) { return a; }
#else
template <typename A> inline const A &with_lds(const A &a, size_t, int) { return a; }
#endif

// THE launch site: every launcher's kernel goes through here, and what it returns is this launch's own error (launch_fresh).  The kernel
// is a REFERENCE template argument, so that `Kernel<<<...>>>` is the direct launch it would be with the kernel's name written out (through
// a pointer it is an indirect call to the compiler, and -fsanitize=function then checks the kernel's host handle as if it were code)
template <auto &Kernel, typename... A>
inline hipError_t launch_kernel(dim3 grid, dim3 block, size_t lds, hipStream_t s, const A &...args)
{
    hipLaunchKernelGGL(Kernel, grid, block, lds, s, with_lds(args, lds, 0)...);
    return hipGetLastError();
}

// ... for a kernel whose dynamic LDS can exceed the 64 KiB default cap (the fused kernels: EASU planes plus the 34x34 intermediate, of the
// 160 KiB per CU).  The attribute is per DEVICE (a one-process node driver holds one ctx per device, examples/bench_node.c): raised once per
// (kernel instantiation, device), latched with one bit per device ordinal; an error is returned before any launch.
template <auto &Kernel, typename... A>
inline hipError_t launch_kernel_big_lds(dim3 grid, dim3 block, size_t lds, hipStream_t s, const A &...args)
{
    static std::atomic<uint64_t> done{0};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const uint64_t bit = 1ull << (dev & 63);
    if (!(done.load(std::memory_order_acquire) & bit)) {
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(&Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFusedLdsMax);
        if (e != hipSuccess) return e;
        done.fetch_or(bit, std::memory_order_release);
    }
    return launch_kernel<Kernel>(grid, block, lds, s, args...);
}

// `return FN<in_fmt, out_fmt>(args)` of a launcher's run-time `in_fmt` / `out_fmt`.  OVRFSR_DISPATCH_OUT: the destinations RGBA8 / RGBA16F /
// RGBA32F of the source IN (falls through for any other); OVRFSR_DISPATCH_FMT: the nine pairs of those three, then TAIL --
// OVRFSR_TEN_BIT_PAIRS: R10G10B10A2, only what the reference's 10-bit path needs (10-bit in -> 10-bit out, PostProcessor.cpp:63-74) plus a
// float destination for un-quantised parity checks; OVRFSR_NO_TEN_BIT: kernels that are not built for it (fused, LDS-staged outside)
#define OVRFSR_DISPATCH_OUT(IN, FN, ...)                          \
    switch (out_fmt) {                                            \
    case FMT_RGBA8: return FN<IN, FMT_RGBA8>(__VA_ARGS__);        \
    case FMT_RGBA16F: return FN<IN, FMT_RGBA16F>(__VA_ARGS__);    \
    case FMT_RGBA32F: return FN<IN, FMT_RGBA32F>(__VA_ARGS__);    \
    default: break;                                               \
    }
#define OVRFSR_DISPATCH_FMT(TAIL, FN, ...)                                          \
    switch (in_fmt) {                                                               \
    case FMT_RGBA8: OVRFSR_DISPATCH_OUT(FMT_RGBA8, FN, __VA_ARGS__) break;          \
    case FMT_RGBA16F: OVRFSR_DISPATCH_OUT(FMT_RGBA16F, FN, __VA_ARGS__) break;      \
    case FMT_RGBA32F: OVRFSR_DISPATCH_OUT(FMT_RGBA32F, FN, __VA_ARGS__) break;      \
    default: break;                                                                 \
    }                                                                               \
    TAIL(FN, __VA_ARGS__)                                                           \
    return hipErrorInvalidValue;
#define OVRFSR_TEN_BIT_PAIRS(FN, ...)                                                                      \
    if (in_fmt == FMT_RGB10A2 && out_fmt == FMT_RGB10A2) return FN<FMT_RGB10A2, FMT_RGB10A2>(__VA_ARGS__); \
    if (in_fmt == FMT_RGB10A2 && out_fmt == FMT_RGBA32F) return FN<FMT_RGB10A2, FMT_RGBA32F>(__VA_ARGS__);
#define OVRFSR_NO_TEN_BIT(FN, ...)

// ---- the pieces every launch_* shares ------------------------------------------------------------------------------------------------------
// the argument block as the kernels want it: the caller's, plus what the launcher fills in
template <typename A> inline A prepared(const A &a_in) { A a = a_in; a.tilesXMagic = div_magic(a.tilesX); return a; }
// one workgroup per entry of the tile list where the launch has one, per tile of the grid otherwise; the batch as z
template <typename A> inline dim3 tile_grid(const A &a, uint32_t nListed, uint32_t batch) { return dim3(a.tileList ? nListed : a.tilesX * a.tilesY, 1, batch); }
inline bool is_masked(const MaskArgs &m) { return m.mode[0] != MASK_ALL_INSIDE || m.mode[1] != MASK_ALL_INSIDE; }
// the LDS-staged outside-tile kernel's block from an EASU or NVScaler launch's (launch_outside_staged fills in the rest)
template <typename A> inline OutsideArgs outside_args(const A &a, uint32_t debug)
{
    OutsideArgs o;
    o.v = a.v; o.tilesX = a.tilesX; o.tileList = a.tileList; o.tileRec = a.tileRec; o.bilX = a.bilX; o.bilY = a.bilY; o.debug = debug;
    o.lds_cols = a.outsideCols; o.lds_rows = a.outsideRows;
    return o;
}
// 1: every row of every image of the batch starts on an `align`-byte boundary (the copy kernels' `vec`: whole-vector loads or stores)
inline uint32_t rows_vectorizable(const void *p, uint32_t pitch, uint64_t stride, uint32_t batch, uint32_t align)
{
    return ((uintptr_t)p % align == 0 && pitch % align == 0 && (batch < 2 || stride % align == 0)) ? 1u : 0u;
}
// read (and optionally clear) the n <= 6 counters of a checked build's __device__ array on the current device
inline hipError_t read_counters(const void *symbol, unsigned long long *out, size_t n, bool reset)
{
    const unsigned long long z[6] = {0, 0, 0, 0, 0, 0};
    hipError_t e = n <= 6 ? hipDeviceSynchronize() : hipErrorInvalidValue;
    if (e == hipSuccess) e = hipMemcpyFromSymbol(out, symbol, n * sizeof z[0]);
    if (e == hipSuccess && reset) e = hipMemcpyToSymbol(symbol, z, n * sizeof z[0]);
    return e;
}

// ---- which intermediates exist --------------------------------------------------------------------------------------------------------------
// The intermediate has the pipeline format of the input (R8G8B8A8 -> UNORM8, RGBA16F and the R11G11B10F words that decode to it -> half:
// PostProcessor::IntermediateFormat with cfg.reference_formats = 0, this library's own rule; nothing writes a 10-bit one) or, with
// quantize_intermediate = 0, stays in float: those are the only (input, intermediate) pairs a ctx asks the FUSED kernel for, so only they
// are instantiated (12 of the 27 format triples of the fused and outside-tile kernels were dead weight in the library until round 4).
// Under cfg.reference_formats = 1 (DetermineOutputFormat, PostProcessor.cpp:63-74) a float or packed input has a UNORM8 intermediate: a
// ctx then asks for (RGBA16F | RGBA32F | R11G11B10F, RGBA8) too, of the outside-tile kernel only -- the fused kernel is refused for that
// pair at (re)build, none is built.  The outside-tile kernel also runs as the EASU pass alone (M < 0).
template <int I, int M> constexpr bool mid_reachable()
{
    return (M == (int)pipeline_format(I) && M != FMT_RGB10A2) || M == FMT_RGBA32F;
}
template <int I, int M> constexpr bool mid_reachable_outside()
{
    return M < 0 || mid_reachable<I, M>() || (M == FMT_RGBA8 && (pipeline_format(I) == FMT_RGBA16F || pipeline_format(I) == FMT_RGBA32F));
}

#ifdef OVRFSR_LAUNCH_FSR
// easu_fast_kernel at the fixed LDS pitch of the footprint (easu_kernel_pitch: 28, 32 or 40), of any source either unit holds
template <int I, int O, bool M>
inline hipError_t easu_fast_go(int pitch, const EasuArgs &a, dim3 grid, hipStream_t s)
{
    const size_t lds = (size_t)pitch * a.cellsH * 36 + (size_t)pitch * kLumPadRows * 4; // colour + analysis (float4) + luma planes + pad rows
    if (pitch == 28) return launch_kernel<ovrfsr_fast::easu_fast_kernel<I, O, 28, M>>(grid, dim3(kThreads), lds, s, a);
    if (pitch == 32) return launch_kernel<ovrfsr_fast::easu_fast_kernel<I, O, 32, M>>(grid, dim3(kThreads), lds, s, a);
    return launch_kernel<ovrfsr_fast::easu_fast_kernel<I, O, 40, M>>(grid, dim3(kThreads), lds, s, a);
}
// One dispatcher per kernel family, by the run-time intermediate format `mid_fmt`: the instance for the M of Ms... that it is, where the
// family has one of source I (hipErrorInvalidValue: not an (input, intermediate) pair a ctx produces).  Ms... lists every candidate, in the
// order in which the unit's code object holds the instances.
// the product fused kernel at the fixed LDS pitch of the footprint (easu_fast_pitch: 32 or 40) ...
template <int I, int M, int O>
struct FusedFast {
    static hipError_t go(const FusedArgs &a, dim3 grid, size_t lds, hipStream_t s)
    {
        const int pitch = easu_fast_pitch(a.cellsW);
        if (pitch == 32) return launch_kernel_big_lds<ovrfsr_fast::fused_kernel<I, M, O, 32, kFusedThreads>>(grid, dim3(kFusedThreads), lds, s, a);
        if (pitch == 40) return launch_kernel_big_lds<ovrfsr_fast::fused_kernel<I, M, O, 40, kFusedThreads>>(grid, dim3(kFusedThreads), lds, s, a);
        return hipErrorInvalidValue;
    }
};
// ... or whatever else the unit's Go<I, M, O>::go launches
template <template <int, int, int> class Go, int I, int M, int O, typename... A>
inline hipError_t fused_of_mid(const A &...args)
{
    if constexpr (mid_reachable<I, M>()) return Go<I, M, O>::go(args...);
    else return hipErrorInvalidValue;
}
template <template <int, int, int> class Go, int I, int O, int... Ms, typename... A>
inline hipError_t fused_go(int mid_fmt, const A &...args)
{
    hipError_t e = hipErrorInvalidValue;
    (..., (mid_fmt == Ms ? (void)(e = fused_of_mid<Go, I, Ms, O>(args...)) : (void)0)); // (a left fold: expanded first to last)
    return e;
}
// the per-pixel outside-tile kernel; mid_fmt < 0 (M = -1): the EASU pass alone
template <int I, int O, int M>
inline hipError_t easu_outside_of_mid(const EasuArgs &a, dim3 grid, hipStream_t s)
{
    if constexpr (mid_reachable_outside<I, M>()) return launch_kernel<ovrfsr_fast::easu_outside_kernel<I, O, M>>(grid, dim3(kThreads), 0, s, a);
    else return hipErrorInvalidValue;
}
template <int I, int O, int... Ms>
inline hipError_t easu_outside_go(int mid_fmt, const EasuArgs &a, dim3 grid, hipStream_t s)
{
    hipError_t e = hipErrorInvalidValue;
    (..., ((mid_fmt < 0 ? -1 : mid_fmt) == Ms ? (void)(e = easu_outside_of_mid<I, O, Ms>(a, grid, s)) : (void)0));
    return e;
}
#endif

} // namespace ovrfsr
