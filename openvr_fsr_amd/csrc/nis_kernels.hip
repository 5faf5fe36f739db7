// nis_kernels.hip -- instantiates the gfx950 NIS kernels (product + strict builds) and their launchers.
#include <hip/hip_runtime.h>
#include "fsr_params.h"
#include "fsr_launch.h"
#include "fsr_bounds.h"

namespace ovrfsr_fast {
#define OVRFSR_STRICT 0
#pragma clang fp contract(fast)
#include "fsr_device.inc"
#include "nis_kernels.inc"
#undef OVRFSR_STRICT
} // namespace ovrfsr_fast

namespace ovrfsr_strict {
#define OVRFSR_STRICT 1
#pragma clang fp contract(off)
#include "fsr_device.inc"
#include "nis_kernels.inc"
#undef OVRFSR_STRICT
} // namespace ovrfsr_strict
#pragma clang fp contract(on)

#include "fsr_launch_impl.h"

namespace ovrfsr {

template <int I, int O>
static hipError_t scaler_go(bool strict, const NisArgs &a, dim3 grid, size_t lds, hipStream_t s)
{
    const int pitch = nis_pitch(a.cellsW);
    if (pitch == 32) {
        if (strict) return launch_kernel<ovrfsr_strict::nis_scaler_kernel<I, O, 32>>(grid, dim3(kThreads), lds, s, a);
        return launch_kernel<ovrfsr_fast::nis_scaler_kernel<I, O, 32>>(grid, dim3(kThreads), lds, s, a);
    }
    if (pitch == 40) {
        if (strict) return launch_kernel<ovrfsr_strict::nis_scaler_kernel<I, O, 40>>(grid, dim3(kThreads), lds, s, a);
        return launch_kernel<ovrfsr_fast::nis_scaler_kernel<I, O, 40>>(grid, dim3(kThreads), lds, s, a);
    }
    return hipErrorInvalidValue;
}
template <int I, int O>
static hipError_t sharpen_go(bool strict, const NisArgs &a, dim3 grid, hipStream_t s)
{
    if (strict) return launch_kernel<ovrfsr_strict::nis_sharpen_kernel<I, O>>(grid, dim3(kThreads), 0, s, a);
    return launch_kernel<ovrfsr_fast::nis_sharpen_kernel<I, O>>(grid, dim3(kThreads), 0, s, a);
}

template <int I, int O>
static hipError_t nis_outside_go(const NisArgs &a, dim3 grid, hipStream_t s)
{
    return launch_kernel<ovrfsr_fast::nis_outside_kernel<I, O>>(grid, dim3(kThreads), 0, s, a);
}

hipError_t launch_nis_outside(int in_fmt, int out_fmt, const NisArgs &a_in, uint32_t nGroups, uint32_t batch, hipStream_t s)
{
    launch_fresh();
    const NisArgs a = prepared(a_in);
    if (!a.tileList || nGroups == 0) return hipErrorInvalidValue;
    if (a.bilX && a.bilY && a.tileRec && outside_staged_ok(a.v, in_fmt)) // no records: the per-pixel kernel below needs none
        return launch_outside_staged(24, in_fmt, FMT_RGBA32F, out_fmt, outside_args(a, a.reserved1 != 0.0f ? 1u : 0u), nGroups, batch, s);
    const dim3 grid(nGroups, 1, batch);
    OVRFSR_DISPATCH_FMT(OVRFSR_TEN_BIT_PAIRS, nis_outside_go, a, grid, s)
}

hipError_t launch_nis_scaler(int prec, int in_fmt, int out_fmt, const NisArgs &a_in, uint32_t batch, hipStream_t s, uint32_t nGroups)
{
    launch_fresh();
    const NisArgs a = prepared(a_in);
    if (prec != PREC_FP32 && prec != PREC_FP32_STRICT) return hipErrorInvalidValue;
    const size_t lds = nis_scaler_lds_bytes(a.cellsW, a.cellsH);
    OVRFSR_DISPATCH_FMT(OVRFSR_TEN_BIT_PAIRS, scaler_go, prec == PREC_FP32_STRICT, a, tile_grid(a, nGroups, batch), lds, s)
}

#ifdef OVRFSR_BOUNDS
hipError_t bounds_read_nis(unsigned long long *out, bool reset) { return ovrfsr_chk::read_counts(out, reset); }
#else
hipError_t bounds_read_nis(unsigned long long *, bool) { return hipErrorNotSupported; }
#endif

hipError_t launch_nis_sharpen(int prec, int in_fmt, int out_fmt, const NisArgs &a_in, uint32_t batch, hipStream_t s)
{
    launch_fresh();
    const NisArgs a = prepared(a_in);
    if (prec != PREC_FP32 && prec != PREC_FP32_STRICT) return hipErrorInvalidValue;
    const dim3 grid(a.tilesX * a.tilesY, 1, batch);
    OVRFSR_DISPATCH_FMT(OVRFSR_TEN_BIT_PAIRS, sharpen_go, prec == PREC_FP32_STRICT, a, grid, s)
}

} // namespace ovrfsr
