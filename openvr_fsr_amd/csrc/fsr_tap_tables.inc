// fsr_tap_tables.inc -- the tap tables of a rescale-capable ctx (header, "Dynamic resolution"), refilled on the device: included in
// fsr_kernels.hip behind fsr_tile_records.inc.  When only the input size moves, the tables keep their layout -- it is sized by the output
// alone -- and every entry is a pure function of its index and the two sizes (bilin_taps.h: the rule the planner's tap_tables evaluates on
// the host, rounding for rounding).  One thread per entry, one 8-byte store each: the column taps, the copies of the last column tap up to
// tapYOff, the row taps.  It runs ahead of tile_records_kernel in stream order, which reads what it wrote.  One rule for every build.
#include "bilin_taps.h"

namespace ovrfsr_fast {

// (a template, like tile_records_kernel: the kernels of this unit are emitted where a launcher first names them, and a plain kernel would
// take bgra_to_rgba_kernel's place at the end of the code object)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void tap_tables_kernel(ovrfsr::TapTablesArgs a)
{
    const uint32_t i = blockIdx.x * (uint32_t)THREADS + threadIdx.x;
    if (i >= a.tapYOff + a.outH) return;
    const ovrfsr::BilinTap t = ovrfsr::tap_table_entry(i, a.outW, a.outH, a.inW, a.inH, a.tapYOff);
    const uint2 words = make_uint2((uint32_t)t.i0, __float_as_uint(t.frac));
    if (i < a.tapYOff) { // (the padding belongs to the column table: every entry of it is written)
        OVRFSR_PTR(ovrfsr::BilinTap) bx = OVRFSR_PLANE(ovrfsr::BilinTap, a.taps, a.tapYOff, 0, K_BIL_X);
        *OVRFSR_AT(uint2, bx + i) = words;
    } else {
        OVRFSR_PTR(ovrfsr::BilinTap) by = OVRFSR_PLANE(ovrfsr::BilinTap, a.taps + a.tapYOff, a.outH, 0, K_BIL_Y);
        *OVRFSR_AT(uint2, by + (i - a.tapYOff)) = words;
    }
}

} // namespace ovrfsr_fast

namespace ovrfsr {

hipError_t launch_tap_tables(const TapTablesArgs &a, hipStream_t s)
{
    launch_fresh();
    if (!a.taps || a.outW == 0 || a.outH == 0 || a.inW == 0 || a.inH == 0 || a.tapYOff < a.outW) return hipErrorInvalidValue;
    const uint32_t n = a.tapYOff + a.outH;
    return launch_kernel<ovrfsr_fast::tap_tables_kernel<256>>(dim3((n + 255u) / 256u), dim3(256), 0, s, a);
}

} // namespace ovrfsr
