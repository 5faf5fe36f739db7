// fsr_tile_records.inc -- the tile records of a gaze-capable ctx (header, "Eye-tracked foveation"), built on the device: included in
// fsr_kernels.hip behind fsr_hdr_domain.inc.  A re-aim uploads the tile lists; the 16-byte record of every list entry (tile_records.h: four
// fifths of what a re-aim would otherwise upload) is a pure integer function of the entry and the tap tables, which live on the device
// already.  One thread per list entry, the two eyes' list regions as blockIdx.y; one 16-byte store per entry.  One rule for every build;
// one instance per tile height -- 32 rows, and the 24 of NVScaler's groups.
#include "tile_records.h"

namespace ovrfsr_fast {

template <int TILE_H>
__global__ __launch_bounds__(256) void tile_records_kernel(ovrfsr::TileRecordsArgs a)
{
    static_assert(TILE_H == 32 || TILE_H == 24, "EASU / RCAS tiles, NVScaler groups");
    const uint32_t eye = blockIdx.y, i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n[eye]) return;
    const size_t e = (size_t)eye * a.regionEntries + i;
    OVRFSR_PTR(const uint32_t) lists = OVRFSR_PLANE(const uint32_t, a.lists, 2ull * a.regionEntries, 0, K_TILE_LIST);
    OVRFSR_PTR(uint32_t) recs = OVRFSR_PLANE(uint32_t, a.recs, 8ull * a.regionEntries, 0, K_TILE_REC);
    OVRFSR_PTR(const ovrfsr::BilinTap) bx = OVRFSR_PLANE(const ovrfsr::BilinTap, a.bilX, a.g.outW, 0, K_BIL_X);
    OVRFSR_PTR(const ovrfsr::BilinTap) by = OVRFSR_PLANE(const ovrfsr::BilinTap, a.bilY, a.g.outH, 0, K_BIL_Y);
    ovrfsr::TileRecordGrid g = a.g;
    g.tileW = (uint32_t)ovrfsr::kTileW; g.tileH = (uint32_t)TILE_H; // (what the launcher checked: constants to the divisions and products)
    const ovrfsr::TileRecord r = ovrfsr::tile_record(lists[e], g, bx, by);
    *OVRFSR_AT(uint4, recs + 4u * e) = make_uint4(r.w[0], r.w[1], r.w[2], r.w[3]);
}

} // namespace ovrfsr_fast

namespace ovrfsr {

hipError_t launch_tile_records(const TileRecordsArgs &a, hipStream_t s)
{
    launch_fresh();
    const uint32_t n = a.n[0] > a.n[1] ? a.n[0] : a.n[1];
    if (n == 0) return hipSuccess; // (both regions empty: nothing to build)
    if (n > a.regionEntries || a.g.tileW != (uint32_t)kTileW) return hipErrorInvalidValue;
    const dim3 grid((n + 255u) / 256u, 2, 1);
    if (a.g.tileH == 32u) return launch_kernel<ovrfsr_fast::tile_records_kernel<32>>(grid, dim3(256), 0, s, a);
    if (a.g.tileH == 24u) return launch_kernel<ovrfsr_fast::tile_records_kernel<24>>(grid, dim3(256), 0, s, a);
    return hipErrorInvalidValue;
}

} // namespace ovrfsr
