// tile_records.h -- one record of the persistent outside-tile kernel (OutsideArgs::tileRec), from a tile index and the tap tables.  A pure
// integer function with one definition and two callers: the planner's outside_records (pipeline_plan.cpp, host) and tile_records_kernel
// (fsr_tile_records.inc, device), which builds the records of a gaze-capable ctx behind every list upload.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OVRFSR_HD __host__ __device__
#else
#define OVRFSR_HD
#endif

namespace ovrfsr {

struct TileRecord {
    uint32_t w[4]; // ox0 | oy0 << 16, (X0 + 1) | (Y0 + 1) << 16, colsN | rowsN << 8, 0
};

// what a record is computed from besides the tile: the grid, the output size and the caps of the footprint (Plan::outsideCols, and
// Plan::outsideRows of the grid's tile height -- 32 rows, or NVScaler's 24)
struct TileRecordGrid {
    uint32_t tx, tileW, tileH;
    uint32_t outW, outH;
    uint32_t colsCap, rowsCap;
};

// Tile origin, footprint origin (first column / row tap) and extent ([first tap, last tap + 1], what the kernel used to fetch through a chain
// of dependent scalar loads: tile index -> tap tables).  `bx`, `by`: the column and row taps, anything indexable that yields a BilinTap
// (a plain pointer on the host, an fsr_bounds.h accessor in the kernel).  t < tx * ty.
template <class TapsX, class TapsY>
OVRFSR_HD inline TileRecord tile_record(uint32_t t, const TileRecordGrid &g, const TapsX &bx, const TapsY &by)
{
    const uint32_t tyi = t / g.tx, txi = t - tyi * g.tx;
    const uint32_t ox0 = txi * g.tileW, oy0 = tyi * g.tileH;
    const uint32_t oxLast = ox0 + g.tileW - 1 < g.outW - 1 ? ox0 + g.tileW - 1 : g.outW - 1;
    const uint32_t oyLast = oy0 + g.tileH - 1 < g.outH - 1 ? oy0 + g.tileH - 1 : g.outH - 1;
    const int X0 = bx[ox0].i0, Y0 = by[oy0].i0;
    const int cols = bx[oxLast].i0 + 2 - X0, rows = by[oyLast].i0 + 2 - Y0;
    const int colsN = cols < (int)g.colsCap ? cols : (int)g.colsCap;
    const int rowsN = rows < (int)g.rowsCap ? rows : (int)g.rowsCap;
    TileRecord r;
    r.w[0] = ox0 | (oy0 << 16);
    r.w[1] = (uint32_t)(X0 + 1) | ((uint32_t)(Y0 + 1) << 16);
    r.w[2] = (uint32_t)colsN | ((uint32_t)rowsN << 8);
    r.w[3] = 0u;
    return r;
}

} // namespace ovrfsr
