// pipeline_plan.cpp -- see pipeline_plan.h.  Host arithmetic only: this unit includes no HIP header and links against constants.cpp and
// nis_config.cpp alone.  Reference: src/postprocess/PostProcessor.cpp (PrepareResources and what it calls).
#include "pipeline_plan.h"
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <utility>
#include "bilin_taps.h"
#include "fsr_formats.h"
#include "fsr_sizes.h"

namespace ovrfsr {

namespace {

enum RefusalId {
    R_OUTPUT_SIZE, R_STAGE_MASK, R_SHARPEN_ONLY_SIZE, R_PRECISION, R_EXACT_NIS, R_EXACT_FUSED_ASKED, R_EXACT_FLOAT_MID, R_EXACT_SOURCE,
    R_NIS_SCALE, R_NIS_LDS, R_EASU_LDS, R_FUSED_TEN_BIT, R_FUSED_FLOAT_REFERENCE, R_FUSED_LDS, R_EXACT_FUSED,
    R_DEST_INPUT_ONLY, R_DEST_TEN_BIT_PAIR, R_DEST_TEN_BIT_MID, R_DEST_EXACT, R_COUNT
};
// in the order they are tested.  Status and text are part of the library's behaviour (tests/golden/launch_forms_parent.json).
const Refusal kRefusals[R_COUNT] = {
    {OVRFSR_ERR_INVALID_ARGUMENT, "output size is zero or beyond 16384 texels (render_scale must be finite and > 0)", true},
    {OVRFSR_ERR_INVALID_ARGUMENT, "bad stage_mask", true},
    {OVRFSR_ERR_INVALID_ARGUMENT, "sharpen-only needs output size == input size", true},
    {OVRFSR_ERR_INVALID_ARGUMENT, "unknown precision", true},
    // exact stores (header): promised where the sharpen stage is RCAS from RGBA8 to RGBA8 behind a quantised intermediate; every other
    // configuration with a sharpen stage is refused -- nothing in it promises the strict build's bytes, so the mode must not pretend to
    {OVRFSR_ERR_UNSUPPORTED, "precision FP32_EXACT: NIS has no exact-stores form (use_nis)", true},
    {OVRFSR_ERR_UNSUPPORTED, "precision FP32_EXACT: the fused kernel has no exact-stores form (fused = 1)", true},
    {OVRFSR_ERR_UNSUPPORTED, "precision FP32_EXACT: RCAS must read a UNORM8 intermediate (quantize_intermediate = 0)", true},
    {OVRFSR_ERR_UNSUPPORTED, "precision FP32_EXACT: RCAS must read RGBA8 (a half, float or 10-bit intermediate or input promises no exact bytes)", true},
    // (the reference ignores a `false` result of NVScalerUpdateConfig and dispatches with a half-filled block; that is undefined there, so it is an error here)
    {OVRFSR_ERR_UNSUPPORTED, "NIS scales 1x..2x only (NVScalerUpdateConfig returned false)", true},
    {OVRFSR_ERR_UNSUPPORTED, "NIS tile does not fit LDS", true},
    {OVRFSR_ERR_UNSUPPORTED, "scale ratio needs more LDS than one tile may use", true},
    {OVRFSR_ERR_UNSUPPORTED, "the fused kernel is not built for RGB10A2 images", true},
    {OVRFSR_ERR_UNSUPPORTED, "the fused kernel is not built for float images under reference_formats (UNORM8 intermediate of a float source)", true},
    {OVRFSR_ERR_UNSUPPORTED, "fused kernel: tile footprint does not fit LDS at this scale", true},
    {OVRFSR_ERR_UNSUPPORTED, "precision FP32_EXACT: the fused kernel has no exact-stores form", true},
    // the destination's: known only once the call names its `out`.  (Of the input-only formats only single-sample BGRA8 gets this far:
    // CheckImage refuses R11G11B10F and multisampled destinations.)
    {OVRFSR_ERR_UNSUPPORTED, input_only(OVRFSR_FORMAT_BGRA8_UNORM), false},
    {OVRFSR_ERR_UNSUPPORTED, "RGB10A2 images pair with an RGB10A2 (or RGBA32F) destination only", false},
    {OVRFSR_ERR_UNSUPPORTED, "RGB10A2 pipelines keep a 10-bit intermediate (quantize_intermediate = 1)", false},
    {OVRFSR_ERR_UNSUPPORTED, "precision FP32_EXACT: RCAS must write RGBA8 (a half, float or 10-bit destination promises no exact bytes)", true},
};

// a*b+c with two roundings, identical to the kernels' mad_unfused (separate statements)
inline float mad2(float a, float b, float c)
{
    volatile float t = a * b;
    return t + c;
}

inline float con_float(uint32_t bits)
{
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}

// LDS footprints of the EASU kernels' tiles (cells per axis, max over tiles)
void easu_footprints(Plan &p)
{
    easu_con(p.easuCon, (float)p.inputWidth, (float)p.inputHeight, (float)p.inputWidth, (float)p.inputHeight, (float)p.outputWidth, (float)p.outputHeight);
    const float sx = con_float(p.easuCon[0]), sy = con_float(p.easuCon[1]), cx = con_float(p.easuCon[2]), cy = con_float(p.easuCon[3]);
    // LDS footprint of one 32x32 output tile: f-texel of first and last pixel, +1/+2 apron.  `pairs`: the product EASU kernel resolves rows in
    // PAIRS (ly, ly + 1), ly even, and evaluates the second pixel of the last pair even when its row lies behind the image (only its store is
    // guarded): the footprint covers that row too.  (Until round 6 it did not: where the LAST, partial tile row defines the extent -- an image of
    // a single tile row with an odd height -- the discarded pixel read up to two cell rows past the colour / analysis planes, into the next
    // plane of the same workgroup.  Found by the fuzz seeds run against the checked build, seed 162312: profiles/r06_bounds.txt.)
    auto extent = [](uint32_t outN, int tile, float s, float c, bool pairs) {
        int best = 0;
        for (uint32_t o0 = 0; o0 < outN; o0 += tile) {
            uint32_t o1 = o0 + tile - 1 < outN ? o0 + tile - 1 : outN - 1;
            if (pairs) o1 |= 1u; // the partner row of the last pair (inside the tile: tile heights are even)
            int f0 = (int)std::floor(mad2((float)o0, s, c)), f1 = (int)std::floor(mad2((float)o1, s, c));
            best = f1 - f0 + 4 > best ? f1 - f0 + 4 : best;
        }
        return best;
    };
    p.cellsW = extent(p.outputWidth, kTileW, sx, cx, false);
    p.cellsH = extent(p.outputHeight, kTileH, sy, cy, true);
    // fused kernel: EASU runs on the tile plus a 1-pixel ring, origin at pixel (o0 - 1)
    auto extentRing = [](uint32_t outN, int tile, float s, float c) {
        int best = 0;
        for (uint32_t o0 = 0; o0 < outN; o0 += tile) {
            uint32_t o1 = o0 + tile < outN ? o0 + tile : outN - 1;
            int f0 = (int)std::floor(mad2((float)o0 - 1.0f, s, c)), f1 = (int)std::floor(mad2((float)o1, s, c));
            best = f1 - f0 + 4 > best ? f1 - f0 + 4 : best;
        }
        return best;
    };
    p.fusedCellsW = extentRing(p.outputWidth, kTileW, sx, cx);
    p.fusedCellsH = extentRing(p.outputHeight, kTileH, sy, cy);
}

// LDS footprint of one NVScaler group (32x24: p.grid)
void nis_footprints(Plan &p)
{
    auto extent = [](uint32_t outN, int blk, float s) {
        int best = 0;
        for (uint32_t o0 = 0; o0 < outN; o0 += blk) {
            uint32_t o1 = o0 + blk - 1 < outN ? o0 + blk - 1 : outN - 1;
            int f0 = (int)std::floor(mad2(0.5f + (float)o0, s, -0.5f)), f1 = (int)std::floor(mad2(0.5f + (float)o1, s, -0.5f));
            best = f1 - f0 + 7 > best ? f1 - f0 + 7 : best; // 6-tap support (+2/+3) and the edge-map ring (+1)
        }
        return best;
    };
    p.nisCellsW = extent(p.outputWidth, (int)p.grid.tileW, p.nis.kScaleX);
    p.nisCellsH = extent(p.outputHeight, (int)p.grid.tileH, p.nis.kScaleY);
}

// o/outW, o/outH of the bilinear fallback as a multiply and two FMAs: verify against IEEE division for every o
void reciprocals(Plan &p)
{
    auto check = [](uint32_t n, float &rn) {
        volatile float r = 1.0f / (float)n;
        rn = r;
        for (uint32_t o = 0; o < n; ++o) {
            const float q0 = (float)o * rn;
            const float rem = std::fma(-q0, (float)n, (float)o);
            volatile float want = (float)o / (float)n;
            if (std::fma(rem, rn, q0) != want) return false;
        }
        return true;
    };
    const bool okW = check(p.outputWidth, p.rcpOut[0]), okH = check(p.outputHeight, p.rcpOut[1]);
    p.rcpExact = okW && okH;
}

// column / row taps of the bilinear fallback / NIS DirectCopy (SampleLevel at pos/outSize, 8-bit sub-texel snap): same IEEE
// operations as fsr_device.inc's bilinear_uv / fixed8, evaluated once per column and row instead of per pixel
// Layout: [ow column taps | copies of the last column tap up to a multiple of the tile width | oh row taps | 64 spare entries].
// The staged outside-tile kernel loads the column taps of every pixel QUAD of a 32-wide tile (outside_staged_kernel::issue_taps);
// the quads on and behind the last column must find VALID taps -- their pixels are never stored, but the taps index the kernel's
// LDS plane.  (Until round 6 the row taps followed the column taps directly and that quad read row taps as column taps:
// out-of-plane LDS reads whose values were discarded -- found by the checked build, profiles/r06_bounds.txt.)
void tap_tables(Plan &p)
{
    const uint32_t ow = p.outputWidth, oh = p.outputHeight;
    std::vector<BilinTap> &taps = p.taps;
    p.tapYOff = (ow + (uint32_t)kTileW - 1u) & ~((uint32_t)kTileW - 1u);
    taps.assign((size_t)p.tapYOff + oh + 64, BilinTap{0, 0.0f});
    auto fill = [](BilinTap *t, uint32_t outN, uint32_t inN) {
        for (uint32_t o = 0; o < outN; ++o) t[o] = bilin_tap(o, outN, inN); // (bilin_taps.h: the rule tap_tables_kernel evaluates too)
    };
    fill(taps.data(), ow, p.inputWidth);
    for (uint32_t o = ow; o < p.tapYOff; ++o) taps[o] = taps[ow - 1];
    fill(taps.data() + p.tapYOff, oh, p.inputHeight);
    // largest [first tap, last tap + 1] span of a tile: the LDS plane of the staged outside-tile kernel
    auto span = [](const BilinTap *t, uint32_t outN, uint32_t tile) {
        int best = 2;
        for (uint32_t o0 = 0; o0 < outN; o0 += tile) {
            const uint32_t o1 = o0 + tile - 1 < outN ? o0 + tile - 1 : outN - 1;
            best = std::max(best, t[o1].i0 + 2 - t[o0].i0);
        }
        return (uint32_t)best;
    };
    p.outsideCols = span(taps.data(), ow, 32);
    p.outsideRows[0] = span(taps.data() + p.tapYOff, oh, 32);
    p.outsideRows[1] = span(taps.data() + p.tapYOff, oh, 24);
}

// Block b of a launch runs on XCD b % 8, each XCD with a private L2: entry b of a work list of n row-major items is item
// xcd_source(b, n), which hands every XCD a contiguous raster run of the list (the n % 8 trailing entries keep their place).
inline uint32_t xcd_source(uint32_t b, uint32_t n)
{
    const uint32_t full = n & ~7u;
    return b < full ? (b & 7u) * (full >> 3) + (b >> 3) : b;
}

// ---- the hidden-area rule (header, ovrfsr_hidden_tiles) ------------------------------------------------------------------------------
// One triangle in 1/256-pixel fixed point, with the pixels whose centres its bounding box holds (clipped to its mesh's columns and the image)
struct HiddenTri {
    int64_t x[3], y[3];
    int64_t px0, px1, py0, py1; // inclusive pixel ranges; empty where px0 > px1 or py0 > py1
};

// u, v -> fixed point: clamped to [-4, 4] in double, then floor(u * n * 256 + 0.5)
inline int64_t hidden_fixed(float c, uint32_t n)
{
    const double d = std::min(4.0, std::max(-4.0, (double)c));
    return (int64_t)std::floor(d * (double)n * 256.0 + 0.5);
}
inline int64_t floor_div256(int64_t a) { return a >= 0 ? a / 256 : -((-a + 255) / 256); }

// the triangles of one mesh that can cover a pixel of columns [x0, x1): zero-area ones and empty boxes are dropped here
void hidden_triangles(const float *uv, uint32_t n, uint32_t x0, uint32_t x1, uint32_t outH, std::vector<HiddenTri> &tris)
{
    if (!uv || x1 <= x0) return;
    for (uint32_t i = 0; i < n; ++i) {
        HiddenTri t;
        for (int k = 0; k < 3; ++k) {
            t.x[k] = hidden_fixed(uv[6 * i + 2 * k], x1 - x0) + 256 * (int64_t)x0;
            t.y[k] = hidden_fixed(uv[6 * i + 2 * k + 1], outH);
        }
        const int64_t area = (t.x[1] - t.x[0]) * (t.y[2] - t.y[0]) - (t.y[1] - t.y[0]) * (t.x[2] - t.x[0]);
        if (area == 0) continue; // covers nothing
        const int64_t xa = std::min({t.x[0], t.x[1], t.x[2]}), xb = std::max({t.x[0], t.x[1], t.x[2]});
        const int64_t ya = std::min({t.y[0], t.y[1], t.y[2]}), yb = std::max({t.y[0], t.y[1], t.y[2]});
        // pixel centres 256 p + 128 inside [a, b]: p >= ceil((a - 128) / 256), p <= floor((b - 128) / 256)
        t.px0 = std::max<int64_t>(floor_div256(xa - 128 + 255), x0); t.px1 = std::min<int64_t>(floor_div256(xb - 128), (int64_t)x1 - 1);
        t.py0 = std::max<int64_t>(floor_div256(ya - 128 + 255), 0); t.py1 = std::min<int64_t>(floor_div256(yb - 128), (int64_t)outH - 1);
        if (t.px0 <= t.px1 && t.py0 <= t.py1) tris.push_back(t);
    }
}

} // namespace

void hidden_tiles(const float *left, uint32_t leftTriangles, const float *right, uint32_t rightTriangles, bool shared, uint32_t outW, uint32_t outH,
                  uint32_t tileW, uint32_t tileH, uint8_t *hidden)
{
    const uint32_t tx = (outW + tileW - 1) / tileW, ty = (outH + tileH - 1) / tileH;
    std::fill(hidden, hidden + (size_t)tx * ty, (uint8_t)0);
    std::vector<HiddenTri> tris;
    if (shared) {
        hidden_triangles(left, leftTriangles, 0, outW / 2, outH, tris);
        hidden_triangles(right, rightTriangles, outW / 2, outW, outH, tris);
    } else {
        hidden_triangles(left, leftTriangles, 0, outW, outH, tris);
    }
    if (tris.empty()) return;
    // one band of tile rows at a time: a byte per pixel of the band, every triangle rasterised over (its box & the band) with the three
    // edge functions stepped along the row -- the work follows the boxes' area, the memory one band
    std::vector<uint8_t> cover;
    for (uint32_t band = 0; band < ty; ++band) {
        const int64_t y0 = (int64_t)band * tileH, y1 = std::min<int64_t>(y0 + tileH, outH) - 1;
        bool touched = false;
        for (const HiddenTri &t : tris) {
            const int64_t ya = std::max(t.py0, y0), yb = std::min(t.py1, y1);
            if (ya > yb) continue;
            if (!touched) { cover.assign((size_t)outW * (size_t)(y1 - y0 + 1), 0); touched = true; }
            for (int64_t y = ya; y <= yb; ++y) {
                uint8_t *row = cover.data() + (size_t)(y - y0) * outW;
                const int64_t cx = 256 * t.px0 + 128, cy = 256 * y + 128;
                int64_t e[3], step[3];
                for (int k = 0; k < 3; ++k) {
                    const int k1 = (k + 1) % 3;
                    const int64_t dx = t.x[k1] - t.x[k], dy = t.y[k1] - t.y[k];
                    e[k] = dx * (cy - t.y[k]) - dy * (cx - t.x[k]);
                    step[k] = -256 * dy;
                }
                for (int64_t x = t.px0; x <= t.px1; ++x) {
                    // either winding, edges inclusive
                    if ((e[0] >= 0 && e[1] >= 0 && e[2] >= 0) || (e[0] <= 0 && e[1] <= 0 && e[2] <= 0)) row[x] = 1;
                    e[0] += step[0]; e[1] += step[1]; e[2] += step[2];
                }
            }
        }
        if (!touched) continue;
        const uint32_t rows = (uint32_t)(y1 - y0 + 1);
        for (uint32_t txi = 0; txi < tx; ++txi) {
            const uint32_t xa = txi * tileW, xb = std::min(xa + tileW, outW);
            bool all = true;
            for (uint32_t r = 0; r < rows && all; ++r) {
                const uint8_t *row = cover.data() + (size_t)r * outW;
                for (uint32_t x = xa; x < xb && all; ++x) all = row[x] != 0;
            }
            hidden[(size_t)band * tx + txi] = all ? 1 : 0;
        }
    }
}

namespace {

// ---- the tile lists ----------------------------------------------------------------------------------------------------------------------
// The radius mask moves only where the host moves it -- never on a ctx without a gaze, per frame at most on one with eye tracking
// (ovrfsr_set_gaze) --, so the tiles are sorted on the host: tiles with at least one mask group inside the radius (EASU kernel, LDS-staged)
// and tiles entirely outside (bilinear only, LDS-free kernel); under a hidden-area mesh, the tiles no lens shows are in neither list.
// tile_lists() builds them in the steps below, each with one job; they run at plan time, and steps 1-5 again when a gaze re-aims the
// mask (reaim_pipeline).

// one eye's tiles by class, each in raster order
struct TileClasses {
    std::vector<uint32_t> inside, outside, hidden;
};

// one eye per texture: each eye's own mesh; a shared side-by-side texture: one map of both halves, the same for both "eyes"
HiddenMaps hidden_maps(const Plan &p, const HiddenArea &mesh)
{
    const TileGrid &g = p.grid;
    HiddenMaps maps;
    maps.eye[0].resize(g.tiles());
    if (p.onlyOneEye) {
        maps.eye[1].resize(g.tiles());
        for (int eye = 0; eye < 2; ++eye)
            hidden_tiles(mesh.uv[eye], mesh.triangles[eye], nullptr, 0, false, p.outputWidth, p.outputHeight, g.tileW, g.tileH, maps.eye[eye].data());
    } else {
        hidden_tiles(mesh.uv[0], mesh.triangles[0], mesh.uv[1], mesh.triangles[1], true, p.outputWidth, p.outputHeight, g.tileW, g.tileH, maps.eye[0].data());
        maps.eye[1] = maps.eye[0];
    }
    return maps;
}

// Step 1.  `hidden` (empty: none) takes its tiles out first.  `byRadius` = false (no mixed mask: the lists exist for the mesh alone): every
// other tile is an "inside" tile, whatever the radius -- the kernel that runs on it is the one the launch without lists runs, mask test included.
// Only the groups the reference dispatches count, ceil(outW / groupW) x ceil(outH / groupH) of them: a partial last tile may hold a group
// column or row that starts behind the image, and with the disc's centre behind that edge too such a group is nearer to it than the tile's
// real ones -- testing it called tiles inside whose every pixel is outside.
TileClasses classify_tiles(const TileGrid &g, uint32_t outW, uint32_t outH, const uint32_t centre[4], uint32_t r2, bool byRadius,
                           const std::vector<uint8_t> &hidden)
{
    const uint32_t gpx = g.tileW / g.groupW, gpy = g.tileH / g.groupH; // mask groups per tile
    TileClasses c;
    for (uint32_t t = 0; t < g.tiles(); ++t) {
        if (!hidden.empty() && hidden[t]) { c.hidden.push_back(t); continue; }
        const uint32_t tyi = t / g.tx, txi = t - tyi * g.tx;
        bool any = !byRadius;
        for (uint32_t k = 0; k < gpx * gpy && !any; ++k) {
            const uint32_t gx = gpx * txi + (k % gpx), gy = gpy * tyi + (k / gpx);
            if (gx * g.groupW >= outW || gy * g.groupH >= outH) continue;
            const uint32_t cx = gx * g.groupW + g.groupW / 2, cy = gy * g.groupH + g.groupH / 2;
            const uint32_t ax = centre[0] - cx, ay = centre[1] - cy, bx = centre[2] - cx, by = centre[3] - cy;
            any = (ax * ax + ay * ay <= r2) || (bx * bx + by * by <= r2);
        }
        (any ? c.inside : c.outside).push_back(t);
    }
    return c;
}

// Step 2.  What RCAS walks, in raster order: the inside tiles -- in the two-pass form under a mesh (`everyVisibleTile`; without a mesh that
// form runs RCAS over the whole image, with no list), every tile that is not hidden.
std::vector<uint32_t> rcas_tiles(const TileClasses &c, bool everyVisibleTile)
{
    std::vector<uint32_t> r = c.inside;
    if (everyVisibleTile) {
        r.insert(r.end(), c.outside.begin(), c.outside.end());
        std::sort(r.begin(), r.end());
    }
    return r;
}

// The ring's candidates, in the order the ring lists them: the outside tiles -- their intermediate is nobody else's.  In the two-kernel forms
// under a mesh a hidden tile next to a tile RCAS processes joins them (`hiddenToo`: mask-sorted), so that EASU still writes the intermediate
// texels RCAS's cross taps read (a hidden ring tile is still a skipped one: nothing of the destination is written there).  Two-pass under a
// mesh (`rcasOwnList`): the outside tiles' intermediate is the outside-tile launch's, so the candidates are the hidden tiles only.
std::vector<uint32_t> ring_candidates(const TileClasses &c, bool rcasOwnList, bool hiddenToo)
{
    std::vector<uint32_t> v;
    if (!rcasOwnList) v = c.outside;
    if (rcasOwnList || hiddenToo) v.insert(v.end(), c.hidden.begin(), c.hidden.end());
    return v;
}

// Step 3.  The candidates that share an edge with a tile of `rcas`, in the candidates' order: RCAS's cross taps reach one pixel across a tile
// edge, so the EASU launch has to write the intermediate there too.
std::vector<uint32_t> ring_tiles(const TileGrid &g, const std::vector<uint32_t> &rcas, const std::vector<uint32_t> &candidates)
{
    const uint32_t tx = g.tx, ty = g.ty;
    std::vector<uint8_t> isIn(g.tiles(), 0);
    for (uint32_t t : rcas) isIn[t] = 1;
    std::vector<uint32_t> ring;
    for (uint32_t t : candidates) {
        const uint32_t tyi = t / tx, txi = t - tyi * tx;
        if ((txi > 0 && isIn[t - 1]) || (txi + 1 < tx && isIn[t + 1]) || (tyi > 0 && isIn[t - tx]) || (tyi + 1 < ty && isIn[t + tx])) ring.push_back(t);
    }
    return ring;
}

// Step 4.  RCAS on RGBA8 walks spans, not tiles (rcas_dpp_kernel<.., true>): per 32-row band, runs of adjacent tiles of `rcas` (row-major
// here), cut into the kernel's 62-column segments {x0 | tileY << 16, xEnd}, appended to `spans`.  Every XCD then gets a contiguous raster run
// of segments (xcd_source), so that the 128-byte lines two neighbouring segments share, and the rows two bands share, are fetched once.
// *first, *count: where the eye's segments start in `spans` (in segments) and how many they are.
void rcas_spans(const TileGrid &g, uint32_t outW, const std::vector<uint32_t> &rcas, std::vector<uint32_t> &spans, size_t *first, uint32_t *count)
{
    const size_t off = *first = spans.size() / 2;
    for (size_t i = 0; i < rcas.size();) {
        size_t j = i;
        while (j + 1 < rcas.size() && rcas[j + 1] == rcas[j] + 1 && (rcas[j + 1] / g.tx) == (rcas[i] / g.tx)) ++j;
        const uint32_t tyi = rcas[i] / g.tx, xa = (rcas[i] - tyi * g.tx) * g.tileW;
        const uint32_t xb = std::min((rcas[j] - tyi * g.tx + 1) * g.tileW, outW);
        for (uint32_t x0 = xa; x0 < xb; x0 += kRcasDppTileW) {
            spans.push_back(x0 | (tyi << 16));
            spans.push_back(std::min(x0 + (uint32_t)kRcasDppTileW, xb));
        }
        i = j + 1;
    }
    const uint32_t n = *count = (uint32_t)(spans.size() / 2 - off);
    std::vector<uint32_t> r(2 * (size_t)n);
    for (uint32_t b = 0; b < n; ++b) {
        const size_t src = off + xcd_source(b, n);
        r[2 * (size_t)b] = spans[2 * src]; r[2 * (size_t)b + 1] = spans[2 * src + 1];
    }
    std::copy(r.begin(), r.end(), spans.begin() + 2 * off);
}

// Step 5.  Writes one eye's part of the plan: its segments behind what p.lists holds already, with their counts and offsets: inside | ring | outside, and `rcas` as a
// fourth where RCAS has a list of its own (null: it walks the inside segment).  Inside, outside and rcas in XCD order; the ring keeps the
// order it was found in.
void pack_lists(Plan &p, int eye, const TileClasses &c, const std::vector<uint32_t> &ring, const std::vector<uint32_t> *rcas)
{
    auto append = [&p](const std::vector<uint32_t> &v, bool xcdOrder, size_t &off, uint32_t &n) {
        off = p.lists.size();
        n = (uint32_t)v.size();
        for (uint32_t b = 0; b < n; ++b) p.lists.push_back(v[xcdOrder ? xcd_source(b, n) : b]);
    };
    append(c.inside, true, p.listOffInside[eye], p.nInside[eye]);
    append(ring, false, p.listOffRing[eye], p.nRing[eye]);
    append(c.outside, true, p.listOffOutside[eye], p.nOutside[eye]);
    p.listOffRcas[eye] = p.listOffInside[eye]; p.nRcas[eye] = p.nInside[eye];
    if (rcas) append(*rcas, true, p.listOffRcas[eye], p.nRcas[eye]);
    p.nSkipped[eye] = (uint32_t)c.hidden.size();
}

// Step 6.  One record per list entry for the persistent outside-tile kernel (outside_staged_kernel): tile origin, footprint origin (first
// column / row tap) and extent ([first tap, last tap + 1], what the kernel used to fetch through a chain of dependent scalar loads: tile
// index -> tap tables): tile_record (tile_records.h), which tile_records_kernel evaluates too.  Reads the plan's grid and lists and the
// tap tables of `tables` (the plan itself, or the one a re-aimed plan left them with); writes nothing.
std::vector<uint32_t> outside_records(const Plan &p, const Plan &tables)
{
    const TileRecordGrid g = record_grid(p);
    std::vector<uint32_t> recs(p.lists.size() * 4, 0u);
    const BilinTap *bx = tables.taps.data(), *by = tables.taps.data() + p.tapYOff;
    for (size_t i = 0; i < p.lists.size(); ++i) {
        const TileRecord r = tile_record(p.lists[i], g, bx, by);
        std::copy(r.w, r.w + 4, recs.begin() + 4 * i);
    }
    return recs;
}

// Is RCAS handed a list of its own (two-pass under a mesh), and are span records cut -- wherever the tiles are the span kernel's and its
// packing holds them?  Both follow from fields no gaze moves.
bool rcas_own_list(const PlanFields &p) { return p.hiddenArea && p.form == Form::TwoPass; }
bool cut_spans(const PlanFields &p)
{
    const TileGrid &g = p.grid;
    return g.tileW == (uint32_t)kTileW && g.tileH == (uint32_t)kRcasDppTileH && p.outputWidth < 65536u && g.ty < 65536u;
}

// The regions of a gaze-capable plan, from grid.tiles() and outW, for ANY mask centre.  Lists: inside, outside and hidden tiles are disjoint
// and the ring is a subset of outside + hidden, so inside | ring | outside hold at most 2 * tiles entries, RCAS's own list (every visible
// tile) at most tiles more; rounded up to 4 entries, so that every region's records start 16-byte aligned.  Spans: a run of k adjacent
// 32-wide tiles is cut into ceil(32 k / 62) <= k segments (cut_spans: outW < 65536, so the packing holds), the runs of an eye are disjoint:
// at most tiles segments.
void gaze_regions(PlanFields &p)
{
    const size_t tiles = p.grid.tiles();
    static_assert(kRcasDppTileW >= kTileW, "a run of k tiles is cut into at most k segments");
    p.listRegion = ((rcas_own_list(p) ? 3 : 2) * tiles + 3) & ~(size_t)3;
    p.spanRegion = cut_spans(p) ? tiles : 0;
}

// The steps, per eye, over p.grid; what steers them is the plan's own: maskLists, hiddenArea (with `hidden`, its per-eye maps) and form.
// Step 6 on the host only where `tables` (the plan holding the tap tables) is given.  A gaze-capable plan: every eye's lists and segments
// start at its region, the bound asserted.
void tile_lists(Plan &p, const HiddenMaps &hidden, const Plan *tables)
{
    const TileGrid &g = p.grid;
    const bool rcasOwnList = rcas_own_list(p), cutSpans = cut_spans(p);
    TileClasses c[2];
    std::vector<uint32_t> ring[2];
    for (int eye = 0; eye < 2; ++eye) {
        if (p.gazeCapable) { p.lists.resize((size_t)eye * p.listRegion, 0u); p.spans.resize(2 * (size_t)eye * p.spanRegion, 0u); }
        c[eye] = classify_tiles(g, p.outputWidth, p.outputHeight, p.centre[eye], p.radius[1], p.maskLists, hidden.eye[eye]);
        const std::vector<uint32_t> rcas = rcas_tiles(c[eye], rcasOwnList);
        ring[eye] = ring_tiles(g, rcas, ring_candidates(c[eye], rcasOwnList, p.hiddenArea && p.form == Form::MaskSorted));
        if (cutSpans) rcas_spans(g, p.outputWidth, rcas, p.spans, &p.spanOff[eye], &p.nSpans[eye]);
        pack_lists(p, eye, c[eye], ring[eye], rcasOwnList ? &rcas : nullptr);
        if (p.gazeCapable) {
            const bool fits = p.lists.size() <= (size_t)(eye + 1) * p.listRegion && p.spans.size() <= 2 * (size_t)(eye + 1) * p.spanRegion;
            assert(fits && "a gaze-capable plan's lists left their region");
            if (!fits) std::abort(); // (also where assert is compiled out: the device allocation is sized by the regions)
        }
    }
    if (p.gazeCapable) { p.lists.resize(2 * p.listRegion, 0u); p.spans.resize(4 * p.spanRegion, 0u); }
    // (the final lists: without a mesh outside and ring follow from inside)
    p.listsShared = c[0].inside == c[1].inside && c[0].outside == c[1].outside && ring[0] == ring[1];
    if (tables) p.recs = outside_records(p, *tables);
}

// Near-tie guard of a half-float intermediate: the smallest value whose flipped half rounding could exceed the 1e-3 tolerance
// behind RCAS.  RCAS's gain on its centre tap is at most 1 / (1 - 4 * 0.1875 * sharp) (lobe >= -FSR_RCAS_LIMIT * sharp,
// ffx_fsr1.h:654,757-765); a half in [b, 2b) moves in steps of b * 2^-10.  Binades whose step times that gain stays under
// 9e-4 are left alone; +inf (guard off) when no sharpening pass follows the upscale.
float tie_half_min(const ovrfsr_config &cfg, const Plan &p)
{
    if (!(p.doUpscale && p.doSharpen) || cfg.use_nis) return INFINITY;
    const float gain = 1.0f / (1.0f - 0.75f * con_float(p.rcasCon[0]));
    float b = 1.0f / 16384.0f; // half's smallest normal binade
    while (b < 65536.0f && gain * b * (1.0f / 1024.0f) < 9e-4f) b *= 2.0f;
    return b;
}

} // namespace

TileRecordGrid record_grid(const PlanFields &p)
{
    const TileGrid &g = p.grid;
    return TileRecordGrid{g.tx, g.tileW, g.tileH, p.outputWidth, p.outputHeight, p.outsideCols, p.outsideRows[g.tileH == (uint32_t)kTileH ? 0 : 1]};
}

const Refusal *plan_refusals(size_t *count)
{
    *count = R_COUNT;
    return kRefusals;
}

TileGrid tile_grid(bool useNis, bool doUpscale, uint32_t outW, uint32_t outH)
{
    TileGrid g;
    g.tileW = (uint32_t)kTileW;
    g.tileH = useNis && doUpscale ? 24u : (uint32_t)kTileH; // NVScaler's groups; NVSharpen dispatches 32x32 (PostProcessor.cpp:397,:492)
    g.groupW = useNis ? g.tileW : 16u;
    g.groupH = useNis ? g.tileH : 16u;
    g.tx = (outW + g.tileW - 1) / g.tileW;
    g.ty = (outH + g.tileH - 1) / g.tileH;
    return g;
}

const char *form_name(Form f)
{
    static const char *const names[] = {"none", "upscale only", "sharpen only", "two-pass", "mask-sorted", "fused", "fused with masked outside tiles"};
    return names[(int)f];
}

// UNORM8 store of a float source (easu_fast_kernel<RGBA16F / RGBA32F, RGBA8>: the kernel has no half store, so the field is its guard's
// SWITCH): +inf = off, the stores of every earlier release; finite = on, the store is the strict build's bit for bit.
float easu_tie_half_min(const Plan &plan, uint32_t inFormat, uint32_t outFormat, float halfGuard)
{
    // (inFormat: what the launch reads -- R11G11B10F words decoded in staging count as the RGBA16F texels they decode to)
    const uint32_t pf = pipeline_format(inFormat);
    const bool floatToUnorm8 = (pf == OVRFSR_FORMAT_RGBA16F || pf == OVRFSR_FORMAT_RGBA32F) && outFormat == OVRFSR_FORMAT_RGBA8_UNORM;
    return floatToUnorm8 ? plan.unorm8StoreGuard : halfGuard;
}

int plan_output_size(const ovrfsr_config &cfg, uint32_t inW, uint32_t inH, uint32_t *outW, uint32_t *outH)
{
    constexpr uint32_t kMaxExtent = 16384; // same limit CheckImage puts on caller images
    if (cfg.out_width != 0 && cfg.out_height != 0) {
        if (cfg.out_width > kMaxExtent || cfg.out_height > kMaxExtent) return OVRFSR_ERR_INVALID_ARGUMENT;
        *outW = cfg.out_width;
        *outH = cfg.out_height;
        return OVRFSR_OK;
    }
    // uint32 <- float truncation, PostProcessor.cpp:512-518.  A zero, negative or non-finite scale (a typo in
    // openvr_mod.cfg) has no defined uint conversion, and a tiny one asks for an unbounded image: both are rejected,
    // like any size beyond the 16384 texels an image may have here.
    const float s = cfg.render_scale;
    if (!std::isfinite(s) || !(s > 0.f)) return OVRFSR_ERR_INVALID_ARGUMENT;
    const float fw = s < 1.f ? inW / s : inW * s, fh = s < 1.f ? inH / s : inH * s;
    if (!(fw < (float)(kMaxExtent + 1)) || !(fh < (float)(kMaxExtent + 1))) return OVRFSR_ERR_INVALID_ARGUMENT;
    *outW = (uint32_t)fw;
    *outH = (uint32_t)fh;
    return OVRFSR_OK;
}

// the plan of one submission as it is filtered: what plan_pipeline has always been
// `maps`: non-null lays the plan out in per-eye regions (a gaze-capable or rescale-capable plan) and leaves the hidden-area maps there.
// `reuse`: the re-scale step (rescale_pipeline) -- the plan of another input size with the same output side: the mask constants and modes,
// the reciprocals, the layout and everything of the lists are taken from it instead of being computed, and no table but the taps is built.
static Refusal plan_filtered(const ovrfsr_config &cfg, uint32_t format, uint32_t width, uint32_t height, bool onlyOneEye, Plan *plan,
                             const HiddenArea *hidden, HiddenMaps *maps, bool rescaleCapable = false, const PlanFields *reuse = nullptr)
{
    Plan p;
    p.inputWidth = width; p.inputHeight = height; p.inputFormat = format;
    p.onlyOneEye = onlyOneEye;
    p.useNis = cfg.use_nis != 0;
    // what the kernels will see: a multisampled submission is resolved and a BGRA8 one re-ordered to RGBA8 first, R11G11B10F unpacked
    // (the RGBA16F route from here on): PostProcessor::ApplyPostProcess
    const uint32_t pf = p.pipelineFormat = pipeline_format(format);
    // The format of the textures the ctx creates for itself -- the quantised intermediate and the ctx-owned output:
    //   cfg.reference_formats = 0 (default): the pipeline input's own format.  This library's rule, not the reference's: half-float pipelines
    //     (BASELINE C5) keep a half intermediate and come back as RGBA16F.  It agrees with the reference for RGBA8, BGRA8 and RGB10A2.
    //   cfg.reference_formats = 1: the reference's DetermineOutputFormat (PostProcessor.cpp:63-74; upscaledTexture :348, sharpenedTexture :470).
    p.ownedFormat = cfg.reference_formats ? reference_output_format(pf) : pf;
    // quantize_intermediate=0 keeps fp32, whatever the format rule.
    const uint32_t mid = p.intermediateFormat = cfg.quantize_intermediate ? p.ownedFormat : (uint32_t)OVRFSR_FORMAT_RGBA32F;
    uint32_t ow = 0, oh = 0;
    if (plan_output_size(cfg, width, height, &ow, &oh) != OVRFSR_OK || ow == 0 || oh == 0) return kRefusals[R_OUTPUT_SIZE];
    p.outputWidth = ow; p.outputHeight = oh;

    const bool explicitSize = cfg.out_width != 0 && cfg.out_height != 0;
    const bool scaleNotOne = explicitSize ? (ow != width || oh != height) : (cfg.render_scale != 1.f);
    p.doUpscale = cfg.fsr_enabled && scaleNotOne;                       // :586
    p.doSharpen = cfg.fsr_enabled && (!cfg.use_nis || !scaleNotOne);    // :591
    if (cfg.stage_mask == 1) p.doSharpen = false;                       // "EASU-only" (BASELINE C1)
    if (cfg.stage_mask == 2) p.doUpscale = false;
    if (cfg.stage_mask < 0 || cfg.stage_mask > 2) return kRefusals[R_STAGE_MASK];
    if (!p.doUpscale && (ow != width || oh != height)) return kRefusals[R_SHARPEN_ONLY_SIZE];
    p.grid = tile_grid(p.useNis, p.doUpscale, ow, oh);
    if (cfg.precision != OVRFSR_PRECISION_FP32 && cfg.precision != OVRFSR_PRECISION_FP32_STRICT && cfg.precision != OVRFSR_PRECISION_FP32_EXACT)
        return kRefusals[R_PRECISION];
    const bool exact = cfg.precision == OVRFSR_PRECISION_FP32_EXACT, both = p.doUpscale && p.doSharpen;
    p.rcasPrec = cfg.precision;
    p.launchPrec = exact ? (int)PREC_FP32 : cfg.precision;
    if (exact) {
        if (cfg.use_nis) return kRefusals[R_EXACT_NIS];
        if (cfg.fused == 1) return kRefusals[R_EXACT_FUSED_ASKED];
        if (both && !cfg.quantize_intermediate) return kRefusals[R_EXACT_FLOAT_MID];
        if (p.doSharpen && (p.doUpscale ? mid : pf) != OVRFSR_FORMAT_RGBA8_UNORM) return kRefusals[R_EXACT_SOURCE];
    }

    for (int eye = 0; eye < 2 && !reuse; ++eye) {
        mask_constants(p.centre[eye], p.radius, ow, oh, cfg.proj_centre, cfg.radius, onlyOneEye ? 1 : 0, eye);
        const uint32_t gw = p.maskGroupW = cfg.use_nis ? 32u : 16u, gh = p.maskGroupH = cfg.use_nis ? (scaleNotOne ? 24u : 32u) : 16u;
        p.maskMode[eye] = classify_mask(p.centre[eye], p.radius[1], ow, oh, gw, gh);
    }
    if (reuse) {
        std::memcpy(p.centre, reuse->centre, sizeof p.centre); std::memcpy(p.radius, reuse->radius, sizeof p.radius);
        p.maskMode[0] = reuse->maskMode[0]; p.maskMode[1] = reuse->maskMode[1];
        p.maskGroupW = reuse->maskGroupW; p.maskGroupH = cfg.use_nis ? (scaleNotOne ? 24u : 32u) : 16u; // (a moved group height: a moved doUpscale)
    }
    if (cfg.use_nis) {
        // NVScalerUpdateConfig (scale != 1) or NVSharpenUpdateConfig (out == in), PostProcessor.cpp:308,:433
        if (!nis_scaler_config(&p.nis, cfg.sharpness, width, height, ow, oh)) return kRefusals[R_NIS_SCALE];
        p.nis.reserved1 = cfg.debug_mode ? 1.f : 0.f; // :309
        if (p.doUpscale) {
            nis_footprints(p);
            if (nis_pitch(p.nisCellsW) == 0 || nis_scaler_lds_bytes(p.nisCellsW, p.nisCellsH) > 64 * 1024) return kRefusals[R_NIS_LDS];
        }
    } else if (p.doUpscale) {
        easu_footprints(p);
        if (easu_lds_bytes(p.launchPrec, (int)pf, p.cellsW, p.cellsH) > 64 * 1024) return kRefusals[R_EASU_LDS];
    }
    if (reuse) { p.rcpOut[0] = reuse->rcpOut[0]; p.rcpOut[1] = reuse->rcpOut[1]; p.rcpExact = reuse->rcpExact; }
    else reciprocals(p);
    if (p.doUpscale) tap_tables(p);
    p.maskLists = p.doUpscale && p.launchPrec == PREC_FP32 && (p.maskMode[0] == MASK_MIXED || p.maskMode[1] == MASK_MIXED);
    // a hidden-area mesh (header, ovrfsr_set_hidden_area): product arithmetic and an upscale stage, like the lists it is built on.  The lists
    // then exist whatever the mask; the FORM below is chosen from the mask alone -- an unmasked two-pass stays two-pass, launched over lists
    p.hiddenArea = (reuse ? reuse->hiddenArea : hidden && (hidden->triangles[0] || hidden->triangles[1])) && p.doUpscale && p.launchPrec == PREC_FP32;
    p.tileLists = p.maskLists || p.hiddenArea;
    if (p.doSharpen && !cfg.use_nis) {
        float s = cfg.sharpness;
        s = s < 1.0f ? s : 1.0f; // AClampF1(x,0,1) = max(0,min(x,1)), PostProcessor.cpp:420
        s = s > 0.0f ? s : 0.0f;
        rcas_con(p.rcasCon, 2.f - 2 * s);
        p.rcasCon[3] = cfg.debug_mode ? 1u : 0u; // :430
    }
    p.tieHalfMin = tie_half_min(cfg, p);
    // on exactly under cfg.reference_formats -- the pipeline's UNORM8 intermediate and an EASU-only RGBA8 output alike
    p.unorm8StoreGuard = cfg.reference_formats ? 0.0f : INFINITY;

    // The form.  One launch with the intermediate in LDS only on request: on this chip both stages are VALU-bound and the ring
    // recompute costs more than the HBM round trip saves, so auto (-1) means two kernels.
    // auto: masked product-build pipelines run fused + mask-sorted (most of their pixels are plain bilinear copies, and tiles outside the
    // radius need no intermediate at all); unmasked ones stay two-pass (VALU-bound, the ring recompute costs 9 %)
    const bool tenBit = pf == OVRFSR_FORMAT_RGB10A2_UNORM; // two-kernel pipeline only (header)
    if (tenBit && cfg.fused == 1) return kRefusals[R_FUSED_TEN_BIT];
    // cfg.reference_formats with a float pipeline input (R11G11B10F counts as RGBA16F here): the intermediate is UNORM8, and no fused kernel is
    // built for a byte intermediate of a float source -- two-kernel forms only, the mask-sorted one where there is a mask
    const bool floatIn = pf == OVRFSR_FORMAT_RGBA16F || pf == OVRFSR_FORMAT_RGBA32F;
    if (cfg.reference_formats && floatIn && cfg.fused == 1) return kRefusals[R_FUSED_FLOAT_REFERENCE];
    const bool byteMidOfFloat = floatIn && mid == OVRFSR_FORMAT_RGBA8_UNORM;
    const bool fusedFits = fused_lds_bytes(p.launchPrec, (int)pf, (int)mid, p.fusedCellsW, p.fusedCellsH) <= kFusedLdsMax;
    const bool autoFused = !tenBit && !byteMidOfFloat && cfg.fused == -1 && p.maskLists && p.fusedCellsW <= 40 && fusedFits;
    // auto on a masked product-build EASU+RCAS pipeline: the two-pass kernels on the tiles touching the radius, tiles
    // outside written in final form (ApplySorted); cfg.fused = 1 keeps the single fused kernel on those tiles
    // Measured: with 4-byte pixels the sorted two-pass form wins (C2 shape, radius 0.5: +13 %); with 8/16-byte
    // pixels the outside kernel dominates the frame, and the three dependent launches of the sorted form lose to the
    // fused kernel (C5: -15 %), so those keep it.  The condition is the INTERMEDIATE's format: under cfg.reference_formats a float source
    // has a UNORM8 intermediate too, and takes this form (RCAS on rcas_dpp_kernel's span records; profiles/reference_formats.txt).
    const bool sorted = cfg.fused == -1 && p.maskLists && both && !cfg.use_nis && (pf == OVRFSR_FORMAT_RGBA8_UNORM || floatIn) &&
                        mid == OVRFSR_FORMAT_RGBA8_UNORM;
    bool fused = false;
    if ((cfg.fused == 1 || (autoFused && !sorted)) && both && !cfg.use_nis) {
        const bool pitchOk = p.launchPrec == PREC_FP32_STRICT || p.fusedCellsW <= 40;
        if (!pitchOk || !fusedFits) return kRefusals[R_FUSED_LDS];
        fused = true;
    }
    if (fused && exact) return kRefusals[R_EXACT_FUSED]; // (fused = -1 picks it for half / float intermediates only, refused above)
    p.form = sorted ? Form::MaskSorted : fused ? (p.maskLists ? Form::FusedMaskedOutside : Form::Fused)
           : both ? Form::TwoPass : p.doUpscale ? Form::UpscaleOnly : p.doSharpen ? Form::SharpenOnly : Form::None;

    // The tiles outside the radius of a masked pass are independent of the tiles touching it: their kernel can run on the ctx's auxiliary
    // stream beside the main kernel.  It does where it is the per-pixel, latency-bound kernel (half / float sources, minification); the
    // LDS-staged one of RGBA8 sources (outside_staged_ok) streams at HBM speed and is faster in order (measurements: PostProcessor::Fork).
    // cfg.reference_formats: the mask-sorted form of a float source (UNORM8 intermediate) runs in order on the caller's stream too, as the
    // RGBA8 one does -- its three launches are short, and the fork / join pair costs ~10 us per cross-queue wait
    BatchView v{};
    v.inW = (int32_t)width; v.inH = (int32_t)height; v.outW = (int32_t)ow; v.outH = (int32_t)oh;
    p.overlapOutside = p.maskLists && !(sorted && pf != OVRFSR_FORMAT_RGBA8_UNORM) && !outside_staged_ok(v, (int)pf);

    if (reuse) { // the layout and the lists stay where they are: rescale_pipeline compares everything else
        const PlanFields &r = *reuse;
        p.gazeCapable = r.gazeCapable; p.rescaleCapable = r.rescaleCapable;
        p.listRegion = r.listRegion; p.spanRegion = r.spanRegion;
        p.listsShared = r.listsShared;
        for (int eye = 0; eye < 2; ++eye) {
            p.nInside[eye] = r.nInside[eye]; p.nOutside[eye] = r.nOutside[eye]; p.nRing[eye] = r.nRing[eye]; p.nSpans[eye] = r.nSpans[eye];
            p.nRcas[eye] = r.nRcas[eye]; p.nSkipped[eye] = r.nSkipped[eye];
            p.listOffInside[eye] = r.listOffInside[eye]; p.listOffOutside[eye] = r.listOffOutside[eye]; p.listOffRing[eye] = r.listOffRing[eye];
            p.listOffRcas[eye] = r.listOffRcas[eye]; p.spanOff[eye] = r.spanOff[eye];
        }
        *plan = std::move(p);
        return Refusal{};
    }
    HiddenMaps rasterised;
    if (p.hiddenArea) rasterised = hidden_maps(p, *hidden);
    if (maps) {
        p.gazeCapable = true;
        p.rescaleCapable = rescaleCapable;
        gaze_regions(p);
    }
    if (p.tileLists) tile_lists(p, rasterised, &p);
    if (maps) *maps = std::move(rasterised);
    *plan = std::move(p);
    return Refusal{};
}

// what plan_pipeline makes of the RGBA32F twin's plan under OVRFSR_HDR_DOMAIN_SRTM
static void as_hdr_domain_plan(Plan &p, const ovrfsr_config &cfg, uint32_t format)
{
    const uint32_t pf = pipeline_format(format);
    p.hdrDomain = true;
    p.inputFormat = format;                                                    // what the plan is FOR (PostProcessor::PlannedFor)
    p.ownedFormat = cfg.reference_formats ? reference_output_format(pf) : pf;  // the submission's own rule
    p.rcasPrec = p.launchPrec;                                                 // RCAS stores fp32 here: nothing for exact stores to guard
}

Refusal plan_pipeline(const ovrfsr_config &cfg, uint32_t format, uint32_t width, uint32_t height, bool onlyOneEye, Plan *plan,
                      const HiddenArea *hidden, int hdrDomain, HiddenMaps *gaze, HiddenMaps *rescale)
{
    const uint32_t pf = pipeline_format(format);
    HiddenMaps *const maps = rescale ? rescale : gaze; // one layout for both; the caller hands the same maps where it asks for both
    if (hdrDomain == OVRFSR_HDR_DOMAIN_SRTM && (pf == OVRFSR_FORMAT_RGBA16F || pf == OVRFSR_FORMAT_RGBA32F)) {
        // FSR 1's reversible tone-mapped domain (header, "HDR domain"): the pipeline is the RGBA32F submission's, between a forward pass that
        // writes its input and a back pass that reads its result, both ctx-owned RGBA32F images.  No mesh: the back pass walks whole images.
        Plan p;
        if (!plan_filtered(cfg, OVRFSR_FORMAT_RGBA32F, width, height, onlyOneEye, &p, nullptr, maps, rescale != nullptr)) {
            as_hdr_domain_plan(p, cfg, format);
            *plan = std::move(p);
            return Refusal{};
        }
        // (refused as RGBA32F: whatever the submission itself gets -- the same refusal, or its own plan with the setting not applied)
    }
    return plan_filtered(cfg, format, width, height, onlyOneEye, plan, hidden, maps, rescale != nullptr);
}

Rescale rescale_pipeline(const Plan &current, const ovrfsr_config &effective, uint32_t width, uint32_t height, const HiddenMaps &hidden,
                         int hdrDomain, Plan *rescaled)
{
    (void)hidden; // (the lists stay as they are: nothing here classifies a tile)
    const PlanFields &c = current;
    if (width == c.inputWidth && height == c.inputHeight) return Rescale::Nothing;
    if (!c.rescaleCapable) return Rescale::Rebuild;
    // the RGBA32F twin of OVRFSR_HDR_DOMAIN_SRTM: in place only where `current` is that twin's plan and the new size's is too
    const uint32_t pf = pipeline_format(c.inputFormat);
    const bool wantsTwin = hdrDomain == OVRFSR_HDR_DOMAIN_SRTM && (pf == OVRFSR_FORMAT_RGBA16F || pf == OVRFSR_FORMAT_RGBA32F);
    if (wantsTwin != c.hdrDomain) return Rescale::Rebuild;
    Plan p;
    if (plan_filtered(effective, c.hdrDomain ? (uint32_t)OVRFSR_FORMAT_RGBA32F : c.inputFormat, width, height, c.onlyOneEye, &p, nullptr, nullptr, true, &c))
        return Rescale::Rebuild; // (a refusal: the rebuild fails as a fresh ctx does)
    if (c.hdrDomain) as_hdr_domain_plan(p, effective, c.inputFormat);
    // everything plan_filtered computed that a re-scale must not move (the mask, the reciprocals, the layout and the lists were taken over)
    const bool same = p.inputFormat == c.inputFormat && p.onlyOneEye == c.onlyOneEye && p.outputWidth == c.outputWidth && p.outputHeight == c.outputHeight &&
                      p.doUpscale == c.doUpscale && p.doSharpen == c.doSharpen && p.useNis == c.useNis && p.form == c.form && p.tileLists == c.tileLists &&
                      p.maskLists == c.maskLists && p.hiddenArea == c.hiddenArea && p.overlapOutside == c.overlapOutside && p.hdrDomain == c.hdrDomain &&
                      p.pipelineFormat == c.pipelineFormat && p.intermediateFormat == c.intermediateFormat && p.ownedFormat == c.ownedFormat &&
                      p.launchPrec == c.launchPrec && p.rcasPrec == c.rcasPrec && !std::memcmp(p.rcasCon, c.rcasCon, sizeof p.rcasCon) &&
                      !std::memcmp(&p.tieHalfMin, &c.tieHalfMin, sizeof(float)) && !std::memcmp(&p.unorm8StoreGuard, &c.unorm8StoreGuard, sizeof(float)) &&
                      p.tapYOff == c.tapYOff && p.maskGroupH == c.maskGroupH && p.grid.tileW == c.grid.tileW && p.grid.tileH == c.grid.tileH &&
                      p.grid.groupW == c.grid.groupW && p.grid.groupH == c.grid.groupH && p.grid.tx == c.grid.tx && p.grid.ty == c.grid.ty;
    if (!same) return Rescale::Rebuild;
    if (p.tileLists && !current.lists.empty()) {
        p.lists = current.lists; p.spans = current.spans;
        p.recs = outside_records(p, p);
    }
    *rescaled = std::move(p);
    return Rescale::InPlace;
}

Reaim reaim_pipeline(const Plan &current, const ovrfsr_config &effective, const HiddenMaps &hidden, Plan *reaimed, bool hostRecords)
{
    const PlanFields &c = current;
    uint32_t centre[2][4], radius[4], mode[2];
    for (int eye = 0; eye < 2; ++eye) {
        mask_constants(centre[eye], radius, c.outputWidth, c.outputHeight, effective.proj_centre, effective.radius, c.onlyOneEye ? 1 : 0, eye);
        mode[eye] = classify_mask(centre[eye], radius[1], c.outputWidth, c.outputHeight, c.maskGroupW, c.maskGroupH);
    }
    if (!std::memcmp(centre, c.centre, sizeof centre)) return Reaim::Nothing; // (the same centres: the same modes and lists)
    // what plan_pipeline derives from the modes: maskLists -- and from it tileLists, the form and overlapOutside --, and resolve_in_staging's
    // "every group of both eyes is inside the radius"
    const bool maskLists = c.doUpscale && c.launchPrec == PREC_FP32 && (mode[0] == MASK_MIXED || mode[1] == MASK_MIXED);
    const bool allInside = mode[0] == MASK_ALL_INSIDE && mode[1] == MASK_ALL_INSIDE;
    const bool wasAllInside = c.maskMode[0] == MASK_ALL_INSIDE && c.maskMode[1] == MASK_ALL_INSIDE;
    if (!c.gazeCapable || maskLists != c.maskLists || allInside != wasAllInside) return Reaim::Rebuild;
    Plan p;
    static_cast<PlanFields &>(p) = c;
    std::memcpy(p.centre, centre, sizeof centre);
    p.maskMode[0] = mode[0]; p.maskMode[1] = mode[1];
    if (p.tileLists) tile_lists(p, hidden, hostRecords ? &current : nullptr);
    *reaimed = std::move(p);
    return Reaim::InPlace;
}

Refusal destination_refusal(const Plan &plan, uint32_t destFormat)
{
    // exact stores: the sharpen stage's destination must be RGBA8 too (a BGRA8 destination is refused below in every mode)
    if (plan.rcasPrec == OVRFSR_PRECISION_FP32_EXACT && plan.doSharpen && destFormat != OVRFSR_FORMAT_RGBA8_UNORM && destFormat != OVRFSR_FORMAT_BGRA8_UNORM)
        return kRefusals[R_DEST_EXACT];
    if (input_only(destFormat)) return kRefusals[R_DEST_INPUT_ONLY]; // (BGRA8: see the table)
    // R10G10B10A2 exists for the reference's 10-bit path: 10-bit in -> 10-bit out (or float, to measure parity)
    const bool inTen = plan.pipelineFormat == OVRFSR_FORMAT_RGB10A2_UNORM, outTen = destFormat == OVRFSR_FORMAT_RGB10A2_UNORM;
    if ((outTen && !inTen) || (inTen && !outTen && destFormat != OVRFSR_FORMAT_RGBA32F)) return kRefusals[R_DEST_TEN_BIT_PAIR];
    // (a float intermediate in front of a 10-bit destination is a kernel pair nobody builds: refused before anything is launched,
    // instead of surfacing as a launch error behind the EASU pass -- found by the round-6 format sweep)
    if (outTen && plan.doUpscale && plan.doSharpen && plan.intermediateFormat != OVRFSR_FORMAT_RGB10A2_UNORM) return kRefusals[R_DEST_TEN_BIT_MID];
    return Refusal{};
}

// 4-sample RGBA8 on C2's path -- product build, unmasked easu_fast_kernel, two-kernel pipeline with a UNORM8 intermediate or EASU-only into
// UNORM8 -- is resolved inside EASU's staging sweep (FMT_RGBA8_MS4, the same resolve_unorm8 the resolve pass runs: identical staged bytes,
// identical output); every other multisampled input takes the resolve pass.  -DOVRFSR_MSAA_RESOLVE_PASS (measurement build, never shipped)
// sends this path through the resolve pass too: the A/B of profiles/msaa_c2.txt.
//
// A single-sample R11G11B10F submission is decoded where the product build's fixed-pitch kernels stage or load their texels (easu_fast_kernel,
// fused_kernel, easu_outside_kernel: the fp32 values the pass's RGBA16F copy would have delivered, so identical output) in every form with an
// upscale stage; the pass and its copy remain for multisampled R11G11B10F, the strict build, NIS, sharpen-only, footprints wider than
// 40 cells (the generic-pitch easu_kernel has no instance) and the masked launches named below.  -DOVRFSR_PACKED_RESOLVE_PASS (measurement build, never shipped) keeps the pass
// everywhere: the A/B of profiles/r11g11b10f_in_place.txt.
//
// One family of masked launches keeps the pass although its kernels exist.  The bilinear fallback of the tiles outside the radius
// (bilinear_column4) blends with contraction allowed wherever no UNORM8 rounding follows; where that blend is rounded to half -- a half
// destination or a half intermediate -- the compiler fuses the last FMA with the rounding for some pixels of a thread and not for others, and
// it does not choose the same pixels for texels decoded from words as for texels loaded as halves: one rounding against two, a last-bit
// difference in about one value of 10^4.  Only the pair the default masked half pipeline launches (half intermediate AND half destination)
// was found equal at full size (C5, 16 images); the other pairs with a half rounding and no UNORM8 one stay behind the pass until their
// bytes are shown equal too: (half, none), (half, float), (float, half) as (destination, intermediate) of the outside-tile launch.
static bool packed_in_staging(const Plan &plan, uint32_t destFormat)
{
#ifdef OVRFSR_PACKED_RESOLVE_PASS
    (void)plan; (void)destFormat;
    return false;
#else
    if (plan.inputFormat != (uint32_t)FMT_R11G11B10F || plan.useNis || plan.launchPrec != PREC_FP32 || !plan.doUpscale) return false;
    bool fixedPitch = false, easuAlone = false;
    switch (plan.form) {
    case Form::UpscaleOnly: case Form::TwoPass: fixedPitch = easu_kernel_pitch(plan.cellsW) != 0; easuAlone = true; break;
    case Form::MaskSorted: fixedPitch = easu_kernel_pitch(plan.cellsW) != 0; break;
    case Form::Fused: case Form::FusedMaskedOutside: fixedPitch = easu_fast_pitch(plan.fusedCellsW) != 0; break;
    default: break;
    }
    if (!fixedPitch) return false;
    // (maskLists, not tileLists: a hidden-area mesh must not move the decision -- the pixels it leaves are the bytes of the call without it)
    const bool masked = plan.maskLists || plan.maskMode[0] != MASK_ALL_INSIDE || plan.maskMode[1] != MASK_ALL_INSIDE;
    if (masked) {
        // what the bilinear fallback of this form stores into, and the intermediate rounding it applies on the way (none: -1)
        const uint32_t none = ~0u, half = OVRFSR_FORMAT_RGBA16F, byte = OVRFSR_FORMAT_RGBA8_UNORM;
        const uint32_t o = easuAlone && plan.doSharpen ? plan.intermediateFormat : destFormat, m = easuAlone ? none : plan.intermediateFormat;
        const bool exactBlend = o == byte || m == byte, halfRounding = o == half || m == half;
        if (!exactBlend && halfRounding && !(o == half && m == half)) return false;
    }
    return true;
#endif
}

bool resolve_in_staging(const Plan &plan, uint32_t destFormat)
{
    if (plan.hdrDomain) return false; // the kernels read the forward pass's RGBA32F copy: the front pass, where one exists, feeds that pass
    if (packed_in_staging(plan, destFormat)) return true;
#ifdef OVRFSR_MSAA_RESOLVE_PASS
    (void)plan; (void)destFormat;
    return false;
#else
    const bool unmasked = !plan.tileLists && plan.maskMode[0] == MASK_ALL_INSIDE && plan.maskMode[1] == MASK_ALL_INSIDE;
    const bool plain = plan.form == Form::UpscaleOnly || plan.form == Form::TwoPass;
    const uint32_t easuOut = plan.doSharpen ? plan.intermediateFormat : destFormat;
    return plan.inputFormat == (uint32_t)FMT_RGBA8_MS4 && plain && !plan.useNis && unmasked &&
           easu_msaa_fused_ok(plan.launchPrec, (int)easuOut, plan.cellsW);
#endif
}

} // namespace ovrfsr
