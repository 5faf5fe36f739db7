// tests/debug/plan_probe.cpp -- the pipeline planner (csrc/pipeline_plan.cpp) on its own: no HIP, no device.  tests/test_pipeline_plan.py
// compiles this file with pipeline_plan.cpp, constants.cpp and nis_config.cpp under -fsanitize=address,undefined and runs it as a child.
//
//   plan_probe --refusals        one line per refusal the planner can produce: <status>\t<text>
//   plan_probe CASES             one JSON line per line of the file CASES:
//       the 25 fields tests/debug/plan_serial.h names (plan_serial::Case)
//   Each line reports the refusal or the plan (form, formats, stage selection, list sizes, the EASU and fused-kernel LDS footprints "cells" /
//   "fused_cells" and the bilinear footprint bound "outside_cols" / "outside_rows" of the outside-tile kernel), the destination refusal and resolve_in_staging
//   for the destination, "unorm8_guard" (is the guard of an EASU launch from the pipeline format into RGBA8 switched on: easu_tie_half_min),
//   "invariants": "ok" or the first structural invariant of the plan's tables that does not hold, and "digest": the FNV-1a digest of the
//   whole plan serialised by value (plan_serial.h).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../openvr_fsr_amd/csrc/pipeline_plan.h"
#include "plan_serial.h"

using namespace ovrfsr;

static std::string fail(const char *fmt, long a = 0, long b = 0, long c = 0)
{
    char buf[256];
    std::snprintf(buf, sizeof buf, fmt, a, b, c);
    return buf;
}

// the structural invariants of the tables a Plan holds; "ok" or the first that does not hold
static std::string invariants(const Plan &p)
{
    const uint32_t outW = p.outputWidth, outH = p.outputHeight;
    if (p.doUpscale) {
        // the tap table is long enough for the padded column reads: every 32-wide tile reads 32 column taps from its origin, the row taps follow
        const uint32_t padded = (outW + 31u) / 32u * 32u;
        if (p.tapYOff < padded) return fail("row taps at %ld, inside the padded column taps (%ld)", p.tapYOff, padded);
        if (p.taps.size() < (size_t)p.tapYOff + outH) return fail("tap table holds %ld entries, needs %ld", (long)p.taps.size(), (long)p.tapYOff + outH);
        for (uint32_t o = 0; o < padded; ++o)
            if (p.taps[o].i0 < -1 || p.taps[o].i0 >= (int)p.inputWidth) return fail("column tap %ld = %ld out of range", o, p.taps[o].i0);
        for (uint32_t o = 0; o < outH; ++o)
            if (p.taps[p.tapYOff + o].i0 < -1 || p.taps[p.tapYOff + o].i0 >= (int)p.inputHeight) return fail("row tap %ld = %ld out of range", o, p.taps[p.tapYOff + o].i0);
    }
    if (!p.tileLists) {
        if (!p.lists.empty() || !p.recs.empty() || !p.spans.empty()) return "tables without tile lists";
        return "ok";
    }
    // the tile size is the plan's; the counts are recomputed from the output size here, so that a wrong grid cannot vouch for itself
    const uint32_t tileW = p.grid.tileW, tileH = p.grid.tileH;
    const uint32_t tx = (outW + tileW - 1) / tileW, ty = (outH + tileH - 1) / tileH, nt = tx * ty;
    if (p.grid.tx != tx || p.grid.ty != ty) return fail("the grid counts %ld x %ld tiles, the output size gives %ld columns", p.grid.tx, p.grid.ty, tx);
    if (p.recs.size() != 4 * p.lists.size()) return "one record per list entry";
    std::vector<uint8_t> seen(nt);
    for (int eye = 0; eye < 2; ++eye) {
        // inside + outside: a permutation of all tiles; ring: a subset of outside, 4-adjacent to an inside tile
        if ((size_t)p.nInside[eye] + p.nOutside[eye] != nt) return fail("eye %ld: inside + outside = %ld of %ld tiles", eye, (long)p.nInside[eye] + p.nOutside[eye], nt);
        if (p.listOffInside[eye] + p.nInside[eye] > p.lists.size() || p.listOffRing[eye] + p.nRing[eye] > p.lists.size() ||
            p.listOffOutside[eye] + p.nOutside[eye] > p.lists.size())
            return fail("eye %ld: a list runs past the table", eye);
        if (p.listOffRing[eye] != p.listOffInside[eye] + p.nInside[eye]) return fail("eye %ld: the ring does not follow the inside list", eye);
        std::fill(seen.begin(), seen.end(), 0);
        for (uint32_t i = 0; i < p.nInside[eye]; ++i) {
            const uint32_t t = p.lists[p.listOffInside[eye] + i];
            if (t >= nt || seen[t]) return fail("eye %ld: inside entry %ld = tile %ld out of range or repeated", eye, i, t);
            seen[t] = 1;
        }
        for (uint32_t i = 0; i < p.nOutside[eye]; ++i) {
            const uint32_t t = p.lists[p.listOffOutside[eye] + i];
            if (t >= nt || seen[t]) return fail("eye %ld: outside entry %ld = tile %ld out of range or repeated", eye, i, t);
            seen[t] = 2;
        }
        for (uint32_t i = 0; i < p.nRing[eye]; ++i) {
            const uint32_t t = p.lists[p.listOffRing[eye] + i];
            if (t >= nt || seen[t] != 2) return fail("eye %ld: ring entry %ld = tile %ld is not an outside tile", eye, i, t);
            const uint32_t y = t / tx, x = t % tx;
            const bool adj = (x > 0 && seen[t - 1] == 1) || (x + 1 < tx && seen[t + 1] == 1) || (y > 0 && seen[t - tx] == 1) || (y + 1 < ty && seen[t + tx] == 1);
            if (!adj) return fail("eye %ld: ring tile %ld touches no inside tile", eye, t);
            seen[t] = 3;
        }
        // spans: inside [0, outW], at most 62 columns, tile row below ty -- and on inside tiles only
        if (2 * (p.spanOff[eye] + p.nSpans[eye]) > p.spans.size()) return fail("eye %ld: spans run past the table", eye);
        for (uint32_t i = 0; i < p.nSpans[eye]; ++i) {
            const uint32_t a = p.spans[2 * (p.spanOff[eye] + i)], xEnd = p.spans[2 * (p.spanOff[eye] + i) + 1];
            const uint32_t x0 = a & 0xffffu, row = a >> 16;
            if (!(x0 < xEnd && xEnd <= outW && xEnd - x0 <= 62u && row < ty)) return fail("eye %ld: span %ld malformed (x0 %ld)", eye, i, x0);
            if (seen[row * tx + x0 / tileW] != 1 || seen[row * tx + (xEnd - 1) / tileW] != 1) return fail("eye %ld: span %ld leaves the inside tiles", eye, i);
        }
    }
    // records: tile origin, footprint origin taps in range, extent within the planes the kernels allocate
    const uint32_t rowsCap = p.outsideRows[p.useNis ? 1 : 0];
    for (size_t i = 0; i < p.lists.size(); ++i) {
        const uint32_t t = p.lists[i], ox0 = (t % tx) * tileW, oy0 = (t / tx) * tileH;
        const uint32_t r0 = p.recs[4 * i], r1 = p.recs[4 * i + 1], r2 = p.recs[4 * i + 2];
        if (r0 != (ox0 | oy0 << 16)) return fail("record %ld: origin", (long)i);
        const int X0 = (int)(r1 & 0xffffu) - 1, Y0 = (int)(r1 >> 16) - 1;
        if (X0 < -1 || X0 >= (int)p.inputWidth || Y0 < -1 || Y0 >= (int)p.inputHeight) return fail("record %ld: origin taps %ld, %ld out of range", (long)i, X0, Y0);
        const uint32_t colsN = r2 & 0xffu, rowsN = r2 >> 8;
        if (colsN < 2 || colsN > p.outsideCols || rowsN < 2 || rowsN > rowsCap) return fail("record %ld: extent %ld x %ld", (long)i, colsN, rowsN);
    }
    return "ok";
}

static std::string quoted(const char *s)
{
    std::string q = "\"";
    for (; *s; ++s) {
        if (*s == '"' || *s == '\\') q += '\\';
        q += *s;
    }
    return q + "\"";
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: plan_probe --refusals | plan_probe CASES\n");
        return 2;
    }
    if (!std::strcmp(argv[1], "--refusals")) {
        size_t n = 0;
        const Refusal *r = plan_refusals(&n);
        for (size_t i = 0; i < n; ++i) std::printf("%d\t%s\n", r[i].status, r[i].text);
        return 0;
    }
    std::ifstream f(argv[1]);
    if (!f) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        plan_serial::Case k;
        if (!plan_serial::parse_case(in, k)) {
            std::fprintf(stderr, "malformed case line: %s\n", line.c_str());
            return 2;
        }
        const ovrfsr_config &c = k.cfg;
        Plan p;
        const Refusal r = plan_pipeline(c, k.format, k.width, k.height, k.oneEye != 0, &p);
        std::printf("{\"id\": %s, \"status\": %d, \"text\": %s", quoted(k.id.c_str()).c_str(), r.status, quoted(r.text).c_str());
        if (!r) {
            const uint32_t d = k.dest < 0 ? p.ownedFormat : (uint32_t)k.dest;
            const Refusal dr = destination_refusal(p, d);
            std::printf(", \"form\": %s, \"out\": [%u, %u], \"upscale\": %d, \"sharpen\": %d, \"pipeline\": %u, \"mid\": %u, \"owned\": %u, \"tile_lists\": %d, "
                        "\"overlap\": %d, \"lists_shared\": %d, \"dest_status\": %d, \"dest_text\": %s, \"dest_disables\": %d, \"resolve_in_staging\": %d, "
                        "\"inside\": [%u, %u], \"ring\": [%u, %u], \"outside\": [%u, %u], \"spans\": [%u, %u], \"unorm8_guard\": %d, \"cells\": [%d, %d], \"fused_cells\": [%d, %d], "
                        "\"outside_cols\": %u, \"outside_rows\": [%u, %u], \"invariants\": %s, \"digest\": \"%s\"",
                        quoted(form_name(p.form)).c_str(), p.outputWidth, p.outputHeight, (int)p.doUpscale, (int)p.doSharpen, p.pipelineFormat,
                        p.intermediateFormat, p.ownedFormat, (int)p.tileLists, (int)p.overlapOutside, (int)p.listsShared, dr.status, quoted(dr.text).c_str(),
                        (int)dr.disables, (int)resolve_in_staging(p, d), p.nInside[0], p.nInside[1], p.nRing[0], p.nRing[1], p.nOutside[0], p.nOutside[1],
                        p.nSpans[0], p.nSpans[1], (int)std::isfinite(easu_tie_half_min(p, p.pipelineFormat, OVRFSR_FORMAT_RGBA8_UNORM, INFINITY)),
                        p.cellsW, p.cellsH, p.fusedCellsW, p.fusedCellsH, p.outsideCols, p.outsideRows[0], p.outsideRows[1],
                        quoted(invariants(p).c_str()).c_str(), plan_serial::digest(p).c_str());
        }
        std::printf("}\n");
    }
    return 0;
}
