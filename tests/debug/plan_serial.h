// tests/debug/plan_serial.h -- what tests/debug/plan_probe.cpp and tests/debug/hidden_probe.cpp share: the case-line parser, and a Plan
// serialised BY VALUE with a 64-bit FNV-1a digest of it (tests/golden/plan_digests_parent.json holds the digests of the commit before the
// planner's tile lists were split into steps; tests/test_pipeline_plan.py and tests/test_hidden_area.py compare every line they plan).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <istream>
#include <string>
#include <vector>
#include "../../openvr_fsr_amd/csrc/pipeline_plan.h"

namespace plan_serial {

// id format width height onlyOneEye destFormat(-1: ctx-owned) fsr_enabled use_nis debug_mode render_scale sharpness radius proj_centre[4]
// out_width out_height precision quantize_intermediate fused stage_mask pair_submit reference_formats
struct Case {
    std::string id;
    uint32_t format = 0, width = 0, height = 0;
    int oneEye = 0;
    long dest = -1;
    ovrfsr_config cfg;
};

// reads the 25 fields from `in` and leaves it behind them (hidden_probe reads its meshes from there); false: malformed
inline bool parse_case(std::istream &in, Case &k)
{
    ovrfsr_config &c = k.cfg;
    std::memset(&c, 0, sizeof c);
    c.struct_size = sizeof c;
    in >> k.id >> k.format >> k.width >> k.height >> k.oneEye >> k.dest >> c.fsr_enabled >> c.use_nis >> c.debug_mode >> c.render_scale >>
        c.sharpness >> c.radius >> c.proj_centre[0] >> c.proj_centre[1] >> c.proj_centre[2] >> c.proj_centre[3] >> c.out_width >>
        c.out_height >> c.precision >> c.quantize_intermediate >> c.fused >> c.stage_mask >> c.pair_submit >> c.reference_formats;
    return (bool)in;
}

// Values are appended in a fixed width, whatever type the Plan keeps them in: u32 (counts, formats, enums, bools as 0 / 1), i32, u64
// (offsets), the 4 bytes of a float -- so the bytes follow from the VALUES in the order below and from nothing else of the Plan's layout.
struct Writer {
    std::string s;
    void raw(const void *p, size_t n) { s.append(static_cast<const char *>(p), n); }
    void u32(uint32_t v) { raw(&v, 4); }
    void i32(int32_t v) { raw(&v, 4); }
    void u64(uint64_t v) { raw(&v, 8); }
    void f32(float v) { raw(&v, 4); }
    void u32s(const uint32_t *v, size_t n) { for (size_t i = 0; i < n; ++i) u32(v[i]); }
    void table(const std::vector<uint32_t> &v) { u64(v.size()); u32s(v.data(), v.size()); }
};

// The field order (a change here changes every digest):
//   1  inputWidth inputHeight inputFormat onlyOneEye outputWidth outputHeight
//   2  doUpscale doSharpen useNis form tileLists maskLists hiddenArea overlapOutside
//   3  pipelineFormat intermediateFormat ownedFormat launchPrec rcasPrec
//   4  easuCon[16] rcasCon[4] nis (the 256-byte NISConfig block as the device reads it)
//   5  centre[2][4] radius[4] maskMode[2] tieHalfMin unorm8StoreGuard
//   6  cellsW cellsH fusedCellsW fusedCellsH nisCellsW nisCellsH rcpOut[2] rcpExact
//   7  taps: count, then (i0, frac) each; tapYOff outsideCols outsideRows[2]
//   8  grid: tileW tileH groupW groupH tx ty
//   9  the tiles per image the lists were built over: tx * ty with tile lists, 0 without
//  10  listsShared
//  11  per eye: inside ring outside rcas spans, each (offset u64, count u32); nSkipped
//  12  lists recs spans: count (u64), then the dwords
inline std::string serialise(const ovrfsr::Plan &p)
{
    Writer w;
    w.u32(p.inputWidth); w.u32(p.inputHeight); w.u32(p.inputFormat); w.u32(p.onlyOneEye); w.u32(p.outputWidth); w.u32(p.outputHeight);
    w.u32(p.doUpscale); w.u32(p.doSharpen); w.u32(p.useNis); w.u32((uint32_t)p.form); w.u32(p.tileLists); w.u32(p.maskLists); w.u32(p.hiddenArea);
    w.u32(p.overlapOutside);
    w.u32(p.pipelineFormat); w.u32(p.intermediateFormat); w.u32(p.ownedFormat); w.i32(p.launchPrec); w.i32(p.rcasPrec);
    w.u32s(p.easuCon, 16); w.u32s(p.rcasCon, 4); w.raw(&p.nis, sizeof p.nis);
    w.u32s(&p.centre[0][0], 8); w.u32s(p.radius, 4); w.u32s(p.maskMode, 2); w.f32(p.tieHalfMin); w.f32(p.unorm8StoreGuard);
    w.i32(p.cellsW); w.i32(p.cellsH); w.i32(p.fusedCellsW); w.i32(p.fusedCellsH); w.i32(p.nisCellsW); w.i32(p.nisCellsH);
    w.f32(p.rcpOut[0]); w.f32(p.rcpOut[1]); w.u32(p.rcpExact);
    w.u64(p.taps.size());
    for (const ovrfsr::BilinTap &t : p.taps) { w.i32(t.i0); w.f32(t.frac); }
    w.u32(p.tapYOff); w.u32(p.outsideCols); w.u32s(p.outsideRows, 2);
    const ovrfsr::TileGrid &g = p.grid;
    w.u32(g.tileW); w.u32(g.tileH); w.u32(g.groupW); w.u32(g.groupH); w.u32(g.tx); w.u32(g.ty);
    w.u32(p.tileLists ? g.tx * g.ty : 0u);
    w.u32(p.listsShared);
    for (int e = 0; e < 2; ++e) {
        w.u64(p.listOffInside[e]); w.u32(p.nInside[e]); w.u64(p.listOffRing[e]); w.u32(p.nRing[e]); w.u64(p.listOffOutside[e]); w.u32(p.nOutside[e]);
        w.u64(p.listOffRcas[e]); w.u32(p.nRcas[e]); w.u64(p.spanOff[e]); w.u32(p.nSpans[e]);
        w.u32(p.nSkipped[e]);
    }
    w.table(p.lists); w.table(p.recs); w.table(p.spans);
    return w.s;
}

inline uint64_t fnv1a64(const std::string &s)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (unsigned char c : s) h = (h ^ c) * 0x100000001b3ull;
    return h;
}

// "digest" of the probes' JSON lines: 16 hex digits
inline std::string digest(const ovrfsr::Plan &p)
{
    char buf[17];
    std::snprintf(buf, sizeof buf, "%016llx", (unsigned long long)fnv1a64(serialise(p)));
    return buf;
}

} // namespace plan_serial
