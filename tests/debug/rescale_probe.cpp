// tests/debug/rescale_probe.cpp -- the planner's re-scale step (csrc/pipeline_plan.cpp, rescale_pipeline) on its own: no HIP, no device.
// tests/test_dynamic_resolution.py compiles this file with pipeline_plan.cpp, constants.cpp and nis_config.cpp under
// -fsanitize=address,undefined and runs it as a child.
//
//   rescale_probe walk CASES    per line: the 25 fields of plan_serial::Case (width, height: the size the ctx is built for), hdrDomain, n, then
//                               n x (width height): the sizes submitted afterwards.  A rescale-capable plan walks them the way the launch
//                               manager does: InPlace -> the rescaled plan becomes the current one; Rebuild -> plan_pipeline at that size (a
//                               refusal ends the walk).  One JSON line: "first" (status of the first plan), "steps": per size the answer, the
//                               fresh plan's status / text / form and flags, and for InPlace "equal": does the rescaled plan equal the fresh
//                               rescale-capable plan of that size by value (plan_serial: every field and table) and in its layout; "final_equal":
//                               the plan after the walk against the fresh plan of the last size; "plain_digest": the digest of the plan of the
//                               first size made WITHOUT a maximum (what tests/golden/plan_digests_parent.json records)
//   rescale_probe taps CASES    per line: inW inH outW outH -> the FNV-1a digest of the tap table [outW column taps | padding | outH row taps |
//                               64 spare] built from bilin_taps.h's host side alone
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "../../openvr_fsr_amd/csrc/bilin_taps.h"
#include "../../openvr_fsr_amd/csrc/pipeline_plan.h"
#include "plan_serial.h"

using namespace ovrfsr;

static std::string quoted(const char *s)
{
    std::string q = "\"";
    for (; *s; ++s) {
        if (*s == '"' || *s == '\\') q += '\\';
        q += *s;
    }
    return q + "\"";
}

static bool same_layout(const PlanFields &a, const PlanFields &b)
{
    return a.gazeCapable == b.gazeCapable && a.rescaleCapable == b.rescaleCapable && a.listRegion == b.listRegion && a.spanRegion == b.spanRegion &&
           a.maskGroupW == b.maskGroupW && a.maskGroupH == b.maskGroupH && a.hdrDomain == b.hdrDomain;
}

static int walk(std::istream &f)
{
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        plan_serial::Case k;
        int hdr = 0, n = 0;
        if (!plan_serial::parse_case(in, k) || !(in >> hdr >> n)) {
            std::fprintf(stderr, "malformed case line: %s\n", line.c_str());
            return 2;
        }
        Plan plain, cur;
        HiddenMaps maps;
        const Refusal pr = plan_pipeline(k.cfg, k.format, k.width, k.height, k.oneEye != 0, &plain, nullptr, hdr);
        const Refusal first = plan_pipeline(k.cfg, k.format, k.width, k.height, k.oneEye != 0, &cur, nullptr, hdr, nullptr, &maps);
        std::printf("{\"id\": %s, \"first\": %d, \"plain_digest\": \"%s\", \"capable_equals_plain\": %d, \"form\": %s, \"steps\": [", quoted(k.id.c_str()).c_str(),
                    first.status, pr ? "" : plan_serial::digest(plain).c_str(),
                    // the same plan in every field the kernels read: everything but the list and span offsets, which the layout moves
                    (int)(!pr && !first && plain.form == cur.form && plain.tileLists == cur.tileLists && plain.taps.size() == cur.taps.size() &&
                          !std::memcmp(plain.easuCon, cur.easuCon, sizeof plain.easuCon) && plain.nInside[0] == cur.nInside[0] && plain.nOutside[1] == cur.nOutside[1]),
                    first ? "\"\"" : quoted(form_name(cur.form)).c_str());
        bool alive = !first, finalEqual = false;
        for (int i = 0; i < n; ++i) {
            uint32_t w = 0, h = 0;
            if (!(in >> w >> h)) {
                std::fprintf(stderr, "malformed size list: %s\n", line.c_str());
                return 2;
            }
            if (!alive) continue;
            Plan next, fresh;
            HiddenMaps m2;
            const Rescale r = rescale_pipeline(cur, k.cfg, w, h, maps, hdr, &next);
            const Refusal fr = plan_pipeline(k.cfg, k.format, w, h, k.oneEye != 0, &fresh, nullptr, hdr, nullptr, &m2);
            const char *name = r == Rescale::Nothing ? "nothing" : r == Rescale::InPlace ? "inplace" : "rebuild";
            int equal = -1;
            if (r == Rescale::InPlace) {
                equal = !fr && plan_serial::serialise(next) == plan_serial::serialise(fresh) && same_layout(next, fresh) ? 1 : 0;
                cur = std::move(next);
            } else if (r == Rescale::Rebuild) {
                if (fr) alive = false;
                else { cur = fresh; maps = m2; }
            }
            finalEqual = !fr && plan_serial::serialise(cur) == plan_serial::serialise(fresh) && same_layout(cur, fresh);
            std::printf("%s{\"size\": [%u, %u], \"answer\": \"%s\", \"equal\": %d, \"status\": %d, \"text\": %s, \"form\": %s, \"tile_lists\": %d, \"mask_lists\": %d, "
                        "\"overlap\": %d, \"upscale\": %d, \"fused_cells\": [%d, %d], \"cells\": [%d, %d], \"out\": [%u, %u], \"resolve_in_staging\": %d}",
                        i ? ", " : "", w, h, name, equal, fr.status, quoted(fr.text).c_str(), fr ? "\"\"" : quoted(form_name(fresh.form)).c_str(),
                        (int)fresh.tileLists, (int)fresh.maskLists, (int)fresh.overlapOutside, (int)fresh.doUpscale, fresh.fusedCellsW, fresh.fusedCellsH,
                        fresh.cellsW, fresh.cellsH, fresh.outputWidth, fresh.outputHeight, fr ? 0 : (int)resolve_in_staging(fresh, fresh.ownedFormat));
        }
        std::printf("], \"alive\": %d, \"final_equal\": %d}\n", (int)alive, (int)finalEqual);
    }
    return 0;
}

static int taps(std::istream &f)
{
    uint32_t inW, inH, outW, outH;
    while (f >> inW >> inH >> outW >> outH) {
        const uint32_t tapYOff = (outW + 31u) & ~31u;
        std::vector<BilinTap> t((size_t)tapYOff + outH + 64, BilinTap{0, 0.0f});
        for (uint32_t i = 0; i < tapYOff + outH; ++i) t[i] = tap_table_entry(i, outW, outH, inW, inH, tapYOff);
        plan_serial::Writer w;
        w.u64(t.size());
        for (const BilinTap &b : t) { w.i32(b.i0); w.f32(b.frac); }
        std::printf("{\"in\": [%u, %u], \"out\": [%u, %u], \"taps\": \"%016llx\"}\n", inW, inH, outW, outH, (unsigned long long)plan_serial::fnv1a64(w.s));
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 3 || (std::strcmp(argv[1], "walk") && std::strcmp(argv[1], "taps"))) {
        std::fprintf(stderr, "usage: rescale_probe walk CASES | rescale_probe taps CASES\n");
        return 2;
    }
    std::ifstream f(argv[2]);
    if (!f) {
        std::fprintf(stderr, "cannot read %s\n", argv[2]);
        return 2;
    }
    return std::strcmp(argv[1], "walk") ? taps(f) : walk(f);
}
