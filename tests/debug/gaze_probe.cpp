// tests/debug/gaze_probe.cpp -- the planner's re-aim step (csrc/pipeline_plan.cpp, reaim_pipeline) on its own: no HIP, no device.
// tests/test_gaze.py compiles this file with pipeline_plan.cpp, constants.cpp and nis_config.cpp under -fsanitize=address,undefined and runs
// it as a child, like plan_probe.
//
//   gaze_probe sweep CASES      one JSON line per line of CASES (the 25 fields of plan_serial::Case, then `full`: 1 = the 9x9 grid of gazes
//                               over [-0.25, 1.25]^2 and the named gazes, 0 = the named gazes only):
//       from each of three previous gazes, to every gaze: the re-aim step's answer against plan_pipeline on the effective configuration --
//       "rebuild" exactly where that plan differs in a field no re-aim may move (or in resolve_in_staging's "every group inside"), "nothing"
//       exactly where the centres are equal, else a plan equal to it in every field but the list offsets, lists, records and spans equal in
//       content and count, inside the regions.  Reports the counts of the three answers, the first violations ("errors"), and the inside
//       list of eye 0 for each named gaze ("named_inside").
//   gaze_probe sequence CASES   per line: the 25 fields, the number of steps, then per step `setL xL yL setR xR yR`: what the launch manager
//       does step by step (PostProcessor::AimGaze) -- "first" (the first build), "nothing", "reaim" or "rebuild" -- one JSON line per case.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../openvr_fsr_amd/csrc/pipeline_plan.h"
#include "plan_serial.h"

using namespace ovrfsr;

struct Gaze { float x, y; };
static const Gaze kNamed[7] = {{0.5f, 0.5f}, {0.2f, 0.3f}, {0.8f, 0.7f}, {0.0f, 0.0f}, {1.0f, 1.0f}, {0.37f, 0.61f}, {2.0f, 2.0f}}; // G, then OUT

static ovrfsr_config with_gaze(ovrfsr_config c, Gaze l, Gaze r)
{
    c.proj_centre[0] = l.x; c.proj_centre[1] = l.y; c.proj_centre[2] = r.x; c.proj_centre[3] = r.y;
    return c;
}

// the plan with everything a re-aim may move taken out: what is left has to be equal, byte for byte of its serialisation
static std::string fixed_part(const Plan &p, const std::vector<BilinTap> &taps)
{
    Plan q;
    static_cast<PlanFields &>(q) = p;
    q.taps = taps;
    std::memset(q.centre, 0, sizeof q.centre);
    for (int e = 0; e < 2; ++e) {
        q.maskMode[e] = 0;
        q.nInside[e] = q.nOutside[e] = q.nRing[e] = q.nSpans[e] = q.nRcas[e] = q.nSkipped[e] = 0;
        q.listOffInside[e] = q.listOffOutside[e] = q.listOffRing[e] = q.listOffRcas[e] = q.spanOff[e] = 0;
    }
    q.listsShared = false;
    return plan_serial::serialise(q);
}

static bool all_inside(const Plan &p) { return p.maskMode[0] == MASK_ALL_INSIDE && p.maskMode[1] == MASK_ALL_INSIDE; }

// "" or what differs between a gaze-capable plan `got` (taps: `taps`) and the plain plan `want` of the same configuration
static std::string compare(const Plan &got, const std::vector<BilinTap> &taps, const Plan &want, bool records)
{
    if (fixed_part(got, taps) != fixed_part(want, want.taps)) return "a field no re-aim may move differs";
    if (std::memcmp(got.centre, want.centre, sizeof got.centre) || got.maskMode[0] != want.maskMode[0] || got.maskMode[1] != want.maskMode[1]) return "centre / maskMode";
    if (got.listsShared != want.listsShared) return "listsShared";
    if (!got.gazeCapable) return "not gaze-capable";
    if (!got.tileLists) return got.lists.empty() && got.spans.empty() ? "" : "tables without tile lists";
    if (got.lists.size() != 2 * got.listRegion || got.spans.size() != 4 * got.spanRegion) return "the tables are not the regions";
    if (records && got.recs.size() != 4 * got.lists.size()) return "one record per list entry";
    for (int e = 0; e < 2; ++e) {
        if (got.nInside[e] != want.nInside[e] || got.nRing[e] != want.nRing[e] || got.nOutside[e] != want.nOutside[e] || got.nRcas[e] != want.nRcas[e] ||
            got.nSpans[e] != want.nSpans[e] || got.nSkipped[e] != want.nSkipped[e])
            return "a count";
        if (got.listOffInside[e] != (size_t)e * got.listRegion || got.listOffRing[e] != got.listOffInside[e] + got.nInside[e]) return "region start / ring behind inside";
        if ((want.listOffRcas[e] == want.listOffInside[e]) != (got.listOffRcas[e] == got.listOffInside[e])) return "RCAS's own list";
        const size_t go[4] = {got.listOffInside[e], got.listOffRing[e], got.listOffOutside[e], got.listOffRcas[e]};
        const size_t wo[4] = {want.listOffInside[e], want.listOffRing[e], want.listOffOutside[e], want.listOffRcas[e]};
        const uint32_t n[4] = {got.nInside[e], got.nRing[e], got.nOutside[e], got.nRcas[e]};
        for (int k = 0; k < 4; ++k) {
            if (go[k] + n[k] > (size_t)(e + 1) * got.listRegion) return "a list leaves its region";   // the capacity bound
            for (uint32_t i = 0; i < n[k]; ++i) {
                if (got.lists[go[k] + i] != want.lists[wo[k] + i]) return "a list entry";
                if (records && std::memcmp(&got.recs[4 * (go[k] + i)], &want.recs[4 * (wo[k] + i)], 16)) return "a record";
            }
        }
        if (got.spanOff[e] != (size_t)e * got.spanRegion || got.nSpans[e] > got.spanRegion) return "a span leaves its region";
        if (got.nSpans[e] && std::memcmp(&got.spans[2 * got.spanOff[e]], &want.spans[2 * want.spanOff[e]], 8 * (size_t)got.nSpans[e])) return "a span";
    }
    return "";
}

static std::string quoted(const std::string &s)
{
    std::string q = "\"";
    for (char c : s) {
        if (c == '"' || c == '\\') q += '\\';
        q += c;
    }
    return q + "\"";
}

static int sweep(std::istream &f)
{
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        plan_serial::Case k;
        int full = 0;
        if (!plan_serial::parse_case(in, k) || !(in >> full)) { std::fprintf(stderr, "malformed case line: %s\n", line.c_str()); return 2; }
        std::vector<std::pair<Gaze, Gaze>> targets; // (left, right)
        for (int i = 0; i < 6; ++i) targets.push_back({kNamed[i], kNamed[(i + 1) % 6]});
        for (int i = 0; i < 7; ++i) targets.push_back({kNamed[i], kNamed[i]});
        targets.push_back({kNamed[0], kNamed[6]});
        targets.push_back({kNamed[6], kNamed[1]});
        targets.push_back({Gaze{0.51f, 0.5f}, kNamed[0]});   // a sub-tile move from (0.5, 0.5)
        targets.push_back({Gaze{0.5001f, 0.5f}, kNamed[0]}); // ... and one below a pixel
        if (full)
            for (int j = 0; j < 9; ++j)
                for (int i = 0; i < 9; ++i) {
                    const Gaze g{-0.25f + 1.5f * (float)i / 8.0f, -0.25f + 1.5f * (float)j / 8.0f};
                    targets.push_back({g, Gaze{1.0f - g.x, g.y}});
                }
        const std::pair<Gaze, Gaze> starts[3] = {{kNamed[0], kNamed[0]}, {kNamed[1], kNamed[2]}, {kNamed[6], kNamed[6]}};

        long nothing = 0, inplace = 0, rebuild = 0, refused = 0;
        std::vector<std::string> errors;
        auto error = [&](const char *what, size_t s, size_t t, const std::string &why) {
            char buf[160];
            std::snprintf(buf, sizeof buf, "%s: start %zu, target %zu: ", what, s, t);
            if (errors.size() < 5) errors.push_back(buf + why);
        };
        std::vector<Plan> want(targets.size());
        for (size_t t = 0; t < targets.size(); ++t)
            if (plan_pipeline(with_gaze(k.cfg, targets[t].first, targets[t].second), k.format, k.width, k.height, k.oneEye != 0, &want[t])) ++refused;
        std::printf("{\"id\": %s, \"refused\": %ld", quoted(k.id).c_str(), refused);
        if (!refused) {
            for (size_t s = 0; s < 3; ++s) {
                Plan cur, plain;
                HiddenMaps maps;
                const ovrfsr_config c0 = with_gaze(k.cfg, starts[s].first, starts[s].second);
                if (plan_pipeline(c0, k.format, k.width, k.height, k.oneEye != 0, &cur, nullptr, OVRFSR_HDR_DOMAIN_LINEAR, &maps) ||
                    plan_pipeline(c0, k.format, k.width, k.height, k.oneEye != 0, &plain)) { error("plan", s, 0, "refused"); continue; }
                const std::string first = compare(cur, cur.taps, plain, true); // the gaze-capable plan itself: the plain one but for the offsets
                if (!first.empty()) error("gaze-capable plan", s, 0, first);
                for (size_t t = 0; t < targets.size(); ++t) {
                    Plan got;
                    const Reaim r = reaim_pipeline(cur, with_gaze(k.cfg, targets[t].first, targets[t].second), maps, &got);
                    const bool same = !std::memcmp(cur.centre, want[t].centre, sizeof cur.centre);
                    const bool moves = fixed_part(cur, cur.taps) != fixed_part(want[t], want[t].taps) || all_inside(cur) != all_inside(want[t]);
                    const Reaim expect = same ? Reaim::Nothing : moves ? Reaim::Rebuild : Reaim::InPlace;
                    if (r != expect) { error("answer", s, t, "got " + std::to_string((int)r) + ", expected " + std::to_string((int)expect)); continue; }
                    if (r == Reaim::Nothing) { ++nothing; continue; }
                    if (r == Reaim::Rebuild) { ++rebuild; continue; }
                    ++inplace;
                    const std::string why = compare(got, cur.taps, want[t], true);
                    if (!why.empty()) error("re-aimed plan", s, t, why);
                    if (!got.taps.empty()) error("re-aimed plan", s, t, "carries tap tables");
                }
            }
            std::printf(", \"nothing\": %ld, \"inplace\": %ld, \"rebuild\": %ld, \"tile\": [%u, %u], \"tile_lists\": %d, \"named_inside\": [", nothing, inplace, rebuild,
                        want[0].grid.tileW, want[0].grid.tileH, (int)want[6].tileLists);
            for (int i = 0; i < 7; ++i) { // targets[6 + i]: both eyes at named gaze i
                const Plan &p = want[6 + i];
                std::printf("%s[", i ? ", " : "");
                for (uint32_t j = 0; p.tileLists && j < p.nInside[0]; ++j) std::printf("%s%u", j ? ", " : "", p.lists[p.listOffInside[0] + j]);
                std::printf("]");
            }
            std::printf("], \"named_mode\": [");
            for (int i = 0; i < 7; ++i) std::printf("%s%u", i ? ", " : "", want[6 + i].maskMode[0]);
            std::printf("], \"errors\": [");
            for (size_t i = 0; i < errors.size(); ++i) std::printf("%s%s", i ? ", " : "", quoted(errors[i]).c_str());
            std::printf("]");
        }
        std::printf("}\n");
    }
    return 0;
}

static int sequence(std::istream &f)
{
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        plan_serial::Case k;
        int steps = 0;
        if (!plan_serial::parse_case(in, k) || !(in >> steps)) { std::fprintf(stderr, "malformed case line: %s\n", line.c_str()); return 2; }
        Plan cur;
        HiddenMaps maps;
        bool planned = false;
        std::printf("{\"id\": %s, \"steps\": [", quoted(k.id).c_str());
        for (int s = 0; s < steps; ++s) {
            int setL = 0, setR = 0;
            Gaze l{}, r{};
            if (!(in >> setL >> l.x >> l.y >> setR >> r.x >> r.y)) { std::fprintf(stderr, "malformed step in: %s\n", line.c_str()); return 2; }
            ovrfsr_config c = k.cfg;
            if (setL) { c.proj_centre[0] = l.x; c.proj_centre[1] = l.y; }
            if (setR) { c.proj_centre[2] = r.x; c.proj_centre[3] = r.y; }
            const char *what = "nothing";
            Plan got;
            const Reaim a = planned ? reaim_pipeline(cur, c, maps, &got, false) : Reaim::Rebuild;
            if (a == Reaim::InPlace) {
                static_cast<PlanFields &>(cur) = got;
                what = "reaim";
            } else if (a == Reaim::Rebuild) {
                what = planned ? "rebuild" : "first";
                maps = HiddenMaps{};
                if (plan_pipeline(c, k.format, k.width, k.height, k.oneEye != 0, &cur, nullptr, OVRFSR_HDR_DOMAIN_LINEAR, (setL || setR) ? &maps : nullptr)) what = "refused";
                planned = true;
            }
            std::printf("%s\"%s\"", s ? ", " : "", what);
        }
        std::printf("]}\n");
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 3 || (std::strcmp(argv[1], "sweep") && std::strcmp(argv[1], "sequence"))) {
        std::fprintf(stderr, "usage: gaze_probe sweep CASES | gaze_probe sequence CASES\n");
        return 2;
    }
    std::ifstream f(argv[2]);
    if (!f) {
        std::fprintf(stderr, "cannot read %s\n", argv[2]);
        return 2;
    }
    return std::strcmp(argv[1], "sweep") ? sequence(f) : sweep(f);
}
