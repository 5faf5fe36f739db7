// tests/debug/hdr_probe.cpp -- the planner under ovrfsr_set_hdr_domain (csrc/pipeline_plan.cpp, plan_pipeline's `hdrDomain`) on its own: no
// HIP, no device.  tests/test_hdr_domain.py compiles this file with pipeline_plan.cpp, constants.cpp and nis_config.cpp under
// -fsanitize=address,undefined and runs it as a child.
//
//   hdr_probe CASES           one JSON line per line of the file CASES: the case line of tests/debug/plan_probe.cpp, followed by
//       hdrDomain triangles and then 6 floats (u v u v u v) per triangle: one hidden-area mesh, set for both eyes
//   Each line reports
//     "status", "form", "input", "pipeline", "mid", "owned", "hdr_domain", "tile_lists", "hidden_area", "skipped" [l, r]
//     "inside", "ring", "outside", "rcas", "spans"   per eye, the entries of each list segment
//     "digest"            the FNV-1a digest of the plan, serialised by value (plan_serial.h)
//     "digest_pipeline"   the same with inputFormat and ownedFormat -- what the setting leaves the submission's -- set to 0: equal for two
//                         plans that run the same pipeline
//     "digest_plain"      the digest of the six-argument call's plan (no mesh, no setting); "" where that call is refused
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "../../openvr_fsr_amd/csrc/pipeline_plan.h"
#include "plan_serial.h"

using namespace ovrfsr;

static void print_list(const char *name, const Plan &p, const size_t off[2], const uint32_t n[2])
{
    std::printf(", \"%s\": [", name);
    for (int eye = 0; eye < 2; ++eye) {
        std::printf("%s[", eye ? ", " : "");
        for (uint32_t i = 0; i < n[eye]; ++i) std::printf("%s%u", i ? ", " : "", p.lists[off[eye] + i]);
        std::printf("]");
    }
    std::printf("]");
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: hdr_probe CASES\n");
        return 2;
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
        int hdr = 0;
        uint32_t count = 0;
        plan_serial::parse_case(in, k);
        in >> hdr >> count;
        std::vector<float> uv(in ? 6 * (size_t)count : 0);
        for (float &x : uv) in >> x;
        if (!in) {
            std::fprintf(stderr, "malformed case line: %s\n", line.c_str());
            return 2;
        }
        HiddenArea mesh;
        for (int eye = 0; eye < 2; ++eye) { mesh.uv[eye] = uv.data(); mesh.triangles[eye] = count; }
        Plan plain, p;
        const Refusal r0 = plan_pipeline(k.cfg, k.format, k.width, k.height, k.oneEye != 0, &plain);
        const Refusal r = plan_pipeline(k.cfg, k.format, k.width, k.height, k.oneEye != 0, &p, count ? &mesh : nullptr, hdr);
        std::printf("{\"id\": \"%s\", \"status\": %d, \"status_plain\": %d, \"digest_plain\": \"%s\"", k.id.c_str(), r.status, r0.status,
                    r0 ? "" : plan_serial::digest(plain).c_str());
        if (!r) {
            std::printf(", \"form\": \"%s\", \"input\": %u, \"pipeline\": %u, \"mid\": %u, \"owned\": %u, \"hdr_domain\": %d, \"tile_lists\": %d, "
                        "\"hidden_area\": %d, \"skipped\": [%u, %u]", form_name(p.form), p.inputFormat, p.pipelineFormat, p.intermediateFormat,
                        p.ownedFormat, (int)p.hdrDomain, (int)p.tileLists, (int)p.hiddenArea, p.nSkipped[0], p.nSkipped[1]);
            print_list("inside", p, p.listOffInside, p.nInside);
            print_list("ring", p, p.listOffRing, p.nRing);
            print_list("outside", p, p.listOffOutside, p.nOutside);
            print_list("rcas", p, p.listOffRcas, p.nRcas);
            std::printf(", \"spans\": [%u, %u], \"resolve_in_staging\": %d, \"digest\": \"%s\"", p.nSpans[0], p.nSpans[1],
                        (int)resolve_in_staging(p, k.dest < 0 ? p.ownedFormat : (uint32_t)k.dest), plan_serial::digest(p).c_str());
            Plan body = p;
            body.inputFormat = body.ownedFormat = 0;
            std::printf(", \"digest_pipeline\": \"%s\"", plan_serial::digest(body).c_str());
        }
        std::printf("}\n");
    }
    return 0;
}
