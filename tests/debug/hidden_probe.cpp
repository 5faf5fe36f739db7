// tests/debug/hidden_probe.cpp -- the planner under a hidden-area mesh (csrc/pipeline_plan.cpp, HiddenArea) on its own: no HIP, no device.
// tests/test_hidden_area.py compiles this file with pipeline_plan.cpp, constants.cpp and nis_config.cpp under -fsanitize=address,undefined
// and runs it as a child.
//
//   hidden_probe CASES           one JSON line per line of the file CASES: the case line of tests/debug/plan_probe.cpp, followed by
//       trianglesLeft trianglesRight and then 6 floats (u v u v u v) per triangle, the left mesh first
//   Each line reports
//     "no_mesh_equal"   the plan of the six-argument call and the plan of the call with an EMPTY mesh, serialised by value (plan_serial.h), are equal
//     "form", "form_plain"   the form with the mesh and of the six-argument call
//     "tile_lists", "hidden_area", "lists_shared", "tiles", "tile" [w, h], "skipped" [l, r]
//     "mask_mode" [l, r]   the plan's maskMode per eye (0 all inside, 1 all outside, 2 mixed), "centre" per eye the four mask centres
//     "inside", "ring", "outside", "rcas"   per eye, the tile indices of each list segment as the plan holds them
//     "spans"           per eye, [x0, tileRow, xEnd] of every RCAS segment
//     "hidden"          per eye, the tile map the rule gives for the planned output size (hidden_tiles), row-major
//     "digest"          the FNV-1a digest of the plan with the mesh, serialised by value (plan_serial.h)
#include <cstdio>
#include <cstring>
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
        std::fprintf(stderr, "usage: hidden_probe CASES\n");
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
        uint32_t count[2] = {0, 0};
        plan_serial::parse_case(in, k);
        in >> count[0] >> count[1];
        const ovrfsr_config &c = k.cfg;
        const uint32_t format = k.format, w = k.width, h = k.height;
        const int oneEye = k.oneEye;
        std::vector<float> uv[2];
        for (int eye = 0; eye < 2 && in; ++eye) {
            uv[eye].resize(6 * (size_t)count[eye]);
            for (float &x : uv[eye]) in >> x;
        }
        if (!in) {
            std::fprintf(stderr, "malformed case line: %s\n", line.c_str());
            return 2;
        }
        Plan plain, empty, p;
        const HiddenArea none;
        HiddenArea mesh;
        for (int eye = 0; eye < 2; ++eye) { mesh.uv[eye] = uv[eye].data(); mesh.triangles[eye] = count[eye]; }
        const Refusal r0 = plan_pipeline(c, format, w, h, oneEye != 0, &plain);
        const Refusal r1 = plan_pipeline(c, format, w, h, oneEye != 0, &empty, &none);
        const Refusal r = plan_pipeline(c, format, w, h, oneEye != 0, &p, &mesh);
        std::printf("{\"id\": \"%s\", \"status\": %d, \"no_mesh_equal\": %d", k.id.c_str(), r.status,
                    (int)(r0.status == r1.status && r0.status == r.status && plan_serial::serialise(plain) == plan_serial::serialise(empty)));
        if (!r) {
            // the tile size is the plan's; the counts are recomputed from the output size, so that the grid does not vouch for itself
            const uint32_t tw = p.grid.tileW, th = p.grid.tileH;
            const uint32_t tx = (p.outputWidth + tw - 1) / tw, ty = (p.outputHeight + th - 1) / th;
            if (p.grid.tx != tx || p.grid.ty != ty) {
                std::fprintf(stderr, "%s: the grid counts %u x %u tiles, the output size gives %u x %u\n", k.id.c_str(), p.grid.tx, p.grid.ty, tx, ty);
                return 3;
            }
            std::printf(", \"form\": \"%s\", \"form_plain\": \"%s\", \"out\": [%u, %u], \"tile_lists\": %d, \"hidden_area\": %d, \"lists_shared\": %d, "
                        "\"tiles\": %u, \"tile\": [%u, %u], \"skipped\": [%u, %u]", form_name(p.form), form_name(plain.form), p.outputWidth, p.outputHeight,
                        (int)p.tileLists, (int)p.hiddenArea, (int)p.listsShared, tx * ty, tw, th, p.nSkipped[0], p.nSkipped[1]);
            std::printf(", \"mask_mode\": [%u, %u], \"centre\": [[%u, %u, %u, %u], [%u, %u, %u, %u]]", p.maskMode[0], p.maskMode[1], p.centre[0][0],
                        p.centre[0][1], p.centre[0][2], p.centre[0][3], p.centre[1][0], p.centre[1][1], p.centre[1][2], p.centre[1][3]);
            print_list("inside", p, p.listOffInside, p.nInside);
            print_list("ring", p, p.listOffRing, p.nRing);
            print_list("outside", p, p.listOffOutside, p.nOutside);
            print_list("rcas", p, p.listOffRcas, p.nRcas);
            std::printf(", \"spans\": [");
            for (int eye = 0; eye < 2; ++eye) {
                std::printf("%s[", eye ? ", " : "");
                for (uint32_t i = 0; i < p.nSpans[eye]; ++i) {
                    const uint32_t a = p.spans[2 * (p.spanOff[eye] + i)], xEnd = p.spans[2 * (p.spanOff[eye] + i) + 1];
                    std::printf("%s[%u, %u, %u]", i ? ", " : "", a & 0xffffu, a >> 16, xEnd);
                }
                std::printf("]");
            }
            std::printf("], \"hidden\": [");
            std::vector<uint8_t> map((size_t)tx * ty);
            for (int eye = 0; eye < 2; ++eye) {
                if (oneEye) hidden_tiles(mesh.uv[eye], mesh.triangles[eye], nullptr, 0, false, p.outputWidth, p.outputHeight, tw, th, map.data());
                else hidden_tiles(mesh.uv[0], mesh.triangles[0], mesh.uv[1], mesh.triangles[1], true, p.outputWidth, p.outputHeight, tw, th, map.data());
                std::printf("%s[", eye ? ", " : "");
                for (size_t i = 0; i < map.size(); ++i) std::printf("%s%u", i ? ", " : "", map[i]);
                std::printf("]");
            }
            std::printf("], \"digest\": \"%s\"", plan_serial::digest(p).c_str());
        }
        std::printf("}\n");
    }
    return 0;
}
