"""rcas_dpp_small (csrc/fsr_sizes.h): which height rcas_dpp_kernel's workgroups take for an unmasked launch, as a pure function of
(outW, outH, batch) that a host compiler can call (no GPU needed).  The rule as compiled is compared with its independent restatement in
Python (tests/test_gpu_exact_stores.py, dpp_rows) at every edge of the rule: the workgroup counts of the 32-row grid where the number of
rounds of resident workgroups (2048) changes for one of the two heights, and the `< 16 * kRcasResident` end of the rule."""
import os
import shutil
import subprocess

import pytest

from tests.test_gpu_exact_stores import dpp_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openvr_fsr_amd", "csrc")

# (workgroups of the 32-row grid, rows): worked out by hand from the rule
EDGES = [(1, 16), (1024, 16), (1025, 32), (2048, 32), (2049, 16), (3073, 32), (30721, 16), (32767, 32), (32768, 32)]
# tx * ty * n = workgroups: outW = 62 * tx, outH = 32 * ty, batch = n
FACTORS = {1: (1, 1, 1), 1024: (32, 32, 1), 1025: (25, 41, 1), 2048: (32, 32, 2), 2049: (3, 683, 1), 3073: (7, 1, 439), 30721: (31, 991, 1),
           32767: (7, 31, 151), 32768: (32, 32, 32)}
# extents that are no multiple of the tile: one pixel more is one tile more (a 32-row grid of 1024 + 32 and of 1024 + 33 + 32 workgroups),
# one pixel less is none less; and the C2 eye image, alone and as a batch of two
RAGGED = [(62 * 32 + 1, 32 * 32, 1), (62 * 32 + 1, 32 * 32 + 1, 1), (62 * 32 - 61, 32 * 32 - 31, 1), (1920, 2133, 1), (1920, 2133, 2)]

PROBE = r"""
#include <cstdio>
#include <cstdlib>
#include "fsr_sizes.h"
int main(int argc, char **argv)
{
    for (int i = 1; i + 2 < argc; i += 3) {
        const int w = atoi(argv[i]), h = atoi(argv[i + 1]);
        const unsigned n = (unsigned)atoi(argv[i + 2]);
        const int rows = ovrfsr::rcas_dpp_small(w, h, n) ? 16 : ovrfsr::kRcasDppTileH;
        printf("%d %u\n", rows, ovrfsr::rcas_dpp_tiles_x(w) * ovrfsr::rcas_dpp_tiles_y(h, ovrfsr::kRcasDppTileH) * n);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("rcas_dpp_rule")
    src, exe = tmp / "probe.cpp", tmp / "probe"
    src.write_text(PROBE)
    subprocess.run([cxx, "-std=c++17", "-O1", "-w", "-I" + CSRC, str(src), "-o", str(exe)], check=True)

    def run(shapes):
        out = subprocess.run([str(exe)] + [str(v) for s in shapes for v in s], check=True, capture_output=True, text=True, timeout=60).stdout
        return [tuple(int(v) for v in line.split()) for line in out.splitlines()]
    return run


def test_python_restatement_gives_the_table():
    for wgs, rows in EDGES:
        tx, ty, n = FACTORS[wgs]
        assert tx * ty * n == wgs
        assert dpp_rows(62 * tx, 32 * ty, n) == rows, (wgs, rows)


def test_compiled_rule_equals_the_python_restatement(rule):
    shapes = [(62 * tx, 32 * ty, n) for tx, ty, n in (FACTORS[wgs] for wgs, _ in EDGES)] + RAGGED
    got = rule(shapes)
    assert len(got) == len(shapes)
    for (w, h, n), (rows, wgs) in zip(shapes, got):
        print("%5d x %5d x %3d: %5d workgroups, %2d rows (python: %d)" % (w, h, n, wgs, rows, dpp_rows(w, h, n)))
        assert wgs == ((w + 61) // 62) * ((h + 31) // 32) * n, (w, h, n, wgs)
        assert rows == dpp_rows(w, h, n), (w, h, n, rows)
    assert [(wgs, rows) for rows, wgs in got[:len(EDGES)]] == EDGES
