"""input_copy_bytes (csrc/fsr_sizes.h): the bytes of ONE image of each copy of its input the launch manager owns -- the resolve / unpack
pass's destination, the BGRA8 re-order's, the HDR domain's mapped RGBA32F copy -- as a pure function of (format, width, height) that a
host compiler can call (no GPU needed).  The build sizes the copies by it at the maximum input size and every apply at the submission's, so
"a re-scale creates nothing" holds while both ask the same function; here the function as compiled is compared with its restatement in
Python, on every input format class and at the sizes where the row padding and the 32-bit range matter."""
import os
import shutil
import subprocess

import pytest

from openvr_fsr_amd._capi import (FORMAT_BGRA8, FORMAT_R11G11B10F, FORMAT_RGBA8, FORMAT_RGBA16F, FORMAT_RGBA32F, FORMAT_SAMPLES_SHIFT,
                                  format_ms)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openvr_fsr_amd", "csrc")

FORMATS = [FORMAT_RGBA8, format_ms(FORMAT_RGBA8, 4), FORMAT_BGRA8, format_ms(FORMAT_BGRA8, 2), format_ms(FORMAT_RGBA16F, 8),
           FORMAT_R11G11B10F, format_ms(FORMAT_R11G11B10F, 4), FORMAT_RGBA32F]
# 3x2: the row bytes of a 4-byte texel are no multiple of 16; 4x1: exactly 16; 96x80: the suite's small shape; 16384^2: the largest image
SIZES = [(1, 1), (3, 2), (4, 1), (5, 3), (96, 80), (16384, 16384)]

# bytes of the texel the pipeline sees in the submission's place: BGRA8 re-ordered to RGBA8, R11G11B10F unpacked to RGBA16F
PIPELINE_TEXEL = {FORMAT_RGBA8: 4, FORMAT_BGRA8: 4, FORMAT_RGBA16F: 8, FORMAT_R11G11B10F: 8, FORMAT_RGBA32F: 16}


def copy_bytes(fmt, w, h):
    """(resolved, re-ordered, mapped): single-sample rows padded to 16 bytes; tight RGBA8; tight RGBA32F.  The sample count does not enter."""
    texel = PIPELINE_TEXEL[fmt & ((1 << FORMAT_SAMPLES_SHIFT) - 1)]
    return (w * texel + 15) // 16 * 16 * h, w * h * 4, w * h * 16


PROBE = r"""
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include "fsr_sizes.h"
using namespace ovrfsr;
static_assert(std::is_same<decltype(input_copy_bytes(InputCopy::Mapped, 0u, 1u, 1u)), uint64_t>::value, "64-bit: 16384^2 x 16 B is 4 GiB");
int main(int argc, char **argv)
{
    for (int i = 1; i + 2 < argc; i += 3) {
        const uint32_t f = (uint32_t)strtoul(argv[i], nullptr, 10), w = (uint32_t)strtoul(argv[i + 1], nullptr, 10), h = (uint32_t)strtoul(argv[i + 2], nullptr, 10);
        printf("%llu %llu %llu\n", (unsigned long long)input_copy_bytes(InputCopy::Resolved, f, w, h),
               (unsigned long long)input_copy_bytes(InputCopy::Reordered, f, w, h), (unsigned long long)input_copy_bytes(InputCopy::Mapped, f, w, h));
    }
    return 0;
}
"""


def test_compiled_sizes_equal_the_python_restatement(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.run([cxx, "-std=c++17", "-O1", "-w", "-I" + CSRC, str(src), "-o", str(exe)], check=True)
    cases = [(f, w, h) for f in FORMATS for w, h in SIZES]
    out = subprocess.run([str(exe)] + [str(v) for c in cases for v in c], check=True, capture_output=True, text=True, timeout=60).stdout
    got = [tuple(int(v) for v in line.split()) for line in out.splitlines()]
    assert len(got) == len(cases)
    for (f, w, h), g in zip(cases, got):
        print("format %#6x %5d x %5d: resolved %11d  re-ordered %11d  mapped %11d" % ((f, w, h) + g))
        assert g == copy_bytes(f, w, h), (f, w, h, g)
    # known answers: the padded rows, and the sizes that do not fit 32 bits
    assert copy_bytes(FORMAT_RGBA8, 3, 2) == (32, 24, 96) and copy_bytes(FORMAT_RGBA8, 4, 1) == (16, 16, 64)
    assert copy_bytes(FORMAT_R11G11B10F, 5, 3) == (48 * 3, 60, 240)
    assert copy_bytes(FORMAT_RGBA32F, 16384, 16384) == (1 << 32, 1 << 30, 1 << 32)
