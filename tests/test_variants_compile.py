"""Every measurement / mutation macro the Makefile documents still type-checks.

The tests and tools drive these builds; a rename that breaks one (round 4: `half2_t` -> `hale2_t` inside a measurement
macro's block) makes its build unusable without anybody noticing.  Syntax-only hipcc passes (templates are instantiated,
no code generation): ~4 s each, run four at a time.
"""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openvr_fsr_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# macros that live in the product sources (Makefile header)
IN_TREE = [
    ("fsr_kernels.hip", "-DOVRFSR_TIE_AUDIT"),
    ("fsr_kernels.hip", "-DOVRFSR_RCAS_NO_DPP"),
    ("postprocessor.cpp", "-DOVRFSR_MUTATE_NO_JOIN"),
    ("postprocessor.cpp", "-DOVRFSR_SERIAL"),
]

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def _syntax(tu, flags):
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", "-Wno-unused-function", "-ffp-contract=on"]
    cmd += ["-x", "hip"] if tu.endswith(".cpp") else ["-fno-slp-vectorize"]
    cmd += flags.split() + ["-fsyntax-only", tu]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    return (tu, flags, r.returncode, r.stderr[-2000:])


def test_in_tree_macros_compile():
    with ThreadPoolExecutor(4) as ex:
        res = list(ex.map(lambda a: _syntax(*a), IN_TREE))
    bad = [r for r in res if r[2] != 0]
    assert not bad, bad

