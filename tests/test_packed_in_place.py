"""R11G11B10F eye images decoded inside kernel staging (no GPU needed): the product build holds instances of easu_fast_kernel, fused_kernel
and easu_outside_kernel whose input format is the packed word, they cost no more registers or LDS than their RGBA16F twins, the planner's
resolve_in_staging sends exactly the forms with a fixed-pitch kernel to them, no existing kernel moved, and the measurement build
(-DOVRFSR_PACKED_RESOLVE_PASS: the pass everywhere, as before) type-checks."""
import os
import re
import subprocess

import pytest

from tests import isa
from tests.test_kernel_resources import _alloc, kernels  # noqa: F401  (the code-object fixture)
from tests.test_pipeline_plan import FORM_TABLE, M, MATRIX, _line, _plan, probe  # noqa: F401  (the planner probe fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openvr_fsr_amd", "csrc")
RGBA8, RGBA16F, RGBA32F, R11G11B10F = 0, 1, 2, 6

EASU = r"ovrfsr_fast16easu_fast_kernelILi6ELi([012])ELi(28|32|40)ELb([01])E"
FUSED = r"ovrfsr_fast12fused_kernelILi6ELi([12])ELi([012])ELi(32|40)ELi256E"
OUTSIDE = r"ovrfsr_fast19easu_outside_kernelILi6ELi([012])ELi(n1|[012])E"


def _new(kernels):  # noqa: F811
    return {k: v for k, v in kernels.items() if re.search(r"(easu_fast_kernel|fused_kernel|easu_outside_kernel)ILi6E", k)}


# ---- 1. the instances ----------------------------------------------------------------------------------------------------------


def test_instances_exist(kernels):  # noqa: F811
    easu = {re.search(EASU, k).groups() for k in kernels if re.search(EASU, k)}
    assert easu == {(o, p, m) for o in "012" for p in ("28", "32", "40") for m in "01"}, sorted(easu)
    fused = {re.search(FUSED, k).groups() for k in kernels if re.search(FUSED, k)}
    assert fused == {(m, o, p) for m in "12" for o in "012" for p in ("32", "40")}, sorted(fused)
    outside = {re.search(OUTSIDE, k).groups() for k in kernels if re.search(OUTSIDE, k)}
    assert outside == {(o, m) for o in "012" for m in ("n1", "0", "1", "2")}, sorted(outside)
    # nothing else reads the word: 18 + 12 + 12 kernels, no generic-pitch easu_kernel, no strict-namespace kernel
    assert len(_new(kernels)) == 42, sorted(_new(kernels))
    assert not [k for k in kernels if "ovrfsr_strict" in k and re.search(r"_kernelILi6E", k)]
    assert not [k for k in kernels if re.search(r"(ovrfsr_fast11easu_kernel|rcas_\w*kernel|outside_staged_kernel)ILi\d+ELi6E|easu_kernelILi6E", k)]


def test_instances_have_a_code_object_of_their_own(tmp_path):
    """The instances are built from a translation unit of their own (csrc/fsr_packed_kernels.hip), so they sit in a code object of their own:
    the runtime loads a code object at the first launch from it, and a process that never submits the format loads exactly the kernels
    it loaded before these existed (with them in fsr_kernels.hip's code object, 18 % larger, the thread-stress driver under the host
    sanitizers no longer left the runtime's exit-time teardown alive: tests/test_sanitizers.py)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("isa_costs", os.path.join(ROOT, "tools", "isa_costs.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    if not os.path.exists(isa.LIB):
        pytest.fail("libopenvr_fsr_amd.so is not built: run __graft_entry__.build()")
    per_object = []
    for elf in tool.extract_code_objects(isa.LIB, str(tmp_path)):
        syms = subprocess.run([tool._tool("llvm-readelf"), "--symbols", "--wide", elf], check=True, capture_output=True, text=True).stdout
        names = {m.group(1) for m in re.finditer(r"\sFUNC\s.*\s(_Z\S+_kernel\S*)$", syms, re.M)}
        per_object.append(names)
    packed = [n for n in per_object if any("_kernelILi6E" in k for k in n)]
    assert len(per_object) == 3 and len(packed) == 1, [len(n) for n in per_object]
    assert len(packed[0]) == 42 and all("_kernelILi6E" in k for k in packed[0]), sorted(k for k in packed[0] if "_kernelILi6E" not in k)


# ---- 2. resources ----------------------------------------------------------------------------------------------------------------


def test_resources_match_the_rgba16f_twins(kernels):  # noqa: F811
    new = _new(kernels)
    assert len(new) == 42
    for k, v in new.items():
        twin = kernels[k.replace("ILi6E", "ILi1E", 1)]   # the same template arguments with input RGBA16F
        assert 512 // _alloc(v["vgpr_count"]) >= 512 // _alloc(twin["vgpr_count"]), (k, v["vgpr_count"], twin["vgpr_count"])
        assert v["group_segment_fixed_size"] == twin["group_segment_fixed_size"], (k, v["group_segment_fixed_size"], twin["group_segment_fixed_size"])
        assert not (v["vgpr_spill_count"] or v["sgpr_spill_count"] or v["private_segment_fixed_size"] or v["agpr_count"]), (k, v)
        assert v["max_flat_workgroup_size"] == 256, (k, v)


def test_packed_c5_pair_fits_one_simd(kernels):  # noqa: F811
    """tests/test_kernel_resources.py::test_c5_pair_fits_one_simd's rule for the packed C5 pair: 3 fused + 5 outside waves per SIMD"""
    fused = {k: v for k, v in kernels.items() if re.search(r"ovrfsr_fast12fused_kernelILi6ELi1ELi1ELi(32|40)ELi256E", k)}
    outside = {k: v for k, v in kernels.items() if re.search(r"ovrfsr_fast19easu_outside_kernelILi6ELi1ELi1E", k)}
    assert len(fused) == 2 and len(outside) == 1
    for k, v in {**fused, **outside}.items():
        assert _alloc(v["vgpr_count"]) <= 64, (k, v["vgpr_count"])
    assert 3 * max(_alloc(v["vgpr_count"]) for v in fused.values()) + 5 * max(_alloc(v["vgpr_count"]) for v in outside.values()) <= 512


# ---- 3. the planner --------------------------------------------------------------------------------------------------------------


def _case(name, fmt, want, shape=MATRIX, dest=-1, **cfg):
    iw, ih, ow, oh = shape
    return (name, _line(name, fmt, iw, ih, 1, dest, fsr_enabled=1, out_width=ow, out_height=oh, **cfg), want)


IN_PLACE = dict(resolve_in_staging=1, pipeline=RGBA16F)
PASS = dict(resolve_in_staging=0, pipeline=RGBA16F)
# minifying by 5/4: a 32-pixel tile's footprint is 40 + 4 cells, beyond the widest fixed pitch (40), and still within the generic kernel's LDS
# (the issue's example, 200x160 -> 128x102, is refused for RGBA16F too: "scale ratio needs more LDS than one tile may use")
WIDE = (160, 128, 128, 102)
PLAN_CASES = [
    _case("unmasked two-pass", R11G11B10F, dict(IN_PLACE, form="two-pass", mid=RGBA16F, owned=RGBA16F), radius=2.0),
    _case("masked default", R11G11B10F, dict(IN_PLACE, form="fused with masked outside tiles", mid=RGBA16F, owned=RGBA16F), **M),
    _case("reference_formats masked", R11G11B10F, dict(IN_PLACE, form="mask-sorted", mid=RGBA8, owned=RGBA8), reference_formats=1, **M),
    _case("reference_formats unmasked", R11G11B10F, dict(IN_PLACE, form="two-pass", mid=RGBA8, owned=RGBA8), reference_formats=1, radius=2.0),
    _case("EASU only into RGBA8", R11G11B10F, dict(IN_PLACE, form="upscale only"), dest=RGBA8, stage_mask=1, radius=2.0),
    _case("EASU only into RGBA16F", R11G11B10F, dict(IN_PLACE, form="upscale only"), dest=RGBA16F, stage_mask=1, radius=2.0),
    _case("EASU only into RGBA8, masked", R11G11B10F, dict(IN_PLACE, form="upscale only", tile_lists=1), dest=RGBA8, stage_mask=1, **M),
    _case("EASU only into RGBA32F, masked", R11G11B10F, dict(IN_PLACE, form="upscale only", tile_lists=1), dest=RGBA32F, stage_mask=1, **M),
    _case("masked default into RGBA8", R11G11B10F, dict(IN_PLACE, form="fused with masked outside tiles"), dest=RGBA8, **M),
    _case("EASU only into RGBA32F", R11G11B10F, dict(IN_PLACE, form="upscale only"), dest=RGBA32F, stage_mask=1, radius=2.0),
    _case("fused on request", R11G11B10F, dict(IN_PLACE, form="fused"), fused=1, radius=2.0),
    _case("fused on request, masked", R11G11B10F, dict(IN_PLACE, form="fused with masked outside tiles"), fused=1, **M),
    _case("masked two-pass (fused = 0), reference_formats", R11G11B10F, dict(IN_PLACE, form="two-pass", tile_lists=1, mid=RGBA8), fused=0, reference_formats=1, **M),
    _case("precision 3 with reference_formats", R11G11B10F, dict(IN_PLACE, form="mask-sorted", mid=RGBA8), precision=3, reference_formats=1, dest=RGBA8, **M),
    # the pass stays
    _case("strict", R11G11B10F, dict(PASS, form="two-pass"), precision=2, radius=2.0),
    _case("strict, masked", R11G11B10F, dict(PASS), precision=2, **M),
    _case("NIS", R11G11B10F, dict(PASS, form="upscale only"), use_nis=1, radius=2.0),
    _case("NIS, masked", R11G11B10F, dict(PASS, form="upscale only"), use_nis=1, **M),
    _case("sharpen only", R11G11B10F, dict(PASS, form="sharpen only"), shape=(96, 80, 96, 80), stage_mask=2),
    _case("multisampled", R11G11B10F | 4 << 8, dict(PASS), radius=2.0),
    _case("multisampled, masked", R11G11B10F | 4 << 8, dict(PASS), **M),
    _case("wide footprint", R11G11B10F, dict(PASS, form="two-pass"), shape=WIDE, radius=2.0),
    _case("wide footprint, masked", R11G11B10F, dict(PASS), shape=WIDE, **M),
    _case("wide footprint, EASU only", R11G11B10F, dict(PASS, form="upscale only"), shape=WIDE, stage_mask=1, radius=2.0),
    # masked launches whose bilinear fallback rounds a contracted blend to half, other than the default pair (half intermediate and half
    # destination): the pass, until their bytes are shown equal at full size (pipeline_plan.cpp, packed_in_staging)
    _case("EASU only into RGBA16F, masked", R11G11B10F, dict(PASS, form="upscale only", tile_lists=1), dest=RGBA16F, stage_mask=1, **M),
    _case("masked two-pass (fused = 0), half intermediate", R11G11B10F, dict(PASS, form="two-pass", tile_lists=1, mid=RGBA16F), fused=0, **M),
    _case("masked default into RGBA32F", R11G11B10F, dict(PASS, form="fused with masked outside tiles"), dest=RGBA32F, **M),
    _case("masked, float intermediate, into RGBA16F", R11G11B10F, dict(PASS, mid=RGBA32F), dest=RGBA16F, quantize_intermediate=0, **M),
    # other formats keep their answers
    _case("plain RGBA16F", RGBA16F, dict(resolve_in_staging=0, form="fused with masked outside tiles"), **M),
    _case("plain RGBA16F, unmasked", RGBA16F, dict(resolve_in_staging=0, form="two-pass"), radius=2.0),
]


def test_planner_sends_the_fixed_pitch_forms_in_place(probe):  # noqa: F811
    got = _plan(probe, [line for _, line, _ in PLAN_CASES])
    for (name, _, want), g in zip(PLAN_CASES, got):
        assert g["status"] == 0, (name, g)
        for k, v in want.items():
            assert g.get(k) == v, (name, k, v, g)
    # the four MS4-RGBA8 lines of the form table
    ms4 = [(n, line, w) for n, line, w in FORM_TABLE if n.startswith("MS4 RGBA8")]
    assert len(ms4) == 4
    for (name, _, want), g in zip(ms4, _plan(probe, [line for _, line, _ in ms4])):
        assert g["resolve_in_staging"] == want["resolve_in_staging"] and g["form"] == want["form"], (name, g)


def test_recorded_shapes_run_in_place(probe):  # noqa: F811
    """the measured shapes (C5: 2370^2 -> 3160^2, C2: 1440x1600 -> 1920x2133) have footprints inside the fixed pitches"""
    for shape in ((2370, 2370, 3160, 3160), (1440, 1600, 1920, 2133)):
        got = _plan(probe, [_case("masked", R11G11B10F, {}, shape=shape, **M)[1], _case("unmasked", R11G11B10F, {}, shape=shape, radius=2.0)[1]])
        assert [g["resolve_in_staging"] for g in got] == [1, 1], got


# ---- 4. fingerprints ---------------------------------------------------------------------------------------------------------------


def test_fingerprint_scope():
    if not os.path.exists(isa.LIB):
        pytest.fail("libopenvr_fsr_amd.so is not built: run __graft_entry__.build()")
    now = isa.fingerprint_of_built_library()
    before = isa.record("r11g11b10f_in_place_fingerprint_before.json")
    assert not sorted(k for k in before if now.get(k) != before[k])   # no kernel of the parent build moved or left
    added = sorted(set(now) - set(before))
    assert len(added) == 42, added
    pat = re.compile(r"^void ovrfsr_fast::(easu_fast_kernel<6, [012], (28|32|40), (true|false)>|fused_kernel<6, [12], [012], (32|40), 256>|"
                     r"easu_outside_kernel<6, [012], (-1|[012])>)\(")
    assert all(pat.match(k) for k in added), [k for k in added if not pat.match(k)]
    for name in ("isa_fingerprint.json", "r06_isa_fingerprint_r06.json", "rcas_one_quotient_fingerprint_before.json",
                 "exact_stores_fingerprint_before.json", "reference_formats_fingerprint_before.json"):
        rec = isa.record(name)
        assert not [k for k in added if rec.get(k) != now[k]], name


# ---- 5. the measurement build ------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("unit", ["postprocessor.cpp", "pipeline_plan.cpp"])
def test_pass_macro_compiles(unit):
    """-DOVRFSR_PACKED_RESOLVE_PASS (measurement build: the resolve pass where the kernels would decode in staging) still type-checks."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not installed")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", "-Wno-unused-function", "-ffp-contract=on", "-x", "hip",
           "-DOVRFSR_PACKED_RESOLVE_PASS", "-fsyntax-only", unit]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_pass_macro_keeps_the_pass(probe):  # noqa: F811
    """... and is listed where the other measurement builds are; the planner built with it answers 0 for the packed format"""
    assert "OVRFSR_PACKED_RESOLVE_PASS" in open(os.path.join(CSRC, "Makefile")).read()
    import shutil
    cxx = shutil.which("g++") or shutil.which("clang++")
    exe = os.path.join(probe.tmp, "plan_probe_pass")
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-DOVRFSR_PACKED_RESOLVE_PASS", os.path.join(ROOT, "tests", "debug", "plan_probe.cpp"),
                    os.path.join(CSRC, "pipeline_plan.cpp"), os.path.join(CSRC, "constants.cpp"), os.path.join(CSRC, "nis_config.cpp"), "-o", exe], check=True)
    path = os.path.join(probe.tmp, "pass_cases.txt")
    lines = [PLAN_CASES[0][1], PLAN_CASES[1][1], [line for n, line, _ in FORM_TABLE if n == "MS4 RGBA8 unmasked"][0]]
    open(path, "w").write("\n".join(lines) + "\n")
    import json
    out = [json.loads(x) for x in subprocess.run([exe, path], capture_output=True, text=True, check=True, timeout=120).stdout.splitlines()]
    assert [g["resolve_in_staging"] for g in out] == [0, 0, 1], out
