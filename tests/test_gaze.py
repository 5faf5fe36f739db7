"""Eye-tracked foveation without a GPU (header, "Eye-tracked foveation"): the four symbols and their NULL-ctx answers; the planner's re-aim step
(csrc/pipeline_plan.cpp, reaim_pipeline) through tests/debug/gaze_probe.cpp -- compiled on the fly with the planner units under AddressSanitizer
and UBSan and run as a child process, like plan_probe -- against plan_pipeline on the effective configuration; and the machine code: nothing of
the parent build moved, the kernels added are tile_records_kernel's, and they are the small copy-class kernels they should be."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from tests import isa
from tests.test_kernel_resources import kernels  # noqa: F401  (fixture: the code objects' metadata notes)
from tests.test_pipeline_plan import FORM_TABLE, _largest_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openvr_fsr_amd", "csrc")
SYMBOLS = ("ovrfsr_set_gaze", "ovrfsr_clear_gaze", "ovrfsr_get_gaze", "ovrfsr_gaze_stats")

# input -> output, the hidden-area test's shapes (S1 S2 S3)
SHAPES = {"S1": (80, 64, 160, 128), "S2": (150, 110, 200, 147), "S3": (240, 200, 320, 267)}
NAMED = [(0.5, 0.5), (0.2, 0.3), (0.8, 0.7), (0.0, 0.0), (1.0, 1.0), (0.37, 0.61)]   # G; the probe's seventh is OUT = (2, 2)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def _lib():
    import openvr_fsr_amd as A
    if not A.have_library():
        pytest.fail("libopenvr_fsr_amd.so is not built: run __graft_entry__.build()")
    return A.library()


def test_the_library_exports_the_four_symbols():
    L = _lib()
    assert [s for s in SYMBOLS if not hasattr(L, s)] == []


def test_null_ctx_is_an_invalid_argument():
    L = _lib()
    xy, flag, a, b = (C.c_float * 2)(), C.c_int(), C.c_uint32(), C.c_uint32()
    assert L.ovrfsr_set_gaze(None, 0, 0.5, 0.5) == 1
    assert L.ovrfsr_clear_gaze(None, 0) == 1
    assert L.ovrfsr_get_gaze(None, 0, xy, C.byref(flag)) == 1
    assert L.ovrfsr_gaze_stats(None, C.byref(a), C.byref(b)) == 1


# ---- the probe ---------------------------------------------------------------------------------------------------------------------------
def build_gaze_probe():
    """-> (run(mode, lines) -> parsed JSON lines, tmp dir); the caller removes the directory"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    tmp = tempfile.mkdtemp(prefix="ovrfsr_gaze_probe_")
    exe = os.path.join(tmp, "gaze_probe")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static + [
                    os.path.join(ROOT, "tests", "debug", "gaze_probe.cpp"), os.path.join(CSRC, "pipeline_plan.cpp"),
                    os.path.join(CSRC, "constants.cpp"), os.path.join(CSRC, "nis_config.cpp"), "-o", exe], check=True)

    def run(mode, lines):
        path = os.path.join(tmp, "cases.txt")
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        r = subprocess.run([exe, mode, path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
        out = [json.loads(x) for x in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out

    return run, tmp


@pytest.fixture(scope="module")
def probe():
    run, tmp = build_gaze_probe()
    yield run
    shutil.rmtree(tmp, ignore_errors=True)


def reshaped(line, cid, shape):
    """a case line of the planner test at another shape (fields: id fmt w h ... out_width out_height at 16, 17)"""
    f = line.split(" ")
    iw, ih, ow, oh = shape
    f[0], f[2], f[3], f[16], f[17] = cid, str(iw), str(ih), str(ow), str(oh)
    return " ".join(f)


def masked_form_lines():
    """every form of the planner test's table that has a mask (radius < 2), at the three shapes"""
    lines = []
    for i, (name, line, want) in enumerate(FORM_TABLE):
        if float(line.split(" ")[11]) < 2.0 and want.get("status", 0) == 0:
            for sn, shape in SHAPES.items():
                lines.append(reshaped(line, "form%d/%s" % (i, sn), shape) + " 1")
    return lines


@pytest.fixture(scope="module")
def sweep(probe):
    lines = masked_form_lines()
    return lines, probe("sweep", lines)


def test_reaim_agrees_with_the_planner(sweep):
    """from three previous gazes to each gaze of the 9x9 grid and the named ones: "rebuild" exactly where plan_pipeline on the effective
    configuration differs in a field no re-aim may move, "nothing" exactly where the centres are equal, else the same plan but for the
    list offsets -- lists, records and spans equal in content and count, inside their regions"""
    lines, got = sweep
    assert len(lines) >= 3 * 15
    planned = [g for g in got if not g["refused"]]
    assert len(planned) >= 0.8 * len(got), [g["id"] for g in got if g["refused"]]   # (a form may refuse a shape; not most of them)
    for g in planned:
        assert g["errors"] == [], g
        if g["tile_lists"]:   # (the strict build has a mask and no lists: centres and modes are all a re-aim moves there)
            assert g["inplace"] > 100 and g["rebuild"] > 10 and g["nothing"] >= 3, g


def test_largest_output_reaims_inside_its_regions(probe):
    """12288^2 -> 16384^2, 512 x 512 tiles per eye: the named gazes from the three previous ones"""
    (g,) = probe("sweep", [_largest_lines()[0] + " 0"])
    assert not g["refused"] and g["errors"] == [] and g["inplace"] >= 20, g


def test_the_named_gazes_cover_what_the_gpu_test_needs(sweep):
    """at each shape and tile size the six G gazes give six pairwise different non-empty inside lists, and OUT an empty one: a re-aim between
    any two of them changes what is launched"""
    lines, got = sweep
    seen = set()
    for line, g in zip(lines, got):
        if g["refused"] or not g["tile_lists"] or float(line.split(" ")[11]) != 0.5:   # (the GPU test's radius)
            continue
        lists = [tuple(x) for x in g["named_inside"]]
        assert all(lists[:6]) and len(set(lists[:6])) == 6 and lists[6] == (), g["id"]
        seen.add((g["id"].split("/")[1], tuple(g["tile"])))
        if g["id"].endswith("/S1") and g["tile"] == [32, 32]:
            assert [len(x) for x in lists] == [6, 4, 4, 1, 1, 6, 0], g
    assert {s for s, _ in seen} == set(SHAPES) and {t for _, t in seen} == {(32, 32), (32, 24)}, seen


def test_sequence_mode_walks_the_launch_managers_steps(probe):
    """first build, a re-aim, a sub-pixel no-op, both eyes out (no mask: rebuild), back (rebuild), cleared onto the same centre (nothing)"""
    line = reshaped(FORM_TABLE[1][1], "seq", SHAPES["S1"])
    steps = [(1, 0.5, 0.5, 1, 0.5, 0.5), (1, 0.2, 0.3, 1, 0.8, 0.7), (1, 0.2001, 0.3, 1, 0.8, 0.7), (1, 2, 2, 1, 2, 2), (1, 0.5, 0.5, 1, 0.5, 0.5),
             (0, 0, 0, 0, 0, 0)]
    (g,) = probe("sequence", [line + " %d " % len(steps) + " ".join(" ".join(repr(float(v)) if i % 3 else str(v) for i, v in enumerate(s)) for s in steps)])
    assert g["steps"] == ["first", "reaim", "nothing", "rebuild", "rebuild", "nothing"], g


# ---- machine code ------------------------------------------------------------------------------------------------------------------------
NEW = re.compile(r"^void ovrfsr_fast::tile_records_kernel<(32|24)>\(")


def test_fingerprint_scope():
    if not os.path.exists(isa.LIB):
        pytest.fail("libopenvr_fsr_amd.so is not built: run __graft_entry__.build()")
    now = isa.fingerprint_of_built_library()
    before = isa.record("gaze_fingerprint_before.json")
    assert not sorted(k for k in before if now.get(k) != before[k])   # no kernel of the parent build moved or left
    added = sorted(set(now) - set(before))
    assert len(added) == 2 and all(NEW.match(k) for k in added), added
    # the records the earlier fingerprint tests read carry the new kernels with the built values
    for name in ("isa_fingerprint.json", "r06_isa_fingerprint_r06.json", "rcas_one_quotient_fingerprint_before.json", "exact_stores_fingerprint_before.json",
                 "reference_formats_fingerprint_before.json", "r11g11b10f_in_place_fingerprint_before.json", "hdr_domain_fingerprint_before.json"):
        rec = isa.record(name)
        assert not [k for k in added if rec.get(k) != now[k]], name


def test_code_object_notes(kernels):  # noqa: F811
    new = {k: v for k, v in kernels.items() if "tile_records_kernel" in k}
    assert len(new) == 2 and all("ovrfsr_fast" in k for k in new), sorted(new)   # the 32-row and the 24-row caps; no strict-namespace copy
    for k, v in new.items():
        assert not (v["vgpr_spill_count"] or v["sgpr_spill_count"] or v["private_segment_fixed_size"]), (k, v)   # no spill, no scratch
        assert v["group_segment_fixed_size"] == 0 and v["agpr_count"] == 0, (k, v)                              # no LDS, no AGPR
        assert v["max_flat_workgroup_size"] == 256, (k, v)
        assert v["vgpr_count"] <= 32, (k, v)


def test_the_kernel_is_plain_cpp_with_one_record_rule():
    """no inline assembly, no LDS; memory through the accessors of fsr_bounds.h; and the record rule has one definition, which the planner's
    outside_records calls too"""
    text = open(os.path.join(CSRC, "fsr_tile_records.inc")).read() + open(os.path.join(CSRC, "tile_records.h")).read()
    code = re.sub(r"//.*", "", text)
    assert not re.search(r"\basm\b|__asm|__shared__", code)
    assert code.count("OVRFSR_PLANE(") == 4 and "OVRFSR_AT(uint4" in code
    assert not re.search(r"\*\s*reinterpret_cast", code)
    planner = re.sub(r"//.*", "", open(os.path.join(CSRC, "pipeline_plan.cpp")).read())
    assert "tile_record(" in planner and "tile_record(" in code and "colsN | " not in planner
