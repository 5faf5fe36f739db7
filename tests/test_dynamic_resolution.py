"""Dynamic resolution without a GPU (header, "dynamic resolution"): the three symbols and their NULL-ctx answers; the planner's re-scale step
(csrc/pipeline_plan.cpp, rescale_pipeline) through tests/debug/rescale_probe.cpp -- compiled on the fly with the planner units under
AddressSanitizer and UBSan and run as a child process, like plan_probe -- against plan_pipeline at every size; the tap rule's host side
(csrc/bilin_taps.h) against the tables the planner built before the rule moved there; and the machine code: nothing of the parent build
moved, the kernel added is tap_tables_kernel, and it is the small store-only kernel it should be."""
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
from tests.test_pipeline_plan import FORM_TABLE, RGBA8, RGBA16F, R11G11B10F, _line, parent_digests

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openvr_fsr_amd", "csrc")
SYMBOLS = ("ovrfsr_set_max_input_size", "ovrfsr_get_max_input_size", "ovrfsr_rescale_stats")

MASK, UNMASKED = dict(radius=0.5, proj_centre=(0.2, 0.3, 0.8, 0.7)), dict(radius=2.0)
# output, ladder of input sizes (tests/test_gpu_dynamic_resolution.py walks the same)
LADDER_A = ((160, 128), [(80, 64), (120, 96), (107, 86), (152, 120), (64, 52), (100, 64), (160, 100), (80, 64)])
LADDER_B = ((200, 147), [(150, 110), (100, 74), (134, 98)])
LADDER_W = ((160, 128), [(80, 64), (200, 160), (80, 64)])


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def _lib():
    import openvr_fsr_amd as A
    if not A.have_library():
        pytest.fail("libopenvr_fsr_amd.so is not built: run __graft_entry__.build()")
    return A.library()


def test_the_library_exports_the_three_symbols():
    L = _lib()
    assert [s for s in SYMBOLS if not hasattr(L, s)] == []


def test_null_ctx_is_an_invalid_argument():
    L = _lib()
    a, b = C.c_uint32(), C.c_uint32()
    assert L.ovrfsr_set_max_input_size(None, 160, 120) == 1
    assert L.ovrfsr_set_max_input_size(None, 0, 0) == 1
    assert L.ovrfsr_get_max_input_size(None, C.byref(a), C.byref(b)) == 1
    assert L.ovrfsr_rescale_stats(None, C.byref(a), C.byref(b)) == 1


# ---- the probe -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe():
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    tmp = tempfile.mkdtemp(prefix="ovrfsr_rescale_probe_")
    exe = os.path.join(tmp, "rescale_probe")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static + [
                    os.path.join(ROOT, "tests", "debug", "rescale_probe.cpp"), os.path.join(CSRC, "pipeline_plan.cpp"),
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

    yield run
    shutil.rmtree(tmp, ignore_errors=True)


def walk_line(cid, fmt, ladder, hdr=0, one_eye=1, dest=-1, **cfg):
    (ow, oh), sizes = ladder
    cfg.setdefault("out_width", ow)
    cfg.setdefault("out_height", oh)
    return _line(cid, fmt, sizes[0][0], sizes[0][1], one_eye, dest, fsr_enabled=1, **cfg) + " %d %d " % (hdr, len(sizes) - 1) + \
        " ".join("%d %d" % s for s in sizes[1:])


def reladdered(line, cid, ladder):
    """a case line of the planner test walking a ladder (fields: id fmt w h ... out_width out_height at 16, 17)"""
    (ow, oh), sizes = ladder
    f = line.split(" ")
    f[0], f[2], f[3], f[16], f[17] = cid, str(sizes[0][0]), str(sizes[0][1]), str(ow), str(oh)
    return " ".join(f) + " 0 %d " % (len(sizes) - 1) + " ".join("%d %d" % s for s in sizes[1:])


def test_the_step_agrees_with_the_planner(probe):
    """every product form of the planner test's table and the strict build, walking the three ladders: whatever the step answers "in place"
    for equals plan_pipeline at that size in every field and table (taps, lists, records, spans: plan_serial), and after the walk the plan
    is the fresh plan of the last size, whatever mixture of re-scales and rebuilds led there"""
    lines = []
    for i, (name, line, want) in enumerate(FORM_TABLE):
        if want.get("status", 0) == 0 and want.get("upscale", 1):
            for ln, ladder in (("A", LADDER_A), ("B", LADDER_B), ("W", LADDER_W)):
                lines.append(reladdered(line, "form%d/%s" % (i, ln), ladder))
    lines.append(walk_line("strict/A", RGBA8, LADDER_A, precision=2, **MASK))
    lines.append(walk_line("srtm/A", RGBA16F, LADDER_A, hdr=1, **MASK))
    got = probe("walk", lines)
    assert len(got) >= 3 * 25
    inplace = 0
    for g in got:
        assert g["first"] == 0, g["id"]
        for s in g["steps"]:
            assert s["answer"] != "inplace" or s["equal"] == 1, (g["id"], s)
            assert s["answer"] != "nothing", (g["id"], s)                      # (consecutive sizes of the ladders differ)
            inplace += s["answer"] == "inplace"
        assert g["final_equal"] == 1 or not g["alive"], g["id"]
        assert g["alive"] or g["steps"][-1]["status"] != 0, g["id"]           # (a walk ends early only in a refusal)
    assert inplace >= 150, inplace


def test_the_ladders_of_the_gpu_test_rescale_in_place(probe):
    """the condition the step exists for: fused = -1, masked and unmasked, RGBA8 and RGBA16F, ladders A and B -- every step is answered in
    place (none of them crosses input = output), and the form and flags do not move between the listed sizes"""
    lines = [walk_line("%s/%d/%s" % (ln, fmt, mn), fmt, ladder, **m)
             for ln, ladder in (("A", LADDER_A), ("B", LADDER_B)) for fmt in (RGBA8, RGBA16F) for mn, m in (("masked", MASK), ("unmasked", UNMASKED))]
    for g in probe("walk", lines):
        assert g["first"] == 0 and g["alive"] == 1 and g["final_equal"] == 1, g["id"]
        assert len(g["steps"]) in (7, 2), g["id"]
        for s in g["steps"]:
            assert s["answer"] == "inplace" and s["equal"] == 1 and s["form"] == g["form"], (g["id"], s)
            assert s["fused_cells"][0] <= 40, (g["id"], s)
    # W: the 200 x 160 input's footprint is wider than 40 cells.  Unmasked (two-pass) that is a re-scale across which an R11G11B10F
    # submission's decode moves from the kernels' staging to the unpack pass and back; masked, the half pipeline leaves the fused form: a rebuild
    unmasked, masked = probe("walk", [walk_line("W/unmasked", R11G11B10F, LADDER_W, **UNMASKED), walk_line("W/masked", R11G11B10F, LADDER_W, **MASK)])
    assert [(s["answer"], s["resolve_in_staging"]) for s in unmasked["steps"]] == [("inplace", 0), ("inplace", 1)] and unmasked["steps"][0]["cells"][0] > 40
    assert [s["answer"] for s in masked["steps"]] == ["rebuild", "rebuild"] and masked["final_equal"] == 1
    assert masked["steps"][0]["form"] == "two-pass" and masked["form"] == "fused with masked outside tiles"


def test_the_classification(probe):
    follows = walk_line("output-follows", RGBA8, ((0, 0), [(80, 64), (120, 96)]), render_scale=0.75, **MASK)
    equal = walk_line("input-equals-output", RGBA8, ((160, 128), [(80, 64), (160, 128), (80, 64)]), **MASK)
    nis = walk_line("nis-too-steep", RGBA8, ((160, 128), [(80, 64), (64, 52)]), use_nis=1, **MASK)
    same = walk_line("same-size", RGBA8, ((160, 128), [(80, 64), (80, 64), (120, 96), (120, 96)]), **MASK)
    f, e, n, s = probe("walk", [follows, equal, nis, same])
    assert [x["answer"] for x in f["steps"]] == ["rebuild"] and f["steps"][0]["out"] == [160, 128] and f["final_equal"] == 1
    # (no upscale stage at 160 x 128: doUpscale flips, and flips back)
    assert [(x["answer"], x["upscale"]) for x in e["steps"]] == [("rebuild", 0), ("rebuild", 1)] and e["final_equal"] == 1
    # the fresh plan's refusal: the rebuild fails as a fresh ctx does
    assert [(x["answer"], x["status"], x["text"]) for x in n["steps"]] == [("rebuild", 2, "NIS scales 1x..2x only (NVScalerUpdateConfig returned false)")]
    assert n["alive"] == 0
    assert [x["answer"] for x in s["steps"]] == ["nothing", "inplace", "nothing"]


def test_without_a_maximum_every_plan_has_its_parent_digest(probe):
    """the plan made without a maximum is the recorded one (tests/golden/plan_digests_parent.json), next to the rescale-capable plan of the
    same line, which differs from it in the layout of its lists only"""
    lines = [line + " 0 0 " for _, line, want in FORM_TABLE if want.get("status", 0) == 0]
    record = parent_digests("plan_probe")
    got = probe("walk", lines)
    assert len(got) >= 30
    for g in got:
        assert g["plain_digest"] == record[g["id"]], g["id"]
        assert g["first"] == 0 and g["capable_equals_plain"] == 1, g["id"]


def test_the_tap_headers_host_side_builds_the_parents_tables(probe):
    """bilin_taps.h against tap_tables as it was before the rule moved into the header: 200 (input, output) pairs, the table digests recorded
    from the parent commit's planner (tests/golden/tap_tables_parent.json)"""
    with open(os.path.join(ROOT, "tests", "golden", "tap_tables_parent.json")) as f:
        pairs = json.load(f)["pairs"]
    assert len(pairs) == 200
    got = probe("taps", ["%d %d %d %d" % tuple(p["in"] + p["out"]) for p in pairs])
    assert got == pairs


# ---- machine code ----------------------------------------------------------------------------------------------------------------------
NEW = re.compile(r"^void ovrfsr_fast::tap_tables_kernel<256>\(")


def test_fingerprint_scope():
    if not os.path.exists(isa.LIB):
        pytest.fail("libopenvr_fsr_amd.so is not built: run __graft_entry__.build()")
    now = isa.fingerprint_of_built_library()
    before = isa.record("dynamic_resolution_fingerprint_before.json")
    assert not sorted(k for k in before if now.get(k) != before[k])   # no kernel of the parent build moved or left
    added = sorted(set(now) - set(before))
    assert len(added) == 1 and NEW.match(added[0]), added
    # the records the earlier fingerprint tests read carry the new kernel with the built value
    for name in ("isa_fingerprint.json", "r06_isa_fingerprint_r06.json", "rcas_one_quotient_fingerprint_before.json", "exact_stores_fingerprint_before.json",
                 "reference_formats_fingerprint_before.json", "r11g11b10f_in_place_fingerprint_before.json", "hdr_domain_fingerprint_before.json",
                 "gaze_fingerprint_before.json"):
        assert isa.record(name).get(added[0]) == now[added[0]], name
    # and none of the patterns older tests count kernels by
    assert not re.search(r"hdr_(forward|back)_kernel|_kernelILi6E|tile_records_kernel", added[0])


def test_code_object_notes(kernels):  # noqa: F811
    new = {k: v for k, v in kernels.items() if "tap_tables_kernel" in k}
    assert len(new) == 1 and all("ovrfsr_fast" in k for k in new), sorted(new)
    for k, v in new.items():
        assert not (v["vgpr_spill_count"] or v["sgpr_spill_count"] or v["private_segment_fixed_size"]), (k, v)   # no spill, no scratch
        assert v["group_segment_fixed_size"] == 0 and v["agpr_count"] == 0, (k, v)                              # no LDS, no AGPR
        assert v["max_flat_workgroup_size"] == 256, (k, v)
        assert v["vgpr_count"] <= 32, (k, v)


def test_the_kernel_is_plain_cpp_with_one_tap_rule():
    """no inline assembly, no LDS; memory through the accessors of fsr_bounds.h; and the tap rule has one definition, which the planner's
    tap_tables calls too"""
    text = open(os.path.join(CSRC, "fsr_tap_tables.inc")).read() + open(os.path.join(CSRC, "bilin_taps.h")).read()
    code = re.sub(r"//.*", "", text)
    assert not re.search(r"\basm\b|__asm|__shared__", code)
    assert code.count("OVRFSR_PLANE(") == 2 and code.count("OVRFSR_AT(uint2") == 2
    assert not re.search(r"\*\s*reinterpret_cast", code)
    planner = re.sub(r"//.*", "", open(os.path.join(CSRC, "pipeline_plan.cpp")).read())
    assert "bilin_tap(" in planner and "bilin_tap(" in code and "256.0f" not in planner
