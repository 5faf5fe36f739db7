"""The pipeline planner (csrc/pipeline_plan.cpp) without a GPU: tests/debug/plan_probe.cpp is compiled on the fly with the planner unit and the
two host constant units (constants.cpp, nis_config.cpp) -- nothing from the kernel units, no HIP -- under AddressSanitizer and UBSan, and run
as a child process.  Checked: (a) a hand-written table of the forms of configurations the project names elsewhere, (b) every refusal the planner
can produce is reached by the launch-form matrix (tools/debug/record_forms.py), (c) structural invariants of the tile, span, record and tap
tables at shapes from 1x1 to 16384^2, (d) status, text and owned format agree, case by case, with what the library at the commit before
the planner did on an MI355X (tests/golden/launch_forms_parent.json), (e) every plan of (a)-(c), serialised by value (tests/debug/plan_serial.h),
has the digest it had before the tile lists were built in steps (tests/golden/plan_digests_parent.json)."""
import functools
import importlib.util
import json
import os
import shutil
import subprocess
import tempfile

import pytest

from tests import isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openvr_fsr_amd", "csrc")

RGBA8, RGBA16F, RGBA32F, RGB10A2, BGRA8, R11G11B10F = 0, 1, 2, 3, 4, 6
MS4_RGBA8 = RGBA8 | 4 << 8
DEFAULTS = dict(fsr_enabled=0, use_nis=0, debug_mode=0, render_scale=1.0, sharpness=0.75, radius=0.5, proj_centre=(0.5, 0.5, 0.5, 0.5),
                out_width=0, out_height=0, precision=0, quantize_intermediate=1, fused=-1, stage_mask=0, pair_submit=0, reference_formats=0)


@functools.lru_cache(maxsize=None)
def _matrix():
    spec = importlib.util.spec_from_file_location("record_forms", os.path.join(ROOT, "tools", "debug", "record_forms.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def probe():
    """the probe, built under the host sanitizers; -> run(argument) -> stdout lines"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    tmp = tempfile.mkdtemp(prefix="ovrfsr_plan_probe_")
    exe = os.path.join(tmp, "plan_probe")
    # (g++ links the sanitizer runtimes dynamically unless told otherwise; linked statically, the probe needs nothing of its environment)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static + [
                    os.path.join(ROOT, "tests", "debug", "plan_probe.cpp"), os.path.join(CSRC, "pipeline_plan.cpp"),
                    os.path.join(CSRC, "constants.cpp"), os.path.join(CSRC, "nis_config.cpp"), "-o", exe], check=True)

    def run(arg):
        r = subprocess.run([exe, arg], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-4000:]
        return r.stdout.splitlines()

    run.tmp = tmp
    yield run
    shutil.rmtree(tmp, ignore_errors=True)


def _line(cid, fmt, w, h, one_eye, dest, **cfg):
    c = dict(DEFAULTS)
    c.update(cfg)
    pc = c.pop("proj_centre")
    vals = [cid.replace(" ", "_"), fmt, w, h, int(one_eye), dest, c["fsr_enabled"], c["use_nis"], c["debug_mode"], repr(float(c["render_scale"])),
            repr(float(c["sharpness"])), repr(float(c["radius"]))] + [repr(float(x)) for x in pc] + \
           [c["out_width"], c["out_height"], c["precision"], c["quantize_intermediate"], c["fused"], c["stage_mask"], c["pair_submit"], c["reference_formats"]]
    return " ".join(str(v) for v in vals)


def _plan(probe, lines):
    path = os.path.join(probe.tmp, "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    out = [json.loads(x) for x in probe(path)]
    assert len(out) == len(lines)
    return out


@functools.lru_cache(maxsize=None)
def parent_digests(probe_name):
    """id -> digest of the plan at the recorded parent commit, for the lines one probe plans"""
    with open(os.path.join(ROOT, "tests", "golden", "plan_digests_parent.json")) as f:
        return json.load(f)[probe_name]


def assert_parent_digests(probe_name, plans):
    """every planned line has its recorded digest -- an id without a record fails -- and a refused line has none"""
    record = parent_digests(probe_name)
    ids = [p["id"] for p in plans]
    assert len(set(ids)) == len(ids), sorted(i for i in set(ids) if ids.count(i) > 1)
    for p in plans:
        if p["status"] == 0:
            assert p["id"] in record, p["id"]
            assert p["digest"] == record[p["id"]], p["id"]
        else:
            assert p["id"] not in record, p["id"]


def _plan_checked(probe, lines):
    plans = _plan(probe, lines)
    assert_parent_digests("plan_probe", plans)
    return plans


# ---- (a) the forms of configurations the project names --------------------------------------------------------------------------
def _named(name, fmt, shape, want, dest=-1, **cfg):
    iw, ih, ow, oh = shape
    return (name, _line(name, fmt, iw, ih, 1, dest, fsr_enabled=1, out_width=ow, out_height=oh, **cfg), want)


CAMPAIGN, BACK_TO_BACK, MATRIX = (150, 110, 200, 147), (960, 810, 1280, 1080), (80, 64, 160, 128)
M = dict(radius=0.5, proj_centre=(0.2, 0.3, 0.8, 0.7))   # the matrix's mask
FORM_TABLE = [
    # the eleven configurations of tools/debug/fault_campaign.py, by the names it gives them
    _named("two-pass RGBA8, unmasked", RGBA8, CAMPAIGN, dict(form="two-pass", tile_lists=0), radius=2.0, sharpness=0.9),
    _named("mask-sorted RGBA8 (tile lists, tap tables)", RGBA8, CAMPAIGN, dict(form="mask-sorted", tile_lists=1, overlap=0), radius=0.5, sharpness=0.9),
    _named("two-pass RGBA8, masked, plain (fused=0)", RGBA8, CAMPAIGN, dict(form="two-pass", tile_lists=1, overlap=0), radius=0.5, fused=0, sharpness=0.9),
    _named("fused half, masked (auxiliary stream)", RGBA16F, CAMPAIGN, dict(form="fused with masked outside tiles", tile_lists=1, overlap=1), radius=0.5, sharpness=0.9),
    _named("fused on request", RGBA8, CAMPAIGN, dict(form="fused", tile_lists=0), radius=2.0, fused=1, sharpness=0.9),
    _named("EASU only", RGBA8, CAMPAIGN, dict(form="upscale only", tile_lists=0, sharpen=0), radius=2.0, stage_mask=1, sharpness=0.9),
    _named("NVScaler, masked", RGBA8, CAMPAIGN, dict(form="upscale only", tile_lists=1, overlap=0), radius=0.5, use_nis=1, sharpness=0.9),
    _named("NVScaler half, masked (auxiliary stream)", RGBA16F, CAMPAIGN, dict(form="upscale only", tile_lists=1, overlap=1), radius=0.5, use_nis=1, sharpness=0.9),
    _named("BGRA8 submission (swizzle buffer)", BGRA8, CAMPAIGN, dict(form="two-pass", pipeline=RGBA8, owned=RGBA8), radius=2.0, sharpness=0.9),
    _named("debug mode (timestamp events)", RGBA8, CAMPAIGN, dict(form="mask-sorted"), radius=0.5, debug_mode=1, sharpness=0.9),
    _named("pair_submit, masked", RGBA8, CAMPAIGN, dict(form="mask-sorted"), radius=0.5, pair_submit=1, sharpness=0.9),
    # tests/test_gpu_back_to_back.py's forms as tests/README.md lists them (960x810 -> 1280x1080)
    _named("b2b unmasked two-pass", RGBA8, BACK_TO_BACK, dict(form="two-pass", tile_lists=0), radius=2.0, sharpness=0.9),
    _named("b2b sorted two-pass", RGBA8, BACK_TO_BACK, dict(form="mask-sorted", overlap=0), radius=0.5, sharpness=0.9, debug_mode=1),
    _named("b2b fused + outside (RGBA16F)", RGBA16F, BACK_TO_BACK, dict(form="fused with masked outside tiles", overlap=1), radius=0.5, sharpness=0.9),
    _named("b2b fused on request", RGBA8, BACK_TO_BACK, dict(form="fused with masked outside tiles", overlap=0), radius=0.6, sharpness=0.7, fused=1),
    _named("b2b NVScaler + DirectCopy", RGBA8, BACK_TO_BACK, dict(form="upscale only", tile_lists=1, overlap=0), radius=0.5, sharpness=0.9, use_nis=1),
    _named("b2b EASU only", RGBA8, BACK_TO_BACK, dict(form="upscale only", tile_lists=1, overlap=0), radius=0.4, stage_mask=1),
    _named("b2b EASU only, RGBA16F (forked)", RGBA16F, BACK_TO_BACK, dict(form="upscale only", tile_lists=1, overlap=1), radius=0.3, stage_mask=1),
    _named("b2b NVScaler + DirectCopy, RGBA16F (forked)", RGBA16F, BACK_TO_BACK, dict(form="upscale only", tile_lists=1, overlap=1), radius=0.4, use_nis=1, sharpness=0.6),
    # 4x RGBA8: resolved in staging when unmasked, through the resolve pass when masked (and whenever EASU does not store UNORM8)
    _named("MS4 RGBA8 unmasked", MS4_RGBA8, MATRIX, dict(form="two-pass", resolve_in_staging=1, pipeline=RGBA8), radius=2.0),
    _named("MS4 RGBA8 masked", MS4_RGBA8, MATRIX, dict(form="mask-sorted", resolve_in_staging=0), **M),
    _named("MS4 RGBA8 unmasked, EASU only into float", MS4_RGBA8, MATRIX, dict(form="upscale only", resolve_in_staging=0), dest=RGBA32F, radius=2.0, stage_mask=1),
    _named("MS4 RGBA8 unmasked, strict", MS4_RGBA8, MATRIX, dict(form="two-pass", resolve_in_staging=0), radius=2.0, precision=2),
    # a float source under reference_formats: UNORM8 intermediate and output, mask-sorted where there is a mask, in order on the caller's stream
    _named("RGBA16F reference_formats masked", RGBA16F, MATRIX, dict(form="mask-sorted", mid=RGBA8, owned=RGBA8, overlap=0, unorm8_guard=1), reference_formats=1, **M),
    _named("R11G11B10F reference_formats masked", R11G11B10F, MATRIX, dict(form="mask-sorted", pipeline=RGBA16F, mid=RGBA8, owned=RGBA8), reference_formats=1, **M),
    _named("RGBA16F reference_formats unmasked", RGBA16F, MATRIX, dict(form="two-pass", mid=RGBA8, owned=RGBA8), reference_formats=1, radius=2.0),
    _named("RGBA16F own formats masked", RGBA16F, MATRIX, dict(form="fused with masked outside tiles", mid=RGBA16F, owned=RGBA16F, unorm8_guard=0), **M),
    # FP32_EXACT: the two-pass and mask-sorted forms only (and the stages on their own)
    _named("FP32_EXACT unmasked", RGBA8, MATRIX, dict(form="two-pass"), precision=3, radius=2.0),
    _named("FP32_EXACT masked", RGBA8, MATRIX, dict(form="mask-sorted"), precision=3, **M),
    _named("FP32_EXACT masked, fused = 0", RGBA8, MATRIX, dict(form="two-pass", tile_lists=1), precision=3, fused=0, **M),
    _named("FP32_EXACT fused = 1", RGBA8, MATRIX, dict(status=2, text="precision FP32_EXACT: the fused kernel has no exact-stores form (fused = 1)"), precision=3, fused=1, **M),
    _named("FP32_EXACT half source", RGBA16F, MATRIX, dict(status=2), precision=3, **M),
    # the two remaining names of the enum
    _named("sharpen only", RGBA8, (96, 80, 96, 80), dict(form="sharpen only", upscale=0, sharpen=1), stage_mask=2),
    _named("EASU only at scale 1: nothing to do", RGBA8, (96, 80, 96, 80), dict(form="none", upscale=0, sharpen=0), stage_mask=1),
]


def _form_lines():
    return [line for _, line, _ in FORM_TABLE]


def test_form_table(probe):
    got = _plan_checked(probe, _form_lines())
    for (name, _, want), g in zip(FORM_TABLE, got):
        want = dict(want)
        want.setdefault("status", 0)
        for k, v in want.items():
            assert g.get(k) == v, (name, k, v, g)


# ---- the launch-form matrix through the planner ----------------------------------------------------------------------------------
DEST = {"owned": -1, "rgba8": RGBA8, "rgba16f": RGBA16F, "rgba32f": RGBA32F, "rgb10a2": RGB10A2, "bgra8": BGRA8}


def _matrix_lines():
    R = _matrix()
    cases = R.cases()
    lines = []
    for c in cases:
        iw, ih, _, _ = c["shape"]
        cfg = dict(c["cfg"], pair_submit=1 if c["kind"] == "pair" else 0)
        lines.append(_line(c["id"], R.SOURCES[c["src"]], iw, ih, c["kind"] != "shared", DEST[c["dst"]], **cfg))
    return cases, lines


@pytest.fixture(scope="module")
def matrix_plans(probe):
    cases, lines = _matrix_lines()
    return cases, _plan_checked(probe, lines)


# every refusal of the planner's table, in its order.  The two marked unreachable are defensive: the matrix cannot produce them, because no
# configuration can --
#   "NIS tile does not fit LDS": NVScalerUpdateConfig accepts 1x..2x upscaling only, so kScale <= 1 and a 32x24 group's footprint is at
#     most 32 + 7 = 39 cells wide (nis_pitch 40) and 24 + 7 rows high: 40 * 31 * 28 + 4096 bytes < 64 KiB;
#   "... the fused kernel has no exact-stores form": under FP32_EXACT fused = 1 is refused earlier by name, and fused = -1 picks the fused
#     kernel for half / float intermediates only, which "RCAS must read RGBA8" has refused by then.
REFUSALS = [
    (1, "output size is zero or beyond 16384 texels (render_scale must be finite and > 0)"),
    (1, "bad stage_mask"),
    (1, "sharpen-only needs output size == input size"),
    (1, "unknown precision"),
    (2, "precision FP32_EXACT: NIS has no exact-stores form (use_nis)"),
    (2, "precision FP32_EXACT: the fused kernel has no exact-stores form (fused = 1)"),
    (2, "precision FP32_EXACT: RCAS must read a UNORM8 intermediate (quantize_intermediate = 0)"),
    (2, "precision FP32_EXACT: RCAS must read RGBA8 (a half, float or 10-bit intermediate or input promises no exact bytes)"),
    (2, "NIS scales 1x..2x only (NVScalerUpdateConfig returned false)"),
    (2, "NIS tile does not fit LDS"),
    (2, "scale ratio needs more LDS than one tile may use"),
    (2, "the fused kernel is not built for RGB10A2 images"),
    (2, "the fused kernel is not built for float images under reference_formats (UNORM8 intermediate of a float source)"),
    (2, "fused kernel: tile footprint does not fit LDS at this scale"),
    (2, "precision FP32_EXACT: the fused kernel has no exact-stores form"),
    (2, "BGRA8 is an input-only format"),
    (2, "RGB10A2 images pair with an RGB10A2 (or RGBA32F) destination only"),
    (2, "RGB10A2 pipelines keep a 10-bit intermediate (quantize_intermediate = 1)"),
    (2, "precision FP32_EXACT: RCAS must write RGBA8 (a half, float or 10-bit destination promises no exact bytes)"),
]
UNREACHABLE = {"NIS tile does not fit LDS", "precision FP32_EXACT: the fused kernel has no exact-stores form"}


def test_refusal_coverage(probe, matrix_plans):
    table = [(int(s), t) for s, t in (x.split("\t", 1) for x in probe("--refusals"))]
    assert table == REFUSALS   # a new refusal, a changed status or text: this list and the matrix have to follow
    _, plans = matrix_plans
    seen = {(p["status"], p["text"]) for p in plans if p["status"]} | {(p["dest_status"], p["dest_text"]) for p in plans if p.get("dest_status")}
    assert seen == {r for r in REFUSALS if r[1] not in UNREACHABLE}, set(REFUSALS) - seen


def test_matrix_mask_is_a_mask(matrix_plans):
    """the masked cases of the matrix cannot silently become unmasked: at 160x128 each eye has at least one tile inside the radius, one ring
    tile and one outside tile that is not ring; and the eyes' centres are unequal (the lists are not shared)"""
    cases, plans = matrix_plans
    n = 0
    for c, p in zip(cases, plans):
        if c["mask"] and p["status"] == 0 and p["out"] == [160, 128] and p["upscale"]:
            n += 1
            assert p["tile_lists"] == (0 if c["cfg"]["precision"] == 2 else 1), c["id"]   # (the strict build tests the mask per group, without lists)
            if p["tile_lists"]:
                assert p["lists_shared"] == (c["kind"] == "shared"), c["id"]   # (a side-by-side texture: one mask with both centres)
                for eye in (0, 1):
                    assert p["inside"][eye] >= 1 and p["ring"][eye] >= 1 and p["outside"][eye] - p["ring"][eye] >= 1, (c["id"], p)
        if not c["mask"] and p["status"] == 0:
            assert not p["tile_lists"], c["id"]
    assert n >= 100, n


def test_matrix_invariants(matrix_plans):
    cases, plans = matrix_plans
    for c, p in zip(cases, plans):
        if p["status"] == 0:
            assert p["invariants"] == "ok", (c["id"], p["invariants"])


def test_agrees_with_the_gpu_record(matrix_plans):
    """status, text and owned format of every case, against what the parent commit's library did on the GPU"""
    record = json.load(open(os.path.join(ROOT, "tests", "golden", "launch_forms_parent.json")))
    cases, plans = matrix_plans
    assert set(record) == {c["id"] for c in cases}
    compared = 0
    for c, p in zip(cases, plans):
        rec = record[c["id"]]
        if "create" in rec:   # ovrfsr_create refused the configuration: the launch manager never saw it
            assert p["status"] == 1, (c["id"], p)
            continue
        calls = [tuple(x) for x in rec["calls"]]
        compared += 1
        if p["status"]:       # refused by the plan: the failed build disables the ctx
            assert calls == [(p["status"], p["text"]), (5, "post-processing disabled after an earlier failure; call reset")], (c["id"], p, calls)
            continue
        refused = p["dest_status"] != 0 and p["form"] != "none"
        if not refused:
            assert all(s == 0 for s, _ in calls), (c["id"], p, calls)
            if c["dst"] == "owned":
                assert rec["owned_format"] == (p["owned"] if p["form"] != "none" else _matrix().SOURCES[c["src"]]), (c["id"], p, rec)
            continue
        want = (p["dest_status"], p["dest_text"])
        after = (5, "post-processing disabled after an earlier failure; call reset") if p["dest_disables"] else want
        if c["kind"] == "pair" and not p["dest_disables"]:
            assert calls == [(0, ""), want, after], (c["id"], calls)   # the first eye is recorded, the pair refused when it is launched
        else:
            assert calls == [want, after], (c["id"], p, calls)
    assert compared >= 570, compared


# ---- (c) structural invariants of the tables --------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1, 1), (80, 64, 160, 128), (150, 110, 200, 147), (128, 96, 96, 72), (16384, 8, 16384, 16), (8, 16384, 16, 16384)]
LARGEST = (12288, 12288, 16384, 16384)
MASKS = [dict(radius=0.5, proj_centre=(0.2, 0.3, 0.8, 0.7)), dict(radius=0.12, proj_centre=(0.5, 0.5, 0.5, 0.5)), dict(radius=0.9, proj_centre=(0.0, 1.0, 1.0, 0.0)),
         dict(radius=2.0)]


def _invariant_lines(shape, variants):
    iw, ih, ow, oh = shape
    lines = []
    for mi, m in enumerate(MASKS):
        for name, fmt, one_eye, cfg in variants:
            lines.append(_line("%dx%d-%dx%d/mask%d/%s" % (iw, ih, ow, oh, mi, name), fmt, iw, ih, one_eye, -1, fsr_enabled=1, out_width=ow, out_height=oh,
                               **dict(m, **cfg)))
    return lines


VARIANTS = [("easu-rcas", RGBA8, 1, {}), ("easu-rcas-shared", RGBA8, 0, {}), ("easu-only", RGBA8, 1, dict(stage_mask=1)), ("fused", RGBA8, 1, dict(fused=1)),
            ("half", RGBA16F, 1, {}), ("nis", RGBA8, 1, dict(use_nis=1)), ("nis-half-shared", RGBA16F, 0, dict(use_nis=1)), ("strict", RGBA8, 1, dict(precision=2)),
            ("exact", RGBA8, 1, dict(precision=3))]


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d-%dx%d" % s for s in SHAPES])
def test_table_invariants(probe, shape):
    lines = _invariant_lines(shape, VARIANTS)
    plans = _plan_checked(probe, lines)
    planned = [p for p in plans if p["status"] == 0]
    assert planned, plans   # (NIS refuses 128x96 -> 96x72 and the fused kernel does not fit there: the other variants plan)
    for p in planned:
        assert p["invariants"] == "ok", p
        assert p["out"] == list(shape[2:]), p
    # the shapes' reasons: the ragged shape has partial last tiles in both axes, minification refuses the fixed-pitch fused kernel
    if shape == (150, 110, 200, 147):
        assert any(p["tile_lists"] and p["ring"][0] for p in planned)
    if shape == (128, 96, 96, 72):
        assert any(p["text"] == "fused kernel: tile footprint does not fit LDS at this scale" for p in plans)
    if shape[0] >= 8 and shape[1] >= 8:
        assert any(p["tile_lists"] for p in planned), shape


def _largest_lines():
    return _invariant_lines(LARGEST, VARIANTS[:1])[:1]


def test_table_invariants_largest_output(probe):
    """12288^2 -> 16384^2: 512 x 512 tiles per eye; tile lists only (the masked EASU+RCAS form)"""
    plans = _plan_checked(probe, _largest_lines())
    p = plans[0]
    assert p["status"] == 0 and p["form"] == "mask-sorted" and p["invariants"] == "ok", p
    assert p["inside"][0] + p["outside"][0] == 512 * 512 and p["spans"][0] > 0, p


def test_digest_record_names_these_lines():
    """the ids of (a)-(c), from the functions the tests above plan from, are unique, and the record holds no plan_probe id that none of them has"""
    lines = _form_lines() + _matrix_lines()[1] + [line for shape in SHAPES for line in _invariant_lines(shape, VARIANTS)] + _largest_lines()
    ids = [line.split(" ", 1)[0] for line in lines]
    assert len(set(ids)) == len(ids), sorted(i for i in set(ids) if ids.count(i) > 1)
    assert set(parent_digests("plan_probe")) <= set(ids)


# ---- machine code unmoved -----------------------------------------------------------------------------------------------------------
def test_fingerprint_unmoved():
    """the planner and what followed it are host refactors: against the record of the current library (profiles/isa_fingerprint.json, unchanged
    since the planner's parent commit) the library holds the same kernels, every one with the same machine code"""
    now = isa.fingerprint_of_built_library()
    before = isa.record("isa_fingerprint.json")
    assert set(now) == set(before), sorted(set(now) ^ set(before))
    assert [k for k in before if now[k] != before[k]] == []
