"""ovrfsr_set_hdr_domain without a GPU (include/openvr_fsr_amd.h, "HDR domain"): (a) the C boundary -- symbols, refusals, and ovrfsr_hdr_map
against the numpy restatement of the two formulas (tests/hdrmap.py), bit for bit; (b) the planner under the setting, tests/debug/hdr_probe.cpp
linked from the planner's three sources under AddressSanitizer and UBSan as a stand-alone program: a float submission plans the pipeline of
its RGBA32F twin, keeps its own owned format, ignores a mesh, and UNORM submissions plan what they always planned; (c) the machine code:
against the parent build's record the library adds exactly the five pass kernels and moves none, and their code-object notes show what
bandwidth-bound copy kernels should."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import openvr_fsr_amd as A
from openvr_fsr_amd import _capi as K
from tests import hdrmap, isa
from tests import test_pipeline_plan as TP
from tests.test_kernel_resources import kernels  # noqa: F401  (the code-object fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openvr_fsr_amd", "csrc")
f32p = C.POINTER(C.c_float)
RGBA8, RGBA16F, RGBA32F, RGB10A2, BGRA8, R11G11B10F = 0, 1, 2, 3, 4, 6
MS4_RGBA16F = RGBA16F | 4 << 8


# ---- (a) the C boundary ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported():
    lib = C.CDLL(A.library_path())
    for name in ("ovrfsr_set_hdr_domain", "ovrfsr_get_hdr_domain", "ovrfsr_hdr_map"):
        assert hasattr(lib, name), name
    assert lib.ovrfsr_abi_version() == 5   # no ABI version change: a host probes for the symbols


def test_setter_and_getter_refuse_a_null_ctx():
    L = A.library()
    d = C.c_int(7)
    assert L.ovrfsr_set_hdr_domain(None, K.HDR_DOMAIN_SRTM) == 1
    assert L.ovrfsr_set_hdr_domain(None, K.HDR_DOMAIN_LINEAR) == 1
    assert L.ovrfsr_get_hdr_domain(None, C.byref(d)) == 1 and d.value == 7


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _special_triples():
    one, tiny = np.float32(1.0), np.float32(2.0 ** -24)
    below_one = np.float32(1.0 - 2.0 ** -24)                # 1 - max = 2^-24, under the 1/32768 clamp
    at_clamp = np.float32(1.0 - 2.0 ** -15)                 # 1 - max = 1/32768 exactly
    rows = [
        (0, 0, 0), (1e-45, 0, 0), (1e-45, 1e-41, 1e-39), (1.1754942e-38, 1e-40, 0),           # zero, fp32 denormals
        (5.9604645e-08, 5.9604645e-08, 0), (6.0975552e-05, 5.9604645e-08, 3e-06),             # half denormals
        (1, 1, 1), (1, 0, 0), (0, 0.5, 1), (65504, 65504, 65504), (65504, 1, 0), (0.25, 65504, 3),
        (65024, 65024, 64512), (65024, 0, 0), (0, 0, 64512), (64512, 65024, 1),               # the R11G11B10F maxima
        (below_one, 0.5, 0.25), (0.1, below_one, below_one), (one, 0.5, 0.25), (0.3, 0.2, one),
        (at_clamp, 0.5, 0), (np.nextafter(at_clamp, np.float32(0)), 0.5, 0), (np.nextafter(at_clamp, np.float32(2)), 0.5, 0),
        (tiny, tiny, tiny), (0.99, 0.98, 0.97), (4096, 0.25, 0.25), (1000, 999, 998),
    ]
    return np.asarray(rows, np.float32)


def _random_triples():
    rng = np.random.default_rng(0x5EED)
    mag = np.exp2(rng.uniform(-24.0, np.log2(65504.0), (100000, 3))).astype(np.float32)
    mag[rng.random((100000, 3)) < 0.02] = 0.0               # exact zeros among them
    return np.minimum(mag, np.float32(65504))


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "back"])
def test_hdr_map_equals_the_numpy_restatement(inverse):
    ref = hdrmap.back if inverse else hdrmap.forward
    triples = np.concatenate([_special_triples(), _random_triples()])
    # the back mapping also on what it will meet: forward-mapped values, all in [0, 1)
    inputs = [triples, hdrmap.forward(triples)] if inverse else [triples]
    for x in inputs:
        got, want = K.hdr_map(x, inverse), ref(x)
        bad = np.flatnonzero((_bits(got) != _bits(want)).any(axis=1))
        assert bad.size == 0, (x[bad[:4]].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())
    # known answers: the forward maximum of (1, 1, 1) is 1/2; the back mapping peaks at 32768 times the value
    assert K.hdr_map(np.ones((1, 3), np.float32)).tolist() == [[0.5, 0.5, 0.5]]
    assert K.hdr_map(np.asarray([[1.0, 0.5, 0.0]], np.float32), True).tolist() == [[32768.0, 16384.0, 0.0]]
    assert K.hdr_map(np.asarray([[1.0 - 2.0 ** -24, 0.5, 0.0]], np.float32), True)[0, 1] == 16384.0


def test_round_trip_is_close_but_not_the_identity():
    x = _random_triples()
    y = K.hdr_map(K.hdr_map(x), True)
    assert (_bits(x) != _bits(y)).any()
    # forward rounds the mapped value to 2^-24 of 1: below the clamp (max <= 16384) what comes back is within ~ (1 + max)^2 * 2^-24 of the
    # texel; a texel beyond 32767 meets the clamp and comes back as at most 32768
    m = x.max(axis=1, keepdims=True).astype(np.float64)
    low = m[:, 0] <= 16384.0
    assert low.any() and (np.abs(y.astype(np.float64) - x)[low] <= ((1.0 + m) ** 2 * 2.0 ** -23 + 1e-30)[low]).all()
    assert (~low).any() and y.max() <= 32768.0 and y[m[:, 0] > 40000.0].max() > 32000.0


def test_hdr_map_argument_checks():
    L = A.library()
    src = np.asarray([1, 2, 3, 4, 5, 6], np.float32)
    dst = np.full(6, 9, np.float32)
    sp, dp = src.ctypes.data_as(f32p), dst.ctypes.data_as(f32p)
    assert L.ovrfsr_hdr_map(None, dp, 2, 0) == 1 and L.ovrfsr_hdr_map(sp, None, 2, 0) == 1
    for inverse in (-1, 2, 255):
        assert L.ovrfsr_hdr_map(sp, dp, 2, inverse) == 1
    assert (dst == 9).all()                                  # nothing written by any refused call
    assert L.ovrfsr_hdr_map(None, None, 0, 0) == 0           # n = 0: nothing to read
    assert L.ovrfsr_hdr_map(sp, dp, 2, 0) == 0 and np.array_equal(dst.reshape(2, 3), hdrmap.forward(src.reshape(2, 3)))
    assert L.ovrfsr_hdr_map(dp, dp, 2, 1) == 0               # in place


# ---- (b) the planner ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe():
    """hdr_probe, built under the host sanitizers like tests/test_pipeline_plan.py's probe; -> plan(lines) -> one dict per line"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    tmp = tempfile.mkdtemp(prefix="ovrfsr_hdr_probe_")
    exe = os.path.join(tmp, "hdr_probe")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static + [
                    os.path.join(ROOT, "tests", "debug", "hdr_probe.cpp"), os.path.join(CSRC, "pipeline_plan.cpp"),
                    os.path.join(CSRC, "constants.cpp"), os.path.join(CSRC, "nis_config.cpp"), "-o", exe], check=True)

    def plan(lines):
        path = os.path.join(tmp, "cases.txt")
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-4000:]
        out = [json.loads(x) for x in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out

    yield plan
    shutil.rmtree(tmp, ignore_errors=True)


SHAPE = (80, 64, 160, 128)
M, U = dict(radius=0.5, proj_centre=(0.2, 0.3, 0.8, 0.7)), dict(radius=2.0)
WEDGE = [(0.0, 0.0), (0.6, 0.0), (0.0, 0.7)]   # a corner wedge that hides whole 32x32 (and 32x24) tiles of a 160x128 image


def _line(name, fmt, hdr, mesh=None, shape=SHAPE, dest=-1, **cfg):
    iw, ih, ow, oh = shape
    base = TP._line(name, fmt, iw, ih, 1, dest, fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, **cfg)
    tail = [hdr, 0] if mesh is None else [hdr, 1] + [repr(float(c)) for v in mesh for c in v]
    return base + " " + " ".join(str(t) for t in tail)


CONFIGS = [("%s-%s-rf%d" % (mn, fn, rf), dict(mask, use_nis=nis, reference_formats=rf))
           for mn, mask in (("masked", M), ("unmasked", U)) for fn, nis in (("fsr", 0), ("nis", 1)) for rf in (0, 1)]
SUBMISSIONS = [("rgba16f", RGBA16F), ("r11g11b10f", R11G11B10F), ("ms4-rgba16f", MS4_RGBA16F), ("rgba32f", RGBA32F)]
LISTS = ("inside", "ring", "outside", "rcas", "spans")


def _owned_rule(fmt, rf):
    return RGBA8 if rf else (RGBA32F if fmt == RGBA32F else RGBA16F)


@pytest.mark.parametrize("name,cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_float_submissions_plan_the_pipeline_of_the_rgba32f_line(probe, name, cfg):
    twin = probe([_line("twin", RGBA32F, 0, **cfg)])[0]
    assert twin["status"] == 0 and twin["hdr_domain"] == 0 and twin["digest"] == twin["digest_plain"]
    got = probe([_line(sn, fmt, 1, **cfg) for sn, fmt in SUBMISSIONS])
    for (sn, fmt), g in zip(SUBMISSIONS, got):
        assert g["status"] == 0 and g["hdr_domain"] == 1, (sn, g)
        assert g["form"] == twin["form"] and g["mid"] == twin["mid"] and g["pipeline"] == RGBA32F, (sn, g["form"], g["mid"])
        assert g["tile_lists"] == twin["tile_lists"] and all(g[k] == twin[k] for k in LISTS), sn
        assert g["digest_pipeline"] == twin["digest_pipeline"], sn            # ... and every other field of the plan, by value
        assert g["input"] == fmt and g["owned"] == _owned_rule(fmt, cfg["reference_formats"]), (sn, g["input"], g["owned"])
        assert g["resolve_in_staging"] == 0, sn                                # the front pass, where there is one, feeds the forward pass
    if cfg["radius"] < 2.0:
        assert twin["tile_lists"] == 1 and twin["inside"][0] and twin["outside"][0]   # (the mask does give this shape both kinds of tiles)


@pytest.mark.parametrize("name,cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_linear_is_the_plan_it_has_always_been(probe, name, cfg):
    for g in probe([_line(sn, fmt, 0, **cfg) for sn, fmt in SUBMISSIONS]):
        assert g["status"] == 0 and g["hdr_domain"] == 0 and g["digest"] == g["digest_plain"], g["id"]


def test_a_mesh_is_ignored_under_the_setting(probe):
    cases = [(sn, fmt, cfg) for sn, fmt in SUBMISSIONS for cfg in (M, U, dict(U, use_nis=1))]
    with_mesh = probe([_line(sn, fmt, 1, WEDGE, **cfg) for sn, fmt, cfg in cases])
    without = probe([_line(sn, fmt, 1, **cfg) for sn, fmt, cfg in cases])
    control = probe([_line(sn, fmt, 0, WEDGE, **cfg) for sn, fmt, cfg in cases])
    for (sn, _, _), a, b, c in zip(cases, with_mesh, without, control):
        assert a["status"] == 0 and a["hidden_area"] == 0 and a["skipped"] == [0, 0] and a["digest"] == b["digest"], sn
        assert c["hidden_area"] == 1 and min(c["skipped"]) > 0, sn               # (without the setting this mesh does hide tiles)


def test_unorm_submissions_ignore_the_setting(probe):
    cases = [(fmt, mesh, cfg) for fmt in (RGBA8, BGRA8, RGB10A2, RGBA8 | 4 << 8) for mesh in (None, WEDGE)
             for cfg in (M, U, dict(M, reference_formats=1), dict(U, use_nis=1), dict(M, precision=2), dict(M, precision=3))]
    on = probe([_line("on", fmt, 1, mesh, **cfg) for fmt, mesh, cfg in cases])
    off = probe([_line("off", fmt, 0, mesh, **cfg) for fmt, mesh, cfg in cases])
    for case, a, b in zip(cases, on, off):
        assert a["status"] == b["status"] == a["status_plain"], case
        if a["status"] != 0:    # (a 10-bit submission has no exact-stores pipeline, with or without the setting)
            continue
        assert a["hdr_domain"] == 0 and a["digest"] == b["digest"] and all(a[k] == b[k] for k in LISTS + ("form", "mid", "owned", "skipped")), case
        if case[1] is None:
            assert a["digest"] == a["digest_plain"], case


def test_other_builds_and_forms_follow_their_twin_too(probe):
    """the strict build, fused on request, EASU only, sharpen only, quantize_intermediate = 0, a caller's RGBA8 destination"""
    variants = [dict(M, precision=2), dict(U, precision=2), dict(M, fused=1), dict(U, fused=1), dict(M, fused=0), dict(U, stage_mask=1),
                dict(M, stage_mask=1), dict(U, quantize_intermediate=0), dict(M, quantize_intermediate=0)]
    for cfg in variants:
        twin = probe([_line("twin", RGBA32F, 0, **cfg)])[0]
        for g in probe([_line(sn, fmt, 1, dest=RGBA8, **cfg) for sn, fmt in SUBMISSIONS]):
            assert g["status"] == twin["status"] == 0 and g["digest_pipeline"] == twin["digest_pipeline"] and g["hdr_domain"] == 1, (cfg, g["id"])
    twin, half = probe([_line("twin", RGBA32F, 0, shape=(96, 80, 96, 80), stage_mask=2, **M), _line("half", RGBA16F, 1, shape=(96, 80, 96, 80), stage_mask=2, **M)])
    assert half["status"] == 0 and half["form"] == "sharpen only" and half["digest_pipeline"] == twin["digest_pipeline"] and half["owned"] == RGBA16F


def test_the_setting_refuses_nothing_new(probe):
    """what a float submission is refused for without the setting it is refused for with it, and nothing else"""
    variants = [dict(M, fused=1, reference_formats=1), dict(M, precision=3), dict(M, precision=3, reference_formats=1), dict(U, stage_mask=3),
                dict(M, precision=3, fused=1), dict(U, use_nis=1, precision=3)]
    shapes = [SHAPE, (200, 160, 128, 102), (168, 134, 128, 102), (160, 128, 128, 102), (128, 96, 96, 72), (300, 200, 100, 67)]
    lines = [(fmt, cfg, shape) for _, fmt in SUBMISSIONS for cfg in variants for shape in shapes[:1]] + \
            [(fmt, cfg, shape) for _, fmt in SUBMISSIONS for cfg in (M, U, dict(M, fused=1), dict(U, use_nis=1)) for shape in shapes[1:]]
    got = probe([_line("case%d" % i, fmt, 1, shape=shape, **cfg) for i, (fmt, cfg, shape) in enumerate(lines)])
    assert any(g["status"] != 0 for g in got) and any(g["status"] == 0 for g in got)
    for case, g in zip(lines, got):
        assert g["status"] == g["status_plain"], (case, g)
    # 168x134 -> 128x102: the footprint of a tile fits the generic EASU kernel's LDS planes with half texels and not with float ones (an
    # RGBA32F submission is refused there) -- the half submission keeps its own plan, the setting not applied (header)
    kept = [g for (fmt, cfg, shape), g in zip(lines, got) if shape == (168, 134, 128, 102) and fmt == RGBA16F and cfg is U]
    assert kept and all(g["status"] == 0 and g["hdr_domain"] == 0 and g["digest"] == g["digest_plain"] for g in kept), kept
    assert all(g["status"] != 0 for (fmt, cfg, shape), g in zip(lines, got) if shape == (168, 134, 128, 102) and fmt == RGBA32F)


# ---- (c) machine code ----------------------------------------------------------------------------------------------------------------------
NEW = re.compile(r"^void ovrfsr_fast::(hdr_forward_kernel<[12]>|hdr_back_kernel<[012]>)\(")


def test_fingerprint_scope():
    if not os.path.exists(isa.LIB):
        pytest.fail("libopenvr_fsr_amd.so is not built: run __graft_entry__.build()")
    now = isa.fingerprint_of_built_library()
    before = isa.record("hdr_domain_fingerprint_before.json")
    assert not sorted(k for k in before if now.get(k) != before[k])   # no kernel of the parent build moved or left
    added = sorted(set(now) - set(before))
    assert len(added) == 5 and all(NEW.match(k) for k in added), added
    # the records the earlier fingerprint tests read carry the new kernels with the built values
    for name in ("isa_fingerprint.json", "r06_isa_fingerprint_r06.json", "rcas_one_quotient_fingerprint_before.json", "exact_stores_fingerprint_before.json",
                 "reference_formats_fingerprint_before.json", "r11g11b10f_in_place_fingerprint_before.json"):
        rec = isa.record(name)
        assert not [k for k in added if rec.get(k) != now[k]], name


def test_code_object_notes(kernels):  # noqa: F811
    new = {k: v for k, v in kernels.items() if re.search(r"ovrfsr_fast(18hdr_forward_kernel|15hdr_back_kernel)ILi[012]E", k)}
    assert len(new) == 5, sorted(new)
    assert not [k for k in kernels if re.search(r"hdr_(forward|back)_kernel", k) and k not in new]   # (no strict-namespace copy: the mapping is exact)
    for k, v in new.items():
        assert not (v["vgpr_spill_count"] or v["sgpr_spill_count"] or v["private_segment_fixed_size"]), (k, v)   # no spill, no scratch
        assert v["group_segment_fixed_size"] == 0 and v["agpr_count"] == 0, (k, v)                              # no LDS, no AGPR
        assert v["max_flat_workgroup_size"] == 256, (k, v)
        assert v["vgpr_count"] <= 32, (k, v)   # copy kernels: far below the 64 VGPRs at which a SIMD still holds 8 waves


def test_the_kernels_are_plain_cpp():
    """no inline assembly, no LDS in the passes' source; memory through the accessors of fsr_bounds.h"""
    text = open(os.path.join(CSRC, "fsr_hdr_domain.inc")).read() + open(os.path.join(CSRC, "hdr_map.h")).read()
    code = re.sub(r"//.*", "", text)
    assert not re.search(r"\basm\b|__asm|__shared__|extern\s+__shared__", code)
    assert code.count("OVRFSR_IMAGE(") == 4 and "OVRFSR_AT(" in code
    assert not re.search(r"\*\s*reinterpret_cast", code)   # no dereference beside the accessors
