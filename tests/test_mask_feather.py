"""The mask feather without a GPU (header, "mask feather"): the rule of csrc/mask_feather.h through ovrfsr_mask_feather_weights against a
numpy restatement, the guard's claim (no pixel of an outside group has w8 > 0), known answers, the setter and getter's argument checks as far
as they go without a ctx, and the machine code: nothing of the parent build moved, the kernel added is mask_feather_kernel, it needs no
scratch, and the new sources hold no inline assembly."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import isa
from tests.test_kernel_resources import kernels  # noqa: F401  (fixture: the code objects' metadata notes)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openvr_fsr_amd", "csrc")
SYMBOLS = ("ovrfsr_set_mask_feather", "ovrfsr_get_mask_feather", "ovrfsr_mask_feather_stats", "ovrfsr_mask_feather_weights")
GUARD = 12


def _A():
    import openvr_fsr_amd as A
    if not A.have_library():
        pytest.fail("libopenvr_fsr_amd.so is not built: run __graft_entry__.build()")
    return A


# ---- the rule, restated ------------------------------------------------------------------------------------------------------------------
def feather_px(width, out_h):
    """F: the expression of radius[0] (0.5f * cfg * outH, one rounding per product, truncated)"""
    v = np.float32(np.float32(0.5) * np.float32(width)) * np.float32(out_h)
    return int(v) if v > 0 else 0


def ramp(R, F):
    ro = R - GUARD if R > GUARD else 0
    ri = ro - F if ro > F else 0
    return ro, ri


def rule(centre, R, F, w, h):
    """(w8 [h, w] int64, inside [h, w] bool) by the header's rule, in numpy int64 / uint32"""
    c = [int(v) for v in centre]
    ro, ri = ramp(R, F)
    x, y = np.meshgrid(np.arange(w, dtype=np.int64), np.arange(h, dtype=np.int64))
    d2 = np.minimum((c[0] - x) ** 2 + (c[1] - y) ** 2, (c[2] - x) ** 2 + (c[3] - y) ** 2)
    if F >= 1 and ro >= 1:
        den = ro * ro - ri * ri
        w8 = np.clip(np.floor_divide(256 * (ro * ro - d2), den), 0, 256)
    else:
        w8 = np.full((h, w), 256, np.int64)
    with np.errstate(over="ignore"):
        gx, gy = ((x // 16) * 16 + 8).astype(np.uint32), ((y // 16) * 16 + 8).astype(np.uint32)
        cu = np.asarray(c, np.uint32)
        ax, ay, bx, by = cu[0] - gx, cu[1] - gy, cu[2] - gx, cu[3] - gy
        r2 = np.uint32((R * R) & 0xFFFFFFFF)
        inside = (ax * ax + ay * ay <= r2) | (bx * bx + by * by <= r2)
    return w8, inside


def band(w8, inside):
    return inside & (w8 < 256)


# (name, out w, out h, one eye per texture, eye, proj_centre, radius, width)
SHAPES = (("128x107", 128, 107, 1, 0, (0.2, 0.3, 0.8, 0.7), 0.9, 0.3),
          ("128x107/right", 128, 107, 1, 1, (0.2, 0.3, 0.8, 0.7), 0.9, 0.3),
          ("49x39", 49, 39, 1, 0, (0.2, 0.3, 0.8, 0.7), 0.9, 0.3),
          ("256x107/shared", 256, 107, 0, 0, (0.2, 0.3, 0.8, 0.7), 0.9, 0.3),
          ("column0", 128, 107, 1, 0, (0.0, 0.5, 0.0, 0.5), 0.9, 0.3),
          ("off-image", 128, 107, 1, 0, (1.3, 0.4, 1.3, 0.4), 0.9, 0.2),
          ("narrow", 128, 107, 1, 0, (0.5, 0.5, 0.5, 0.5), 0.6, 0.02),
          ("wide", 128, 107, 1, 0, (0.5, 0.5, 0.5, 0.5), 0.9, 2.0))


def constants(ow, oh, one_eye, eye, proj, radius, width):
    A = _A()
    centre, rad = A._capi.mask_constants(ow, oh, proj, radius, one_eye, eye)
    return centre, int(rad[0]), feather_px(width, oh)


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_the_weights_equal_the_numpy_rule(shape):
    A = _A()
    _, ow, oh, one_eye, eye, proj, radius, width = shape
    centre, R, F = constants(ow, oh, one_eye, eye, proj, radius, width)
    got_w8, got_in = A._capi.mask_feather_weights(centre, R, F, ow, oh)
    w8, inside = rule(centre, R, F, ow, oh)
    assert np.array_equal(got_w8.astype(np.int64), w8)
    assert np.array_equal(got_in.astype(bool), inside)
    # the guard: no pixel of an outside group has w8 > 0
    assert not ((w8 > 0) & ~inside).any()
    if shape[0] not in ("narrow",):
        assert band(w8, inside).any() and inside.any() and (~inside).any()


def test_known_answers():
    A = _A()
    centre, R, F = constants(128, 107, 1, 0, (0.2, 0.3, 0.8, 0.7), 0.9, 0.3)
    assert (int(centre[0]), int(centre[1]), R, F) == (25, 32, 48, 16)
    assert ramp(R, F) == (36, 20)
    w8, inside = A._capi.mask_feather_weights(centre, R, F, 128, 107)
    w8, inside = w8.astype(np.int64), inside.astype(bool)
    b = band(w8, inside)
    assert int(inside.sum()) == 5376 and int(b.sum()) == 4119
    assert int((b & (w8 > 0)).sum()) == 2361 and int((b & (w8 == 0)).sum()) == 1758
    # the ramp's ends: 256 at the centre, 0 from Ro outwards along a row
    assert w8[32, 25] == 256 and w8[32, 25 + 20] == 256 and w8[32, 25 + 21] < 256 and w8[32, 25 + 35] > 0 and w8[32, 25 + 36] == 0


def test_no_ramp_is_a_weight_of_256_everywhere():
    A = _A()
    for R, F in ((48, 0), (12, 16), (0, 5)):
        w8, _ = A._capi.mask_feather_weights((25, 32, 25, 32), R, F, 64, 48)
        assert (w8 == 256).all(), (R, F)


def test_the_weights_call_checks_its_arguments_and_writes_nothing():
    L = _A().library()
    c = (C.c_uint32 * 4)(25, 32, 25, 32)
    w8 = np.full(64 * 48, 7, np.uint16)
    ins = np.full(64 * 48, 7, np.uint8)
    pw, pi = w8.ctypes.data_as(C.POINTER(C.c_uint16)), ins.ctypes.data_as(C.POINTER(C.c_uint8))
    assert L.ovrfsr_mask_feather_weights(c, 20, 4, 64, 48, pw, pi, 64 * 48 - 1) == 1
    assert L.ovrfsr_mask_feather_weights(None, 20, 4, 64, 48, pw, pi, 64 * 48) == 1
    assert L.ovrfsr_mask_feather_weights(c, 20, 4, 0, 48, pw, pi, 64 * 48) == 1
    assert L.ovrfsr_mask_feather_weights(c, 20, 4, 64, 16385, pw, pi, 64 * 48) == 1
    assert L.ovrfsr_mask_feather_weights(c, 20, 4, 64, 48, None, pi, 64 * 48) == 1
    assert L.ovrfsr_mask_feather_weights(c, 20, 4, 64, 48, pw, None, 64 * 48) == 1
    assert (w8 == 7).all() and (ins == 7).all()
    assert L.ovrfsr_mask_feather_weights(c, 20, 4, 64, 48, pw, pi, 64 * 48) == 0 and not (w8 == 7).all()


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_symbols():
    L = _A().library()
    assert [s for s in SYMBOLS if not hasattr(L, s)] == []
    assert L.ovrfsr_abi_version() == 5


def test_null_ctx_is_an_invalid_argument():
    L = _A().library()
    w, n = C.c_float(), C.c_uint32()
    assert L.ovrfsr_set_mask_feather(None, 0.1) == 1
    assert L.ovrfsr_get_mask_feather(None, C.byref(w)) == 1
    assert L.ovrfsr_mask_feather_stats(None, C.byref(n)) == 1


def test_the_header_states_the_rule():
    text = open(os.path.join(ROOT, "include", "openvr_fsr_amd.h")).read()
    for needle in ("ovrfsr_set_mask_feather", "Ro  = R > 12 ? R - 12 : 0", "Ri  = Ro > F ? Ro - F : 0", "w8 = clamp(floor(256 * (Ro * Ro - d2) / den), 0, 256)",
                   "v = o + (s - o) * t", "IGNORE the setting", "cfg.radius"):
        assert needle in text, needle


# ---- machine code ------------------------------------------------------------------------------------------------------------------------
NEW = re.compile(r"^void ovrfsr_fast::mask_feather_kernel<256>\(")


def test_fingerprint_scope():
    if not os.path.exists(isa.LIB):
        pytest.fail("libopenvr_fsr_amd.so is not built: run __graft_entry__.build()")
    now = isa.fingerprint_of_built_library()
    before = isa.record("mask_feather_fingerprint_before.json")
    assert not sorted(k for k in before if now.get(k) != before[k])   # no kernel of the parent build moved or left
    added = sorted(set(now) - set(before))
    assert 1 <= len(added) <= 4 and all(NEW.match(k) for k in added), added
    # the records the earlier fingerprint tests read carry the new kernel with the built value
    for name in ("isa_fingerprint.json", "r06_isa_fingerprint_r06.json", "rcas_one_quotient_fingerprint_before.json", "exact_stores_fingerprint_before.json",
                 "reference_formats_fingerprint_before.json", "r11g11b10f_in_place_fingerprint_before.json", "hdr_domain_fingerprint_before.json",
                 "gaze_fingerprint_before.json", "dynamic_resolution_fingerprint_before.json"):
        for k in added:
            assert isa.record(name).get(k) == now[k], (name, k)
    # and none of the patterns older tests count kernels by
    for k in added:
        assert not re.search(r"hdr_(forward|back)_kernel|_kernelILi6E|tile_records_kernel|tap_tables_kernel", k)


def test_code_object_notes(kernels):  # noqa: F811
    new = {k: v for k, v in kernels.items() if "mask_feather_kernel" in k}
    assert 1 <= len(new) <= 4 and all("ovrfsr_fast" in k for k in new), sorted(new)
    for k, v in new.items():
        assert not (v["vgpr_spill_count"] or v["sgpr_spill_count"] or v["private_segment_fixed_size"]), (k, v)   # no spill, no scratch
        assert v["group_segment_fixed_size"] == 0 and v["agpr_count"] == 0, (k, v)                              # no LDS, no AGPR
        assert v["max_flat_workgroup_size"] == 256, (k, v)
        assert v["vgpr_count"] <= 128, (k, v)   # (the raw words of four pixels wait in registers: still four workgroups per CU)


def test_the_new_sources_are_plain_cpp():
    """no inline assembly and no LDS in the pass or the rule; memory through the accessors of fsr_bounds.h; the rule has one definition, which
    the C ABI's constants-only call and the launch manager use too"""
    inc = open(os.path.join(CSRC, "fsr_mask_feather.inc")).read()
    hdr = open(os.path.join(CSRC, "mask_feather.h")).read()
    code = re.sub(r"//.*", "", inc + hdr)
    assert not re.search(r"\basm\b|__asm|__shared__|__builtin_amdgcn", code)
    assert not re.search(r"\*\s*reinterpret_cast", code)
    assert "OVRFSR_IMAGE(" in inc and "OVRFSR_PLANE(" in inc and "contract(off)" in inc
    assert "template <int THREADS>" in inc
    assert "feather_w8(" in re.sub(r"//.*", "", open(os.path.join(CSRC, "capi.cpp")).read())
    assert "feather_box(" in re.sub(r"//.*", "", open(os.path.join(CSRC, "postprocessor.cpp")).read())
    tail = open(os.path.join(CSRC, "fsr_kernels.hip")).read()
    assert tail.index('#include "fsr_tap_tables.inc"') < tail.index('#include "fsr_mask_feather.inc"')
