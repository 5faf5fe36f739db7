"""cfg.reference_formats (the reference's DetermineOutputFormat rule as an opt-in), the parts that need no GPU: the header and the ctypes
mirror, the validation, the six new outside-tile kernels and the guarded EASU instances' resources, and the scope of the machine-code change."""
import ctypes as C
import os
import re
import subprocess

import pytest

import openvr_fsr_amd as A
from tests import isa
from tests.test_kernel_resources import _alloc, kernels  # noqa: F401  (the code-object fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- ABI --------------------------------------------------------------------------------------------------------------------


def test_header_compiles_from_c11_with_the_named_field(tmp_path):
    """reserved[0] became reference_formats: same struct size, same ABI version, and the field sits where reserved[0] sat."""
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "openvr_fsr_amd.h"\n'
                   "int main(void) {\n"
                   "    ovrfsr_config c = {0};\n"
                   "    c.reference_formats = 1;\n"
                   "    c.reserved[0] = 0;\n"
                   '    printf("%zu %zu %zu %zu %u\\n", sizeof(ovrfsr_config), offsetof(ovrfsr_config, reference_formats),\n'
                   "           offsetof(ovrfsr_config, pair_submit), sizeof(c.reserved) / sizeof(c.reserved[0]), OVRFSR_ABI_VERSION);\n"
                   "    return c.reference_formats - 1;\n}\n")
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [80, 72, 68, 1, 5]
    assert C.sizeof(A.Config) == 80 and A.Config.reference_formats.offset == 72 and A.Config.reserved.offset == 76
    assert A.library().ovrfsr_abi_version() == 5


def test_default_is_off_and_the_field_round_trips():
    assert A.Config.default().reference_formats == 0
    cfg = A.Config.default(reference_formats=1)
    assert cfg.reference_formats == 1 and cfg.struct_size == 80
    raw = (C.c_int32 * 20).from_buffer_copy(cfg)
    assert raw[18] == 1 and raw[19] == 0   # where reserved[0] was
    # the config file has no such key (the reference has none): the parser leaves the field at its default
    rc, parsed = A.config_from_json('{"fsr": {"enabled": true, "referenceFormats": 1, "reference_formats": 1}}')
    assert rc == 0 and parsed.reference_formats == 0


@pytest.mark.parametrize("value", [2, -1, 256])
def test_create_rejects_other_values(value):
    """0 or 1 only: INVALID_ARGUMENT at create, before any device is touched (set_config: tests/test_gpu_reference_formats.py)."""
    ctx = C.c_void_p()
    cfg = A.Config.default(fsr_enabled=1, reference_formats=value)
    assert A.library().ovrfsr_create(0, C.byref(cfg), C.byref(ctx)) == 1 and not ctx


def test_create_accepts_the_rule():
    import torch
    ctx = C.c_void_p()
    cfg = A.Config.default(fsr_enabled=1, reference_formats=1)
    rc = A.library().ovrfsr_create(0, C.byref(cfg), C.byref(ctx))
    assert rc == (0 if torch.cuda.is_available() else 4), rc   # past the validation: NO_DEVICE without a GPU, never INVALID_ARGUMENT
    if ctx:
        A.library().ovrfsr_destroy(ctx)


# ---- kernels ----------------------------------------------------------------------------------------------------------------


def _outside_u8mid(kernels):  # noqa: F811
    """easu_outside_kernel<I, O, FMT_RGBA8> of a FLOAT source (I = 1 RGBA16F, 2 RGBA32F)"""
    return {k: v for k, v in kernels.items() if re.search(r"ovrfsr_fast19easu_outside_kernelILi[12]ELi\dELi0EEE", k)}


def test_the_six_outside_tile_kernels_are_built(kernels):  # noqa: F811
    sel = _outside_u8mid(kernels)
    got = sorted(tuple(int(x) for x in re.search(r"kernelILi(\d)ELi(\d)ELi0E", k).groups()) for k in sel)
    assert got == [(i, o) for i in (1, 2) for o in (0, 1, 2)], got
    for k, v in sel.items():
        assert not (v["vgpr_spill_count"] or v["sgpr_spill_count"] or v["private_segment_fixed_size"]), (k, v)
        assert _alloc(v["vgpr_count"]) <= 64, (k, v["vgpr_count"])   # the C5 rule of tests/test_kernel_resources.py


def test_no_fused_kernel_with_a_byte_intermediate_of_a_float_source(kernels):  # noqa: F811
    """cfg.fused = 1 is refused for that pair at (re)build; every fused_kernel<N, 0, ...> has N = 0 (RGBA8 input)."""
    fused = [k for k in kernels if "12fused_kernelILi" in k]
    assert fused
    bad = [k for k in fused if re.search(r"12fused_kernelILi[^0]\d*ELi0E", k)]
    assert not bad, bad


def test_guarded_easu_instances_stay_inside_the_half_store_forms_budget(kernels):  # noqa: F811
    """easu_fast_kernel<RGBA16F | RGBA32F, RGBA8, P, M> now carries the near-tie list and the tile maximum, as the half-store form
    <same input, RGBA16F, P, M> always has: no more registers than that one, no spill."""
    n = 0
    for k, v in kernels.items():
        m = re.search(r"ovrfsr_fast16easu_fast_kernelILi([12])ELi0ELi(\d+)ELb([01])E", k)
        if not m:
            continue
        n += 1
        twin = k.replace("ILi%sELi0E" % m.group(1), "ILi%sELi1E" % m.group(1))
        assert twin in kernels, twin
        assert _alloc(v["vgpr_count"]) <= _alloc(kernels[twin]["vgpr_count"]), (k, v["vgpr_count"], kernels[twin]["vgpr_count"])
        assert v["vgpr_count"] <= kernels[twin]["vgpr_count"], (k, v["vgpr_count"], kernels[twin]["vgpr_count"])
        assert not (v["vgpr_spill_count"] or v["sgpr_spill_count"] or v["private_segment_fixed_size"]), (k, v)
        assert v["group_segment_fixed_size"] >= 2048, (k, v)   # the list is there: 4 waves x 256 entries
    assert n == 12, n


def test_fingerprint_scope():
    """Against the parent commit's build (profiles/reference_formats_fingerprint_before.json) the library differs in exactly the twelve
    guarded easu_fast_kernel instances and the six new outside-tile kernels; no other kernel's machine code moved."""
    now = isa.fingerprint_of_built_library()
    before = isa.record("reference_formats_fingerprint_before.json")
    added = sorted(set(now) - set(before))
    assert not set(before) - set(now)
    assert added == ["void ovrfsr_fast::easu_outside_kernel<%d, %d, 0>(ovrfsr::EasuArgs)" % (i, o) for i in (1, 2) for o in (0, 1, 2)], added
    changed = sorted(k for k in before if now[k] != before[k])
    want = sorted("void ovrfsr_fast::easu_fast_kernel<%d, 0, %d, %s>(ovrfsr::EasuArgs)" % (i, p, m) for i in (1, 2) for p in (28, 32, 40) for m in ("false", "true"))
    assert changed == want, changed
    # and the records the other fingerprint tests read carry the same values
    for rec in ("r06_isa_fingerprint_r06.json", "isa_fingerprint.json"):
        d = isa.record(rec)
        for k in added + changed:
            assert d[k] == now[k], (rec, k)
