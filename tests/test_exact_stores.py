"""OVRFSR_PRECISION_FP32_EXACT (exact stores), the parts that need no GPU: the public value and its probe, the guarded RCAS instances in the
code object, the fingerprint record, and the tie-rich fixture the GPU tests stand on (tests/rcas_ties.py)."""
import ctypes as C
import os

import openvr_fsr_amd as A
from openvr_fsr_amd import _capi as K
from tests import isa
from tests.test_kernel_resources import kernels  # noqa: F401  (the code-object fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP_NOW, FP_BEFORE = "r06_isa_fingerprint_r06.json", "exact_stores_fingerprint_before.json"   # (records under profiles/: tests/isa.py)
# mangled-name fragments of the guarded instances: rcas_dpp_exact_kernel<SPANS, TH> and rcas_direct_exact_kernel
EXACT_KERNELS = ("21rcas_dpp_exact_kernelILb0ELi32E", "21rcas_dpp_exact_kernelILb0ELi16E", "21rcas_dpp_exact_kernelILb1ELi32E", "24rcas_direct_exact_kernel")
EXACT_NAMES = ("void ovrfsr_fast::rcas_dpp_exact_kernel<false, 32>(ovrfsr::RcasArgs)", "void ovrfsr_fast::rcas_dpp_exact_kernel<false, 16>(ovrfsr::RcasArgs)",
               "void ovrfsr_fast::rcas_dpp_exact_kernel<true, 32>(ovrfsr::RcasArgs)", "ovrfsr_fast::rcas_direct_exact_kernel(ovrfsr::RcasArgs)")


def test_create_accepts_precision_3_and_nothing_else_new():
    """The probe the header describes: ovrfsr_create with precision = 3 gets past validation (NO_DEVICE without a GPU, never INVALID_ARGUMENT);
    1, 4 and 7 are refused as before."""
    import torch
    assert K.PRECISION_FP32_EXACT == 3 and A.PRECISION_FP32_EXACT == 3
    assert (K.PRECISION_FP32, K.PRECISION_FP32_STRICT) == (0, 2)
    ctx = C.c_void_p()
    cfg = A.Config.default(fsr_enabled=1, precision=3)
    rc = A.library().ovrfsr_create(0, C.byref(cfg), C.byref(ctx))
    assert rc == (0 if torch.cuda.is_available() else 4), rc
    if ctx:
        A.library().ovrfsr_destroy(ctx)
    for p in (1, 4, 7, -1):
        ctx = C.c_void_p()
        cfg = A.Config.default(fsr_enabled=1, precision=p)
        assert A.library().ovrfsr_create(0, C.byref(cfg), C.byref(ctx)) == 1 and not ctx, p
    enum = open(os.path.join(ROOT, "include", "openvr_fsr_amd.h")).read().split("typedef enum ovrfsr_precision")[1].split("}")[0]
    assert "OVRFSR_PRECISION_FP32_EXACT = 3" in enum and "OVRFSR_PRECISION_FP32 = 0" in enum and "OVRFSR_PRECISION_FP32_STRICT = 2" in enum


def test_guarded_rcas_instances_exist_and_stay_in_registers(kernels):  # noqa: F811
    """No spills, no scratch, no AGPRs, no LDS, 256 threads.  The VGPR / SGPR counts are printed next to the unguarded twins'
    (profiles/exact_stores.txt records them; they are not a gate)."""
    twins = ("15rcas_dpp_kernelILi0ELb0ELi32E", "15rcas_dpp_kernelILi0ELb0ELi16E", "15rcas_dpp_kernelILi0ELb1ELi32E", "18rcas_direct_kernelILi0ELi0E")
    for frag, twin in zip(EXACT_KERNELS, twins):
        sel = {k: v for k, v in kernels.items() if "ovrfsr_fast" + frag in k}
        assert len(sel) == 1, (frag, sorted(sel))
        (name, v), = sel.items()
        (tname, t), = {k: w for k, w in kernels.items() if "ovrfsr_fast" + twin in k}.items()
        print("%s: %d VGPRs, %d SGPRs (twin %s: %d, %d)" % (name, v["vgpr_count"], v["sgpr_count"], tname, t["vgpr_count"], t["sgpr_count"]))
        assert not (v["vgpr_spill_count"] or v["sgpr_spill_count"] or v["private_segment_fixed_size"]), (name, v)
        assert v["agpr_count"] == 0 and v["group_segment_fixed_size"] == 0, (name, v)
        assert v["max_flat_workgroup_size"] == 256, (name, v)


def test_fingerprint_lists_the_new_kernels_and_keeps_every_old_hash():
    now, before = isa.record(FP_NOW), isa.record(FP_BEFORE)
    for name in EXACT_NAMES:
        assert name in now and name not in before, name
    assert sorted(set(now) - set(before)) == sorted(EXACT_NAMES)
    changed = sorted(k for k in before if now.get(k) != before[k])
    assert not changed, changed


def test_tie_rich_fixture():
    """tests/rcas_ties.py: at least 50 of the 96 x 96 image's pixels sit within 2^-15 byte of a rounding boundary under the oracle (a plain
    random image of that size: about 6 within 2^-13), and the image is reproducible."""
    from tests import rcas_ties as T
    img, harvested, n15, n13 = T.fixture(7)
    print("tie-rich fixture, seed 7: %d neighbourhoods harvested, %d pixels within 2^-15 byte, %d within 2^-13 byte" % (harvested, n15, n13))
    assert img.shape == (96, 96, 4) and img.dtype.name == "uint8" and (img[..., 3] == 255).all()
    assert harvested >= 50 and n13 >= n15 >= 50
    assert T.fixture(7)[0] is img
