"""Multisampled inputs (OVRFSR_FORMAT_MS), the parts that need no GPU: the resolve rule's known answers, the resolve kernels' resources,
the shipped kernels' machine code, the header encoding and the Python descriptors."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import isa, msaa
from tests.test_kernel_resources import _alloc, kernels  # noqa: F401  (the code-object fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "openvr_fsr_amd", "libopenvr_fsr_amd.so")


# ---- the resolve rule (header, OVRFSR_FORMAT_MS) -----------------------------------------------------------------------------


def test_unorm8_rounds_half_up():
    ms = np.array([[[0, 0, 0, 0], [0, 0, 0, 0], [1, 1, 1, 1], [1, 1, 1, 1]]], np.uint8).reshape(1, 1, 4, 4)
    assert msaa.resolve_unorm8(ms).ravel().tolist() == [1, 1, 1, 1]              # (2 + 2) >> 2: the tie goes up
    one = np.array([0, 0, 0, 1], np.uint8).reshape(1, 1, 4, 1).repeat(4, axis=3)
    assert msaa.resolve_unorm8(one).ravel().tolist() == [0, 0, 0, 0]             # (1 + 2) >> 2
    three = np.array([0, 1, 1, 1], np.uint8).reshape(1, 1, 4, 1).repeat(4, axis=3)
    assert msaa.resolve_unorm8(three).ravel().tolist() == [1, 1, 1, 1]           # (3 + 2) >> 2
    two = np.array([[254, 255, 0, 1]], np.uint8).reshape(1, 1, 1, 4).repeat(2, axis=2)
    two[0, 0, 1] = [255, 255, 1, 2]
    assert msaa.resolve_unorm8(two).ravel().tolist() == [255, 255, 1, 2]         # (509 + 1) >> 1, (1 + 1) >> 1, (3 + 1) >> 1
    eight = np.full((1, 1, 8, 4), 255, np.uint8)
    assert msaa.resolve_unorm8(eight).ravel().tolist() == [255] * 4              # 2040 + 4 >> 3 stays in range


def test_bgra8_resolves_then_reorders():
    ms = np.array([[10, 20, 30, 40], [11, 21, 31, 41]], np.uint8).reshape(1, 1, 2, 4)
    assert msaa.resolve_bgra8(ms).ravel().tolist() == [31, 21, 11, 41]


def _pack(r, g, b, a):
    return np.array([r | (g << 10) | (b << 20) | (a << 30)], np.uint32).view(np.int32)[0]


def test_rgb10a2_ties():
    ms = np.array([[[_pack(0, 1022, 1, 0), _pack(1, 1023, 2, 3)]]], np.int32)    # S = 2: (1 + 1) >> 1, (2045 + 1) >> 1, (3 + 1) >> 1, (3 + 1) >> 1
    assert msaa.resolve_rgb10a2(ms)[0, 0] == _pack(1, 1023, 2, 2)
    ms4 = np.array([[[_pack(0, 0, 1023, 0), _pack(0, 1, 1023, 0), _pack(1, 0, 1023, 1), _pack(1, 0, 1022, 1)]]], np.int32)
    # S = 4: R (2 + 2) >> 2 = 1, G (1 + 2) >> 2 = 0, B (4091 + 2) >> 2 = 1023, A (2 + 2) >> 2 = 1
    assert msaa.resolve_rgb10a2(ms4)[0, 0] == _pack(1, 0, 1023, 1)
    ms8 = np.array([[[_pack(1023, 0, 0, 3)] * 8]], np.int32)
    assert msaa.resolve_rgb10a2(ms8)[0, 0] == _pack(1023, 0, 0, 3)


def test_half_sum_is_in_sample_order():
    # 1024 + 2^-14 is a tie in fp32 (ulp 2^-13 there) and rounds back to 1024: summed s0 + s1 + s2 + s3 the two small samples vanish.
    # Pairwise ((s0 + s1) + (s2 + s3)) would give 2^-14 / 4, the reverse order 2^-13 / 4: the stated order is the only answer.
    e = np.float16(2.0 ** -14)
    ms = np.array([1024, e, e, -1024], np.float16).reshape(1, 1, 4, 1).repeat(4, axis=3)
    assert msaa.resolve_float(ms).ravel().tolist() == [0.0] * 4
    rev = ms[:, :, ::-1, :]
    assert msaa.resolve_float(rev).ravel().tolist() == [2.0 ** -15] * 4
    # the result is rounded to half once, nearest even: (3 + (1 + 2^-10)) / 4 = 1 + 2^-12, a quarter of a half-ulp -> 1
    ms2 = np.array([1.0, 1.0, 1.0, 1.0 + 2.0 ** -10], np.float16).reshape(1, 1, 4, 1)
    assert float(msaa.resolve_float(ms2).ravel()[0]) == 1.0
    ms3 = np.array([1.0, 1.0 + 2.0 ** -10], np.float16).reshape(1, 1, 2, 1)   # 1 + 2^-11: tie between 1 and 1 + 2^-10 -> 1 (even)
    assert float(msaa.resolve_float(ms3).ravel()[0]) == 1.0
    ms4 = np.array([1.0 + 2.0 ** -10, 1.0 + 2.0 ** -9], np.float16).reshape(1, 1, 2, 1)  # 1 + 3 * 2^-11: tie -> 1 + 2^-9 (even)
    assert float(msaa.resolve_float(ms4).ravel()[0]) == 1.0 + 2.0 ** -9


def test_float_resolve_is_fp32_and_exact_scale():
    ms = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8], np.float32).reshape(1, 1, 8, 1)
    acc = np.float32(0.1)
    for v in (0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8):
        acc = np.float32(acc + np.float32(v))
    assert msaa.resolve_float(ms).ravel()[0] == np.float32(acc * np.float32(0.125))


def test_sample_sets_have_the_stated_layout():
    for fmt in msaa.FORMATS:
        ms = msaa.make_ms(9, 5, 4, fmt, "structured", 3)
        assert ms.shape[:3] == (5, 9, 4)
        r = msaa.resolve(ms, fmt)
        assert r.shape[:2] == (5, 9) and r.dtype == ms.dtype


# ---- the resolve kernels in the library -------------------------------------------------------------------------------------


def _resolve_kernels(kernels):  # noqa: F811
    return {k: v for k, v in kernels.items() if "resolve_kernel" in k}


def test_resolve_kernels_are_built_for_every_format_and_count(kernels):  # noqa: F811
    sel = _resolve_kernels(kernels)
    for f in range(5):                      # RGBA8, RGBA16F, RGBA32F, RGB10A2, BGRA8
        for s in (2, 4, 8):
            assert any(k == "_ZN11ovrfsr_fast14resolve_kernelILi%dELi%dEEEvPKhjmPhjjjj" % (f, s) for k in sel), (f, s, sorted(sel))


def test_resolve_kernels_budget(kernels):  # noqa: F811
    for k, v in _resolve_kernels(kernels).items():
        assert not (v["vgpr_spill_count"] or v["sgpr_spill_count"] or v["private_segment_fixed_size"]), (k, v)
        assert v["agpr_count"] == 0, (k, v)
        assert v["group_segment_fixed_size"] == 0, (k, v)
        assert v["max_flat_workgroup_size"] == 256, (k, v)
        assert _alloc(v["vgpr_count"]) <= 64, (k, v["vgpr_count"])  # a streaming kernel: 8 waves per SIMD


def _fused_msaa_kernels(kernels):  # noqa: F811
    """easu_fast_kernel with the 4-sample RGBA8 input code (FMT_RGBA8_MS4 = 0x400): the resolve inside the staging sweep"""
    return {k: v for k, v in kernels.items() if k.startswith("_ZN11ovrfsr_fast16easu_fast_kernelILi1024E")}


def test_fused_msaa_easu_instances_keep_easus_budget(kernels):  # noqa: F811
    """The resolving staging sweep must not cost EASU its 5 workgroups per CU (test_kernel_resources.py's rule for the RGBA8 kernel)."""
    sel = _fused_msaa_kernels(kernels)
    assert {k.split("ILi1024ELi0ELi")[1][:2] for k in sel} == {"28", "32", "40"}, sorted(sel)
    for k, v in sel.items():
        assert _alloc(v["vgpr_count"]) * 5 <= 512, (k, v["vgpr_count"])
        assert v["group_segment_fixed_size"] <= 2560, (k, v["group_segment_fixed_size"])
        assert not (v["vgpr_spill_count"] or v["sgpr_spill_count"] or v["private_segment_fixed_size"]), (k, v)
        assert v["agpr_count"] == 0, (k, v)
        assert v["max_flat_workgroup_size"] == 256, (k, v)


def test_resolve_pass_macro_compiles():
    """-DOVRFSR_MSAA_RESOLVE_PASS (measurement build: the resolve pass where the staging sweep would resolve) still type-checks."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not installed")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", "-Wno-unused-function", "-ffp-contract=on", "-x", "hip",
           "-DOVRFSR_MSAA_RESOLVE_PASS", "-fsyntax-only", "postprocessor.cpp"]
    r = subprocess.run(cmd, cwd=os.path.join(ROOT, "openvr_fsr_amd", "csrc"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_shipped_kernels_are_unchanged():
    """tools/isa_fingerprint.py of the built library against the last recorded fingerprint: every kernel it lists keeps its machine code;
    the only additions are the resolve kernels and the 4-sample RGBA8 instances of easu_fast_kernel."""
    if not os.path.exists(LIB):
        pytest.fail("libopenvr_fsr_amd.so is not built: run __graft_entry__.build()")
    now = isa.fingerprint_of_built_library()
    base = isa.record("r06_isa_fingerprint_r06.json")
    changed = sorted(k for k in base if now.get(k) != base[k])
    assert not changed, changed
    added = sorted(set(now) - set(base))
    assert added and all("resolve_kernel" in k or k.startswith("void ovrfsr_fast::easu_fast_kernel<1024,") for k in added), added


# ---- the public encoding ----------------------------------------------------------------------------------------------------


def test_header_macro(tmp_path):
    src = tmp_path / "ms.c"
    src.write_text('#include <stdio.h>\n#include "openvr_fsr_amd.h"\nint main(void){printf("%u %u %d\\n", OVRFSR_FORMAT_MS(OVRFSR_FORMAT_RGBA8_UNORM, 4),'
                   ' OVRFSR_FORMAT_MS(OVRFSR_FORMAT_RGB10A2_UNORM, 8), OVRFSR_FORMAT_SAMPLES_SHIFT); return 0;}\n')
    exe = tmp_path / "ms"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split() == ["1024", "2051", "8"]


def test_python_format_helper():
    from openvr_fsr_amd import _capi as K
    assert K.FORMAT_SAMPLES_SHIFT == 8
    assert K.format_ms(K.FORMAT_RGBA8, 4) == 0x400 and K.format_ms(K.FORMAT_BGRA8, 2) == 0x204 and K.format_ms(K.FORMAT_RGBA16F, 1) == 0x101


class _OnDevice:
    """A host tensor that reports itself as a device tensor: image_of only reads the descriptor (pointer, shape, strides)."""
    is_cuda = True

    def __init__(self, t):
        self._t = t

    def __getattr__(self, k):
        return getattr(self._t, k)

    def reshape(self, *shape):
        return _OnDevice(self._t.reshape(*shape))


def test_image_of_multisampled_tensors():
    from openvr_fsr_amd import _capi as K
    from openvr_fsr_amd.postprocessor import image_of
    for dt, fmt, tb in ((torch.uint8, K.FORMAT_RGBA8, 4), (torch.float16, K.FORMAT_RGBA16F, 8), (torch.float32, K.FORMAT_RGBA32F, 16)):
        t = torch.zeros(6, 7, 4, 4, dtype=dt)
        img = image_of(_OnDevice(t))
        assert (img.width, img.height, img.pitch_bytes, img.format) == (7, 6, 7 * 4 * tb, K.format_ms(fmt, 4))
        assert img.data == t.data_ptr()
    t = torch.zeros(6, 7, 2, 4, dtype=torch.uint8)
    assert image_of(_OnDevice(t), K.FORMAT_BGRA8).format == K.format_ms(K.FORMAT_BGRA8, 2)
    p = torch.zeros(5, 3, 8, dtype=torch.int32)
    img = image_of(_OnDevice(p))
    assert (img.width, img.height, img.pitch_bytes, img.format) == (3, 5, 3 * 8 * 4, K.format_ms(K.FORMAT_RGB10A2, 8))
    # a row-padded view keeps its pitch
    big = torch.zeros(6, 10, 4, 4, dtype=torch.uint8)
    img = image_of(_OnDevice(big[:, :7]))
    assert (img.width, img.pitch_bytes) == (7, 10 * 4 * 4)
    # samples that are not contiguous within a texel are refused
    with pytest.raises(ValueError):
        image_of(_OnDevice(torch.zeros(6, 4, 7, 4, dtype=torch.uint8).permute(0, 2, 1, 3)))
    # a batch of single-sample images handed to apply by mistake is still refused as before (not read as 7 or 5 samples)
    for bad in (torch.zeros(3, 6, 7, 4, dtype=torch.uint8), torch.zeros(3, 6, 5, dtype=torch.int32)):
        with pytest.raises(ValueError):
            image_of(_OnDevice(bad))
    # single-sample descriptors are unchanged
    img = image_of(_OnDevice(torch.zeros(6, 7, 4, dtype=torch.uint8)))
    assert (img.width, img.pitch_bytes, img.format) == (7, 28, K.FORMAT_RGBA8)
