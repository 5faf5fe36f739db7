"""R11G11B10F inputs (OVRFSR_FORMAT_R11G11B10F), the parts that need no GPU: the decode rule against the format's definition for every
code, the multisample rule on packed samples, the unpack kernels' presence and resources, the shipped kernels' machine code, the header
and the Python descriptors."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import isa, msaa, packedf
from tests.test_kernel_resources import _alloc, kernels  # noqa: F401  (the code-object fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "openvr_fsr_amd", "libopenvr_fsr_amd.so")


# ---- the decode rule (header, OVRFSR_FORMAT_R11G11B10F) -----------------------------------------------------------------------


def test_shift_decode_equals_the_definition_for_every_code():
    """All 2048 R / G codes and all 1024 B codes: the half float whose bits are code << 4 (<< 5) IS the value exponent and mantissa
    define -- denormals, Inf and NaN included."""
    r = np.arange(2048, dtype=np.uint32)
    b = np.arange(1024, dtype=np.uint32)
    dec_r = packedf.unpack(packedf.pack(r, 0 * r, 0 * r))[..., 0].astype(np.float64)
    dec_g = packedf.unpack(packedf.pack(0 * r, r, 0 * r))[..., 1].astype(np.float64)
    dec_b = packedf.unpack(packedf.pack(0 * b, 0 * b, b))[..., 2].astype(np.float64)
    want_r, want_b = packedf.value_of(r, 6), packedf.value_of(b, 5)
    for dec, want in ((dec_r, want_r), (dec_g, want_r), (dec_b, want_b)):
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(dec), nan)
        assert np.array_equal(dec[~nan], want[~nan])
    # the landmarks of the format
    assert want_r[0] == 0.0 and want_r[1] == 2.0 ** -20 and want_b[1] == 2.0 ** -19          # smallest denormals: 1/64 (1/32) x 2^-14
    assert want_r[15 << 6] == 1.0 and want_b[15 << 5] == 1.0
    assert want_r[0x7BF] == packedf.MAX_RG == 65024.0 and want_b[0x3DF] == packedf.MAX_B == 64512.0
    assert np.isinf(want_r[0x7C0]) and np.isinf(want_b[0x3E0])
    assert np.isnan(want_r[0x7C1:]).all() and np.isnan(want_b[0x3E1:]).all()
    assert int(np.isnan(want_r).sum()) == 63 and int(np.isnan(want_b).sum()) == 31
    # the channels do not leak into each other and alpha reads 1.0
    one = packedf.unpack(packedf.pack([0x7FF, 0, 0], [0, 0x7FF, 0], [0, 0, 0x3FF])).view(np.uint16)
    assert one.tolist() == [[0x7FF0, 0, 0, 0x3C00], [0, 0x7FF0, 0, 0x3C00], [0, 0, 0x7FE0, 0x3C00]]


def test_encode_round_trips_through_the_decode():
    rng = np.random.default_rng(5)
    p = rng.integers(0, 2 ** 32, (64, 33), dtype=np.uint64).astype(np.uint32)
    r, g, b = packedf.channels(p.view(np.int32))
    keep = ((r >> 6) < 31) & ((g >> 6) < 31) & ((b >> 5) < 31)      # finite codes only
    dec = packedf.unpack(p.view(np.int32))
    again = packedf.encode(np.where(keep[..., None], dec.astype(np.float32), np.float32(0)))
    assert np.array_equal(again.view(np.uint32)[keep], p[keep])
    assert float(packedf.unpack(packedf.encode(np.array([1e9, 1e9, 1e9], np.float32)))[..., :3].astype(np.float32).max()) == 65024.0


def test_multisample_rule_on_packed_samples():
    """The packed resolve is msaa.resolve_float of the decoded half samples: fp32 sum in sample order, times 1/S, half to nearest even."""
    for s in (2, 4, 8):
        ms = packedf.make_ms(21, 9, s, "structured", 3, scale=3.0)
        want = msaa.resolve_float(packedf.unpack(ms))
        got = packedf.resolve(ms)
        assert got.dtype == np.float16 and got.shape == (9, 21, 4)
        assert got.tobytes() == want.tobytes()
        assert (got[..., 3] == np.float16(1.0)).all()
    # order: no negative values exist, so the sum order shows only where the fp32 sum lands next to a half rounding tie.  Two sample sets
    # (R = G codes; found by a search over random codes) whose in-order sum and reversed sum round to different halves:
    for codes, fwd, rev in (((1854, 342, 1617, 1567), 4544.0, 4548.0), ((1629, 677, 584, 878, 410, 295, 1400, 1356), 210.5, 210.625)):
        c = np.array(codes, np.uint32)
        ms = packedf.pack(c, c, c >> 1).reshape(1, 1, len(codes))
        assert packedf.resolve(ms)[0, 0, :2].tolist() == [fwd, fwd]
        assert packedf.resolve(np.ascontiguousarray(ms[..., ::-1]))[0, 0, :2].tolist() == [rev, rev]
    # the final rounding is to the nearest even half: (2048 + 1) / 2 = 1024.5 -> 1024, (2048 + 3) / 2 = 1025.5 -> 1026
    big = packedf.encode(np.array([2048.0] * 3, np.float32))
    for small, want in ((1.0, 1024.0), (3.0, 1026.0)):
        tie = np.array([big, packedf.encode(np.array([small] * 3, np.float32))], np.int32).reshape(1, 1, 2)
        assert packedf.resolve(tie)[0, 0, :3].tolist() == [want] * 3
    # neighbours of 1.0: (1 + (1 + 2^-6)) / 2 = 1 + 2^-7, blue's step is 2^-5
    one, nxt = packedf.pack(15 << 6, 15 << 6, 15 << 5), packedf.pack((15 << 6) + 1, (15 << 6) + 1, (15 << 5) + 1)
    pair = np.array([one, nxt], np.int32).reshape(1, 1, 2)
    assert packedf.resolve(pair)[0, 0, :3].astype(np.float64).tolist() == [1 + 2.0 ** -7, 1 + 2.0 ** -7, 1 + 2.0 ** -6]
    # S = 1 is the plain decode
    p = packedf.make(7, 5, "random", 1)
    assert packedf.resolve(p[..., None]).tobytes() == packedf.unpack(p).tobytes()


# ---- the unpack kernels in the library ----------------------------------------------------------------------------------------


def _packed_kernels(kernels):  # noqa: F811
    return {k: v for k, v in kernels.items() if "packed_resolve_kernel" in k}


def test_unpack_kernels_are_built_for_every_count(kernels):  # noqa: F811
    """One instance per sample count, S = 1 (the plain unpack) included.  The resolve pass has one rule for every build and precision, so
    its kernels -- these too -- exist in the fast namespace only."""
    sel = _packed_kernels(kernels)
    assert sorted(sel) == ["_ZN11ovrfsr_fast21packed_resolve_kernelILi%dEEEvPKhjmPhjjjj" % s for s in (1, 2, 4, 8)], sorted(sel)
    assert not any("ovrfsr_strict" in k and "resolve_kernel" in k for k in kernels)


def test_unpack_kernels_budget(kernels):  # noqa: F811
    """A streaming kernel at 8 waves per SIMD: at S = 8 the sixteen sample words of a texel pair and the fp32 accumulators fit 64 VGPRs."""
    sel = _packed_kernels(kernels)
    assert len(sel) == 4
    for k, v in sel.items():
        assert not (v["vgpr_spill_count"] or v["sgpr_spill_count"] or v["private_segment_fixed_size"]), (k, v)
        assert v["agpr_count"] == 0, (k, v)
        assert v["group_segment_fixed_size"] == 0, (k, v)
        assert v["max_flat_workgroup_size"] == 256, (k, v)
        assert _alloc(v["vgpr_count"]) <= 64, (k, v["vgpr_count"])


def test_only_the_unpack_kernels_are_added():
    """Against the last recorded fingerprint every listed kernel keeps its machine code, and against the one recorded with this format
    (which lists the multisample kernels too) nothing changed and nothing is missing or extra: the additions of this format are exactly
    the four packed_resolve_kernel instances."""
    if not os.path.exists(LIB):
        pytest.fail("libopenvr_fsr_amd.so is not built: run __graft_entry__.build()")
    now = isa.fingerprint_of_built_library()
    r06 = isa.record("r06_isa_fingerprint_r06.json")
    assert not sorted(k for k in r06 if now.get(k) != r06[k])
    added = sorted(set(now) - set(r06))
    mine = [k for k in added if "packed_resolve_kernel" in k]
    assert [k.split("(")[0] for k in mine] == ["void ovrfsr_fast::packed_resolve_kernel<%d>" % s for s in (1, 2, 4, 8)], mine
    rest = [k for k in added if k not in mine]
    assert len(rest) == 18 and all(k.startswith("void ovrfsr_fast::resolve_kernel<") or k.startswith("void ovrfsr_fast::easu_fast_kernel<1024,")
                                   for k in rest), rest
    rec = isa.record("isa_fingerprint.json")
    assert sorted(rec) == sorted(now)
    assert not sorted(k for k in rec if now[k] != rec[k])


def test_unpack_kernels_are_plain_cpp_with_one_vector_store():
    """Plain C++ with vector loads and stores: every store of the new kernels is one global 16-byte vector store."""
    text = open(os.path.join(ROOT, "openvr_fsr_amd", "csrc", "fsr_kernels.hip")).read()
    body = text[text.index("void packed_resolve_kernel"):text.index("} // namespace ovrfsr_fast", text.index("void packed_resolve_kernel"))]
    assert "asm" not in body and "__shared__" not in body and "OVRFSR_LDS" not in body
    assert body.count("*OVRFSR_AT(uint4, d +") == 1


# ---- the public encoding ------------------------------------------------------------------------------------------------------


def test_header_constants(tmp_path):
    src = tmp_path / "pf.c"
    src.write_text('#include <stdio.h>\n#include "openvr_fsr_amd.h"\nint main(void){ovrfsr_format f = OVRFSR_FORMAT_R11G11B10F;\n'
                   'printf("%d 0x%x %u\\n", (int)f, OVRFSR_FORMAT_MS(OVRFSR_FORMAT_R11G11B10F, 4), OVRFSR_ABI_VERSION); return 0;}\n')
    exe = tmp_path / "pf"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split() == ["6", "0x406", "5"]
    hdr = open(os.path.join(ROOT, "include", "openvr_fsr_amd.h")).read()
    assert "5 is unassigned" in hdr


def test_python_constants():
    import openvr_fsr_amd as A
    from openvr_fsr_amd import _capi as K
    assert K.FORMAT_R11G11B10F == 6 and A.FORMAT_R11G11B10F == 6
    assert K.format_ms(K.FORMAT_R11G11B10F, 4) == 0x406
    assert 5 not in (K.FORMAT_RGBA8, K.FORMAT_RGBA16F, K.FORMAT_RGBA32F, K.FORMAT_RGB10A2, K.FORMAT_BGRA8, K.FORMAT_R11G11B10F)


class _OnDevice:
    """A host tensor that reports itself as a device tensor: image_of only reads the descriptor (pointer, shape, strides)."""
    is_cuda = True

    def __init__(self, t):
        self._t = t

    def __getattr__(self, k):
        return getattr(self._t, k)

    def reshape(self, *shape):
        return _OnDevice(self._t.reshape(*shape))


def test_image_of_packed_float_tensors():
    from openvr_fsr_amd import _capi as K
    from openvr_fsr_amd.postprocessor import image_of
    t = torch.zeros(6, 7, dtype=torch.int32)
    img = image_of(_OnDevice(t), K.FORMAT_R11G11B10F)
    assert (img.width, img.height, img.pitch_bytes, img.format, img.data) == (7, 6, 28, K.FORMAT_R11G11B10F, t.data_ptr())
    # without the override the shape keeps meaning RGB10A2
    assert image_of(_OnDevice(t)).format == K.FORMAT_RGB10A2
    # multisampled: [H, W, S] int32 with the override
    for s in (2, 4, 8):
        m = torch.zeros(5, 3, s, dtype=torch.int32)
        img = image_of(_OnDevice(m), K.FORMAT_R11G11B10F)
        assert (img.width, img.height, img.pitch_bytes, img.format) == (3, 5, 3 * s * 4, K.format_ms(K.FORMAT_R11G11B10F, s))
        assert image_of(_OnDevice(m)).format == K.format_ms(K.FORMAT_RGB10A2, s)
    # a row-padded view keeps its pitch
    big = torch.zeros(6, 10, dtype=torch.int32)
    img = image_of(_OnDevice(big[:, :7]), K.FORMAT_R11G11B10F)
    assert (img.width, img.pitch_bytes) == (7, 40)
    # a packed tensor is no RGBA8 / RGBA16F image
    for bad in (K.FORMAT_RGBA8, K.FORMAT_RGBA16F, K.FORMAT_BGRA8):
        with pytest.raises(ValueError):
            image_of(_OnDevice(t), bad)
