"""cfg.reference_formats = 1 on the GPU: the reference's DetermineOutputFormat rule (PostProcessor.cpp:63-74) -- a float submission
(RGBA16F, RGBA32F, R11G11B10F, multisampled ones) runs through a UNORM8 intermediate and comes back as RGBA8.

Oracle composition for a float image f (R11G11B10F behind tests/packedf.py's decode, multisampled input behind the numpy resolve):
    float_to_unorm8(rcas(unorm8_to_float(float_to_unorm8(easu(f))), rcas_con(s), centre, rad))
The strict build equals it bit for bit; the product build's UNORM8 EASU store is the strict build's bit for bit (near-tie guard for float
sources), its pipeline output within 1 LSB.  With the field at 0 nothing changes."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import msaa, packedf, synth

pytestmark = pytest.mark.gpu
STRICT, FP32 = 2, 0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = (474, 360, 632, 480)
RAGGED = (61, 47, 80, 63)
SHARP = 0.9


def _hdr_image(iw, ih, seed, scale, kind):
    """tests/test_gpu_formats.py::_hdr_image: RGBA16F eye image reaching `scale` -- the structured generator scaled as a whole, or a
    DARK image (values <= 1) with sparse highlights at `scale`"""
    base = synth.structured_u8(iw, ih, seed).astype(np.float32) / 255.0
    if kind == "scaled":
        img = base * np.float32(scale)
    else:
        rng = np.random.default_rng(seed)
        img = base.copy()
        hot = rng.random((ih, iw)) < 0.02
        img[hot, :3] = np.float32(scale) * rng.uniform(0.5, 1.0, (int(hot.sum()), 3)).astype(np.float32)
    img = img.astype(np.float16)
    img[..., 3] = np.float16(1.0)
    return img


def _variants(imgh, seed=3):
    """{input kind: (what is submitted, the float32 image the pipeline sees)} of one RGBA16F image"""
    rng = np.random.default_rng(seed)
    f = imgh.astype(np.float32)
    ms = (f[:, :, None, :] * rng.uniform(0.9, 1.1, f.shape[:2] + (4, 4)).astype(np.float32)).astype(np.float16)
    ms[..., 3] = np.float16(1.0)
    packed = packedf.encode(f)
    packed_ms = packedf.encode(ms.astype(np.float32))
    return {
        "rgba16f": (imgh, f),
        "rgba32f": (f, f),
        "r11g11b10f": (packed, packedf.unpack(packed).astype(np.float32)),
        "rgba16f x4": (ms, msaa.resolve_float(ms).astype(np.float32)),
        "r11g11b10f x4": (packed_ms, packedf.resolve(packed_ms).astype(np.float32)),
    }


def _oracle(f, ow, oh, radius=2.0, eye=0, debug=0, sharp=SHARP, stages=3):
    """the composition of the module docstring -> uint8 [oh, ow, 4] (stages = 1: the EASU pass alone, stored as UNORM8)"""
    ih, iw = f.shape[:2]
    centre, rad = O.mask_constants(ow, oh, radius, eye=eye)
    mid8 = O.float_to_unorm8(O.easu(f, ow, oh, O.easu_con(iw, ih, ow, oh), centre, rad))
    if stages == 1:
        return mid8
    return O.float_to_unorm8(O.rcas(O.unorm8_to_float(mid8), O.rcas_con(sharp, debug), centre, rad))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _fmt(a):
    import openvr_fsr_amd as A
    return A.FORMAT_R11G11B10F if a.dtype == np.int32 else None


def _pp(ow, oh, **cfg):
    import openvr_fsr_amd as A
    kw = dict(fsr_enabled=1, out_width=ow, out_height=oh, radius=2.0, sharpness=SHARP, reference_formats=1)
    kw.update(cfg)
    return A.PostProcessor(**kw)


def _apply(src, ow, oh, out_dt=np.uint8, eye=0, in_format="auto", **cfg):
    """one ovrfsr_apply on a fresh ctx with a caller-owned `out` -> numpy"""
    import torch
    pp = _pp(ow, oh, **cfg)
    try:
        tdt = {np.uint8: torch.uint8, np.float16: torch.float16, np.float32: torch.float32, np.int32: torch.int32}[out_dt]
        out = pp.apply(eye, _dev(src), out_dtype=tdt, in_format=_fmt(src) if in_format == "auto" else in_format)
        torch.cuda.synchronize()
        return out.cpu().numpy()
    finally:
        pp.close()


def _apply_owned(src, ow, oh, eye=0, in_format="auto", **cfg):
    """one ovrfsr_apply with out->data == NULL -> (format the ctx chose, numpy copy of the ctx-owned image)"""
    import torch
    from openvr_fsr_amd import _capi as K
    from openvr_fsr_amd.postprocessor import _wrap, image_of
    pp = _pp(ow, oh, **cfg)
    try:
        t = _dev(src)
        oimg = K.Image()
        pp._check(pp._lib.ovrfsr_apply(pp._ctx, eye, C.byref(image_of(t, _fmt(src) if in_format == "auto" else in_format)), None, C.byref(oimg), pp._stream()))
        torch.cuda.synchronize()
        got = _wrap(oimg, t.device)
        return oimg.format, got.dtype, got.cpu().numpy()
    finally:
        pp.close()


def _lsb(a, b):
    d = np.abs(a.astype(np.int16) - b.astype(np.int16))
    return int(d.max()), int((d != 0).sum())


# ---- strict build: the composition, bit for bit -----------------------------------------------------------------------------


@pytest.mark.parametrize("kind", ["rgba16f", "rgba32f", "r11g11b10f", "rgba16f x4", "r11g11b10f x4"])
def test_strict_build_is_the_oracle_composition(gpu, kind):
    import torch
    from openvr_fsr_amd import _capi as K
    ran = 0
    for (iw, ih, ow, oh) in (RAGGED, BIG):
        for (scale, hk) in ((2.0, "scaled"), (40.0, "highlights")):
            src, f = _variants(_hdr_image(iw, ih, 5, scale, hk))[kind]
            for (radius, debug, eye) in ((2.0, 0, 0), (0.6, 0, 1), (0.6, 1, 0)):
                if (iw, ih, ow, oh) == BIG and hk == "scaled" and debug:
                    continue
                want = _oracle(f, ow, oh, radius, eye, debug)
                cfg = dict(precision=STRICT, radius=radius, debug_mode=debug)
                got = _apply(src, ow, oh, eye=eye, **cfg)
                assert _lsb(got, want) == (0, 0), ("caller-owned", kind, (iw, ih), scale, hk, radius, debug, _lsb(got, want))
                fmt, dt, own = _apply_owned(src, ow, oh, eye=eye, **cfg)
                assert fmt == K.FORMAT_RGBA8 and dt == torch.uint8 and own.shape == (oh, ow, 4), (fmt, dt, own.shape)
                assert np.array_equal(own, want), ("ctx-owned", kind, (iw, ih), scale, hk, radius, debug, _lsb(own, want))
                ran += 1
    assert ran == 11


def test_strict_build_caller_owned_float_out_and_float_intermediate(gpu):
    """A caller-owned `out` keeps selecting the final store conversion: RGBA32F out = the un-rounded RCAS result of the UNORM8 intermediate.
    quantize_intermediate = 0 keeps its fp32 intermediate; only the ctx-owned output's format follows the rule."""
    import torch
    from openvr_fsr_amd import _capi as K
    iw, ih, ow, oh = RAGGED
    imgh = _hdr_image(iw, ih, 5, 2.0, "scaled")
    f = imgh.astype(np.float32)
    centre, rad = O.mask_constants(ow, oh, 0.6)
    e = O.easu(f, ow, oh, O.easu_con(iw, ih, ow, oh), centre, rad)
    want = O.rcas(O.unorm8_to_float(O.float_to_unorm8(e)), O.rcas_con(SHARP), centre, rad)
    got = _apply(imgh, ow, oh, np.float32, precision=STRICT, radius=0.6)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    want0 = O.float_to_unorm8(O.rcas(e, O.rcas_con(SHARP), centre, rad))
    fmt, dt, own = _apply_owned(imgh, ow, oh, precision=STRICT, radius=0.6, quantize_intermediate=0)
    assert fmt == K.FORMAT_RGBA8 and dt == torch.uint8
    assert np.array_equal(own, want0)


# ---- content the guard tests run on -----------------------------------------------------------------------------------------

# (scale, kind, meant to saturate)
CONTENT = ((1.0, "scaled", False), (2.0, "scaled", True), (6.0, "highlights", True), (40.0, "highlights", True), (400.0, "highlights", True))


def _content(scale, kind, saturating):
    """The case's image, held to the content condition BY THE ORACLE: a guard test that meets no near-tie proves nothing.  At least 1 000
    in-range EASU channels within 2^-9 byte of a rounding boundary; 1 % .. 60 % of the intermediate bytes saturated where the case is
    meant to saturate."""
    iw, ih, ow, oh = BIG
    imgh = _hdr_image(iw, ih, 5, scale, kind)
    e = O.easu(imgh.astype(np.float32), ow, oh)[..., :3]
    x = np.clip(e, 0.0, 1.0).astype(np.float64) * 255.0
    inside = (x > 0.0) & (x < 255.0)
    near = inside & (np.abs((x - np.floor(x)) - 0.5) < 2.0 ** -9)
    sat = float((O.float_to_unorm8(e) == 255).mean())
    print("content %s x%g: %d near-tie channels (%.2f %%), %.1f %% of the intermediate bytes saturated" % (kind, scale, int(near.sum()), 100.0 * near.mean(), 100.0 * sat))
    assert near.sum() >= 1000, (scale, kind, int(near.sum()))
    if saturating:
        assert 0.01 <= sat <= 0.60, (scale, kind, sat)
    return imgh


# ---- product build ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("scale,kind,saturating", CONTENT)
def test_product_easu_store_is_the_strict_builds(gpu, scale, kind, saturating):
    """EASU alone into a caller-owned uint8 image: the UNORM8 store of a float source.  n_diff == 0 against the strict build (and so against
    the oracle), unmasked and masked, RGBA16F and RGBA32F staging."""
    iw, ih, ow, oh = BIG
    imgh = _content(scale, kind, saturating)
    for src in (imgh, imgh.astype(np.float32)):
        for radius in (2.0, 0.6):
            s = _apply(src, ow, oh, precision=STRICT, radius=radius, stage_mask=1)
            p = _apply(src, ow, oh, precision=FP32, radius=radius, stage_mask=1)
            mx, n_diff = _lsb(p, s)
            print("EASU store %s x%g %s radius %g: n_diff %d (max %d LSB)" % (kind, scale, src.dtype, radius, n_diff, mx))
            assert np.array_equal(s, _oracle(src.astype(np.float32), ow, oh, radius, stages=1))
            assert n_diff == 0, (scale, kind, str(src.dtype), radius, n_diff, mx)


@pytest.mark.parametrize("scale,kind,saturating", CONTENT)
def test_product_pipeline_within_one_lsb(gpu, scale, kind, saturating):
    import openvr_fsr_amd as A
    iw, ih, ow, oh = BIG
    imgh = _content(scale, kind, saturating)
    for radius in (2.0, 0.6):
        want = _oracle(imgh.astype(np.float32), ow, oh, radius)
        for fused in (-1, 0):
            got = _apply(imgh, ow, oh, precision=FP32, radius=radius, fused=fused)
            mx, n = _lsb(got, want)
            print("pipeline %s x%g radius %g fused %d: max %d LSB, %d differing bytes" % (kind, scale, radius, fused, mx, n))
            assert mx <= 1, (scale, kind, radius, fused, mx, n)
            assert (got[..., 3] == 255).all()
        with pytest.raises(A.OvrFsrError) as ei:
            _apply(imgh, ow, oh, precision=FP32, radius=radius, fused=1)
        assert ei.value.status == 2   # OVRFSR_ERR_UNSUPPORTED
    # the debug tint of the pixels outside the radius (easu_outside_kernel<.., RGBA8>: UNORM8 round trip, then the tint), every output format
    want = _oracle(imgh.astype(np.float32), ow, oh, 0.6, debug=1)
    got = _apply(imgh, ow, oh, precision=FP32, radius=0.6, debug_mode=1)
    assert _lsb(got, want)[0] <= 1, _lsb(got, want)
    for out_dt in (np.float16, np.float32):
        gotf = _apply(imgh, ow, oh, out_dt, precision=FP32, radius=0.6, debug_mode=1).astype(np.float32)
        wantf = _apply(imgh, ow, oh, out_dt, precision=STRICT, radius=0.6, debug_mode=1).astype(np.float32)
        assert np.abs(gotf - wantf).max() <= 1.001 / 255.0, (out_dt, float(np.abs(gotf - wantf).max()))


def test_fused_refusal_disables_until_reset(gpu):
    """cfg.fused = 1 with the rule and a float pipeline input fails the (re)build like the RGB10A2 case: UNSUPPORTED, the ctx disabled,
    `reset` enables it again (and a set_config to fused = -1 then runs); an RGBA8 input on the same configuration is served."""
    import torch
    import openvr_fsr_amd as A
    iw, ih, ow, oh = RAGGED
    imgh = _hdr_image(iw, ih, 5, 2.0, "scaled")
    for src in (imgh, imgh.astype(np.float32), packedf.encode(imgh.astype(np.float32))):
        pp = _pp(ow, oh, fused=1, radius=0.6)
        t = _dev(src)
        with pytest.raises(A.OvrFsrError) as ei:
            pp.apply(0, t, out_dtype=torch.uint8, in_format=_fmt(src))
        assert ei.value.status == 2
        with pytest.raises(A.OvrFsrError) as ei:
            pp.apply(0, t, out_dtype=torch.uint8, in_format=_fmt(src))
        assert ei.value.status == 5   # OVRFSR_ERR_DISABLED
        pp.reset()
        u8 = _dev(synth.structured_u8(iw, ih, 2))
        got = pp.apply(0, u8, out_dtype=torch.uint8)   # the fused kernel exists for an RGBA8 input
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), _apply(synth.structured_u8(iw, ih, 2), ow, oh, fused=1, radius=0.6, reference_formats=0))
        pp.set_config(A.Config.default(fsr_enabled=1, out_width=ow, out_height=oh, radius=0.6, sharpness=SHARP, reference_formats=1))
        got = pp.apply(0, t, out_dtype=torch.uint8, in_format=_fmt(src))
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), _apply(src, ow, oh, radius=0.6))
        pp.close()


# ---- the field where it must change nothing ---------------------------------------------------------------------------------


def test_rule_is_a_no_op_for_unorm_inputs(gpu):
    import openvr_fsr_amd as A
    from tests.test_gpu_formats import img10
    iw, ih, ow, oh = 96, 80, 128, 107
    u8 = synth.structured_u8(iw, ih, 4)
    for radius in (2.0, 0.5):
        for fused in (-1, 0, 1):
            for prec in (FP32, STRICT):
                cfg = dict(radius=radius, fused=fused, precision=prec)
                for (src, fmt, out_dt) in ((u8, None, np.uint8), (u8, A.FORMAT_BGRA8, np.uint8), (u8, None, np.float16)):
                    on = _apply(src, ow, oh, out_dt, in_format=fmt, reference_formats=1, **cfg)
                    off = _apply(src, ow, oh, out_dt, in_format=fmt, reference_formats=0, **cfg)
                    assert on.tobytes() == off.tobytes(), (radius, fused, prec, fmt, out_dt)
                if fused != 1:
                    p = img10(iw, ih, 3)
                    on = _apply(p, ow, oh, np.int32, in_format=None, reference_formats=1, **cfg)
                    off = _apply(p, ow, oh, np.int32, in_format=None, reference_formats=0, **cfg)
                    assert on.tobytes() == off.tobytes(), ("rgb10a2", radius, fused, prec)
    # ctx-owned outputs of those inputs keep their formats
    for (src, fmt, want) in ((u8, None, A.FORMAT_RGBA8), (u8, A.FORMAT_BGRA8, A.FORMAT_RGBA8), (img10(iw, ih, 3), None, A.FORMAT_RGB10A2)):
        f1, _, a = _apply_owned(src, ow, oh, in_format=fmt, reference_formats=1)
        f0, _, b = _apply_owned(src, ow, oh, in_format=fmt, reference_formats=0)
        assert f1 == f0 == want and a.tobytes() == b.tobytes()


def test_rule_off_keeps_the_ctx_owned_format_and_the_bytes(gpu):
    """The default (0) is this library's own behaviour: an RGBA16F input comes back as RGBA16F through a half intermediate, an RGBA32F one
    as RGBA32F; a caller-owned uint8 `out` with the rule off is still served through the half intermediate (not the rule-on bytes' path)."""
    import torch
    import openvr_fsr_amd as A
    iw, ih, ow, oh = RAGGED
    imgh = _hdr_image(iw, ih, 5, 1.0, "scaled")
    f0, dt, own = _apply_owned(imgh, ow, oh, reference_formats=0, precision=STRICT, radius=0.6)
    assert f0 == A.FORMAT_RGBA16F and dt == torch.float16
    centre, rad = O.mask_constants(ow, oh, 0.6)
    e = O.easu(imgh.astype(np.float32), ow, oh, O.easu_con(iw, ih, ow, oh), centre, rad)
    want = O.rcas(e.astype(np.float16).astype(np.float32), O.rcas_con(SHARP), centre, rad).astype(np.float16)
    assert np.array_equal(own.view(np.uint16), want.view(np.uint16))
    f0, dt, _ = _apply_owned(imgh.astype(np.float32), ow, oh, reference_formats=0)
    assert f0 == A.FORMAT_RGBA32F and dt == torch.float32
    f0, dt, _ = _apply_owned(packedf.encode(imgh.astype(np.float32)), ow, oh, reference_formats=0)
    assert f0 == A.FORMAT_RGBA16F


def test_nis_has_no_intermediate_only_the_ctx_owned_format_follows(gpu):
    """NVScaler / NVSharpen are single-stage: under the rule a float submission's ctx-owned output is RGBA8 and holds the bytes a
    caller-owned uint8 `out` gets with the rule off."""
    import torch
    import openvr_fsr_amd as A
    iw, ih, ow, oh = 96, 80, 128, 107
    imgh = _hdr_image(iw, ih, 5, 2.0, "scaled")
    for radius in (2.0, 0.5):
        for prec in (FP32, STRICT):
            cfg = dict(use_nis=1, sharpness=0.6, radius=radius, precision=prec)
            fmt, dt, own = _apply_owned(imgh, ow, oh, **cfg)
            assert fmt == A.FORMAT_RGBA8 and dt == torch.uint8
            assert np.array_equal(own, _apply(imgh, ow, oh, reference_formats=0, **cfg)), (radius, prec)
            assert np.array_equal(own, _apply(imgh, ow, oh, **cfg)), (radius, prec)


# ---- launch forms -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("radius", [2.0, 0.5])
def test_batches_equal_the_per_eye_result(gpu, radius):
    import torch
    iw, ih, ow, oh = 96, 80, 128, 107
    n = 5
    imgs = np.stack([_hdr_image(iw, ih, 20 + i, (1.0, 2.0, 40.0)[i % 3], ("scaled", "scaled", "highlights")[i % 3]) for i in range(n)])
    for src in (imgs, imgs.astype(np.float32), np.stack([packedf.encode(i.astype(np.float32)) for i in imgs])):
        pp = _pp(ow, oh, radius=radius, proj_centre=(0.45, 0.5, 0.55, 0.5))
        outs = torch.zeros((n, oh, ow, 4), dtype=torch.uint8, device="cuda")
        pp.apply_batch(_dev(src), outs, in_format=_fmt(src))
        torch.cuda.synchronize()
        got = outs.cpu().numpy()
        pp.close()
        for i in range(n):
            want = _apply(src[i], ow, oh, eye=i & 1, radius=radius, proj_centre=(0.45, 0.5, 0.55, 0.5))
            assert np.array_equal(got[i], want), (str(src.dtype), i)


def test_batch_shared(gpu):
    import torch
    iw, ih, ow, oh = 192, 80, 256, 107
    n = 3
    imgs = np.stack([_hdr_image(iw, ih, 40 + i, 2.0, "scaled") for i in range(n)])
    pp = _pp(ow, oh, radius=0.5)
    outs = torch.zeros((n, oh, ow, 4), dtype=torch.uint8, device="cuda")
    pp.apply_batch(_dev(imgs), outs, shared=True)
    torch.cuda.synchronize()
    got = outs.cpu().numpy()
    pp.close()
    from openvr_fsr_amd import _capi as K
    for i in range(n):
        # a side-by-side texture through ovrfsr_apply: bounds that span the whole texture
        pp = _pp(ow, oh, radius=0.5)
        o = pp.apply(0, _dev(imgs[i]), bounds=K.Bounds(0.0, 0.0, 0.5, 1.0), out_dtype=torch.uint8)
        torch.cuda.synchronize()
        assert np.array_equal(got[i], o.cpu().numpy()), i
        pp.close()


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_pair_submit_ctx_owned_images_are_rgba8(gpu, order):
    import torch
    from openvr_fsr_amd import _capi as K
    from openvr_fsr_amd.postprocessor import _wrap, image_of
    iw, ih, ow, oh = 96, 80, 128, 107
    pp = _pp(ow, oh, radius=0.5, pair_submit=1)
    for frame in range(2):
        imgs = {e: _hdr_image(iw, ih, 60 + 2 * frame + e, 2.0, "scaled") for e in (0, 1)}
        held, outs, pending = [], {}, []
        for eye in order:
            t = _dev(imgs[eye])
            held.append(t)
            oimg = K.Image()
            pp._check(pp._lib.ovrfsr_apply(pp._ctx, eye, C.byref(image_of(t)), None, C.byref(oimg), pp._stream()))
            pending.append(pp.pair_pending())
            assert oimg.format == K.FORMAT_RGBA8 and (oimg.width, oimg.height, oimg.pitch_bytes) == (ow, oh, ow * 4)
            outs[eye] = oimg
        assert pending == [True, False]
        assert outs[0].data != outs[1].data
        torch.cuda.synchronize()
        for eye in (0, 1):
            got = _wrap(outs[eye], held[0].device).cpu().numpy()
            assert np.array_equal(got, _apply(imgs[eye], ow, oh, eye=eye, radius=0.5)), (frame, eye)
    pp.close()


# ---- set_config, rebuilds, capture ------------------------------------------------------------------------------------------


def test_set_config_validates_and_rebuilds(gpu):
    import torch
    import openvr_fsr_amd as A
    iw, ih, ow, oh = RAGGED
    imgh = _hdr_image(iw, ih, 5, 2.0, "scaled")
    t = _dev(imgh)
    pp = _pp(ow, oh, radius=0.6, reference_formats=0)
    base = dict(fsr_enabled=1, out_width=ow, out_height=oh, radius=0.6, sharpness=SHARP)
    for bad in (2, -1):
        with pytest.raises(A.OvrFsrError) as ei:
            pp.set_config(A.Config.default(reference_formats=bad, **base))
        assert ei.value.status == 1
    pp.cfg = A.Config.default(reference_formats=0, **base)
    for value in (0, 1, 0, 1):
        pp.set_config(A.Config.default(reference_formats=value, **base))
        got = pp.apply(0, t)
        torch.cuda.synchronize()
        assert got.dtype == (torch.uint8 if value else torch.float16), value
        want = _apply(imgh, ow, oh, np.uint8 if value else np.float16, radius=0.6, reference_formats=value)
        assert got.cpu().numpy().tobytes() == want.tobytes(), value
    pp.close()


@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_toggle_under_capture_is_refused_like_any_build(gpu):
    import torch
    import openvr_fsr_amd as A
    iw, ih, ow, oh = 96, 80, 128, 107
    src = _dev(np.stack([_hdr_image(iw, ih, 70 + i, 2.0, "scaled") for i in range(2)]))
    base = dict(fsr_enabled=1, out_width=ow, out_height=oh, radius=0.5, sharpness=SHARP)
    pp = _pp(ow, oh, radius=0.5, reference_formats=0)
    out = torch.zeros((2, oh, ow, 4), dtype=torch.uint8, device="cuda")
    ref = torch.zeros_like(out)
    pp.apply_batch(src, ref)   # built with the rule off
    torch.cuda.synchronize()
    side = torch.cuda.Stream()

    def capture():
        g = torch.cuda.CUDAGraph()
        side.wait_stream(torch.cuda.current_stream())
        err = None
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                try:
                    pp.apply_batch(src, out)
                except A.OvrFsrError as e:
                    err = e
        torch.cuda.synchronize()
        return g, err

    pp.set_config(A.Config.default(reference_formats=1, **base))   # the toggle: the next call has to rebuild
    g, err = capture()
    assert err is not None and err.status == 1, err
    pp.apply_batch(src, ref)   # (the ctx stayed enabled) once outside the capture
    torch.cuda.synchronize()
    g, err = capture()
    assert err is None
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    assert np.array_equal(ref[0].cpu().numpy(), _apply(src[0].cpu().numpy(), ow, oh, radius=0.5))
    pp.close()


# ---- audit and checked builds -----------------------------------------------------------------------------------------------


def test_audit_build_finds_no_flip_in_float_source_unorm8_stores(gpu):
    """tools/debug/tie_audit.py --reference-formats against a fresh audit build: every product-resolved pixel of a float-source UNORM8 store
    re-resolved in reference order on the device -- unit range and every HDR kind, masked and unmasked, the three LDS pitches.  The band
    (2^-9 byte x max(1, tile maximum)) is audited, not derived: FLIPS 0 over >= 1e8 pixels, with pixels listed."""
    from tests.variants import variant
    lib = variant("audit", "-DOVRFSR_TIE_AUDIT")
    env = dict(os.environ, OVRFSR_LIB=lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "debug", "tie_audit.py"), "--reference-formats"], capture_output=True, text=True,
                       timeout=900, env=env, cwd=ROOT)
    print(r.stdout[-6000:])
    m = re.search(r"TOTAL audited (\d+) pixels, listed (\d+) \([\d.]+ %\), FLIPS (\d+), max \|product - strict\| ([\d.eE+-]+) of the band", r.stdout)
    assert m, (r.stdout[-1500:], r.stderr[-1500:])
    audited, listed, flips, dist = int(m.group(1)), int(m.group(2)), int(m.group(3)), float(m.group(4))
    print("audit: %d pixels, %d listed, %d flips, largest product-versus-strict distance %.3f of the band" % (audited, listed, flips, dist))
    assert r.returncode == 0 and flips == 0, m.group(0)
    assert audited >= 1e8 and listed > 0, m.group(0)


_CHILD = r"""
import ctypes, sys
sys.path.insert(0, %r)
import numpy as np
import openvr_fsr_amd as A
from tests import test_gpu_reference_formats as T
lib = A.library()
n = lib.ovrfsr_debug_bounds_slots()
buf = (ctypes.c_ulonglong * n)()
lib.ovrfsr_debug_bounds.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.c_int]
assert lib.ovrfsr_debug_bounds(buf, n, 1) == 0
ran = 0
for (iw, ih, ow, oh) in (T.RAGGED, (96, 80, 128, 107), (37, 29, 63, 49), (150, 120, 167, 133)):
    for (scale, kind) in ((1.0, "scaled"), (40.0, "highlights"), (400.0, "highlights")):
        for src in T._variants(T._hdr_image(iw, ih, 5, scale, kind)).values():
            for cfg in (dict(radius=2.0), dict(radius=0.5), dict(radius=0.5, fused=0), dict(radius=0.5, debug_mode=1), dict(radius=2.0, stage_mask=1),
                        dict(radius=0.5, stage_mask=1), dict(radius=0.5, precision=2), dict(radius=0.5, quantize_intermediate=0)):
                for out_dt in (np.uint8, np.float16):
                    T._apply(src[0], ow, oh, out_dt, **cfg)
                    ran += 1
                T._apply_owned(src[0], ow, oh, **cfg)
import torch; torch.cuda.synchronize()
assert lib.ovrfsr_debug_bounds(buf, n, 0) == 0
nk = (n - 5) // 3
v = list(buf)
print("reference_formats checked: launched %%d, checked %%d, out of bounds %%d" %% (ran, sum(v[2 * nk:3 * nk]), sum(v[:nk])))
"""


def test_checked_build(gpu):
    """The rule-on paths at small sizes against the -DOVRFSR_BOUNDS build: every access of the new outside-tile instances, the guarded
    EASU instances (their list, their tile maximum) and everything around them through the checked accessors, 0 violations."""
    from tests.variants import variant
    lib = variant("bounds", "-DOVRFSR_BOUNDS")
    env = dict(os.environ, OVRFSR_LIB=lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    m = re.search(r"reference_formats checked: launched (\d+), checked (\d+), out of bounds (\d+)", r.stdout)
    assert r.returncode == 0 and m, (r.stdout[-1500:], r.stderr[-1500:])
    print(m.group(0))
    assert int(m.group(1)) > 500 and int(m.group(2)) > 1e6 and int(m.group(3)) == 0, m.group(0)
