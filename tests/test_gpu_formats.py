"""R10G10B10A2_UNORM images -- the other texture format the reference allocates (DetermineOutputFormat,
PostProcessor.cpp:63-74: a 10-bit submission keeps 10-bit intermediate and output textures) -- through the HIP path
against the oracle: the float filters of the oracle composed with the UNORM10 decode / encode stated here."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import synth

pytestmark = pytest.mark.gpu
STRICT, FP32 = 2, 0


def pack10(f):
    """float [H,W,4] -> packed dwords [H,W] (UNORM10 x3 + UNORM2): floor(sat(x)*scale + 0.5), fp32, unfused"""
    f = np.clip(np.asarray(f, np.float32), 0, 1)
    q = np.floor(f[..., :3] * np.float32(1023) + np.float32(0.5)).astype(np.uint32)
    a = np.floor(f[..., 3] * np.float32(3) + np.float32(0.5)).astype(np.uint32)
    return (q[..., 0] | (q[..., 1] << 10) | (q[..., 2] << 20) | (a << 30)).view(np.int32)


def unpack10(p):
    v = np.ascontiguousarray(p).view(np.uint32)
    out = np.empty(v.shape + (4,), np.float32)
    for c in range(3):
        out[..., c] = ((v >> (10 * c)) & 1023).astype(np.float32) / np.float32(1023)
    out[..., 3] = (v >> 30).astype(np.float32) / np.float32(3)
    return out


def img10(w, h, seed):
    rng = np.random.default_rng(seed)
    base = synth.structured_u8(w, h, seed).astype(np.float32) / 255.0
    base[..., :3] = np.clip(base[..., :3] + rng.uniform(-0.002, 0.002, (h, w, 3)).astype(np.float32), 0, 1)   # use all 10 bits
    base[..., 3] = 1.0
    return pack10(base)


def oracle_fsr10(p, ow, oh, sharp, radius=2.0, proj=(0.5,) * 4, eye=0, debug=0, stages=3):
    ih, iw = p.shape
    centre, rad = O.mask_constants(ow, oh, radius, proj, True, eye)
    x = unpack10(p)
    if stages & 1:
        x = unpack10(pack10(O.easu(x, ow, oh, O.easu_con(iw, ih, ow, oh), centre, rad)))     # 10-bit intermediate texture
    if stages & 2:
        x = O.rcas(x, O.rcas_con(sharp, debug), centre, rad)
    return x


def run10(p, ow, oh, out_dtype, eye=0, **kw):
    import torch
    import openvr_fsr_amd as A
    cfg = dict(fsr_enabled=1, out_width=ow, out_height=oh, radius=2.0)
    cfg.update(kw)
    pp = A.PostProcessor(**cfg)
    out = pp.apply(eye, torch.from_numpy(p).cuda(), out_dtype=out_dtype)
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    pp.close()
    return res


@pytest.mark.parametrize("iw,ih,ow,oh", [(96, 80, 128, 107), (150, 120, 200, 160), (61, 47, 80, 63)])
@pytest.mark.parametrize("radius,debug", [(2.0, 0), (0.5, 1)])
def test_fsr_rgb10a2_strict_bit_exact(gpu, iw, ih, ow, oh, radius, debug):
    import torch
    p = img10(iw, ih, 3)
    proj = (0.45, 0.5, 0.55, 0.5)
    want = oracle_fsr10(p, ow, oh, 0.8, radius, proj, 1, debug)
    got = run10(p, ow, oh, torch.int32, eye=1, precision=STRICT, sharpness=0.8, radius=radius, proj_centre=proj, debug_mode=debug)
    assert np.array_equal(got.view(np.uint32), pack10(want).view(np.uint32))
    gotf = run10(p, ow, oh, torch.float32, eye=1, precision=STRICT, sharpness=0.8, radius=radius, proj_centre=proj, debug_mode=debug)
    assert np.array_equal(gotf.view(np.uint32), want.view(np.uint32))
    # EASU alone (stage_mask 1) writes the 10-bit texture directly
    wante = oracle_fsr10(p, ow, oh, 0.8, radius, proj, 1, debug, stages=1)
    gote = run10(p, ow, oh, torch.int32, eye=1, precision=STRICT, sharpness=0.8, radius=radius, proj_centre=proj, debug_mode=debug, stage_mask=1)
    assert np.array_equal(gote.view(np.uint32), pack10(wante).view(np.uint32))


@pytest.mark.parametrize("radius", [2.0, 0.5])
def test_fsr_rgb10a2_product_tolerance(gpu, radius):
    import torch
    iw, ih, ow, oh = 330, 250, 440, 333
    p = img10(iw, ih, 9)
    want = unpack10(pack10(oracle_fsr10(p, ow, oh, 0.9, radius)))
    got = unpack10(run10(p, ow, oh, torch.int32, precision=FP32, sharpness=0.9, radius=radius))
    d = np.abs(got - want)[..., :3] * 1023.0
    # the 10-bit EASU pass runs in the reference's operator order in every build (easu_go): only RCAS's rounding noise is left
    assert d.max() <= 1.01 and (d > 0.5).mean() <= 4e-3, (float(d.max()), float((d > 0.5).mean()))
    assert np.array_equal(got[..., 3], want[..., 3])


def test_fsr_rgb10a2_rejections(gpu):
    import torch
    import openvr_fsr_amd as A
    p = img10(60, 50, 1)
    with pytest.raises(A.OvrFsrError):
        run10(p, 80, 67, torch.uint8)                       # 10-bit in -> 8-bit out is not a pair the reference forms
    with pytest.raises(A.OvrFsrError):
        run10(p, 80, 67, torch.int32, fused=1)              # two-kernel pipeline only
    pp = A.PostProcessor(fsr_enabled=1, out_width=80, out_height=67)
    with pytest.raises(A.OvrFsrError):
        pp.apply(0, torch.from_numpy(synth.random_u8(60, 50, 1)).cuda(), out_dtype=torch.int32)   # 8-bit in -> 10-bit out
    pp.close()


def test_nis_rgb10a2_strict_bit_exact(gpu):
    import torch
    import openvr_fsr_amd as A
    iw, ih, ow, oh = 150, 120, 200, 160
    p = img10(iw, ih, 4)
    cs, cu = A.nis_coefs()
    ok, cfg = A.nis_scaler_config(0.6, iw, ih, ow, oh)
    assert ok
    for radius in (2.0, 0.5):
        centre, rad = O.mask_constants(ow, oh, radius)
        want = O.nis_upscale(unpack10(p), ow, oh, O.nis_block(cfg, centre, rad, 0), cs, cu)
        got = run10(p, ow, oh, torch.int32, precision=STRICT, use_nis=1, sharpness=0.6, radius=radius)
        assert np.array_equal(got.view(np.uint32), pack10(want).view(np.uint32)), radius
        gotp = unpack10(run10(p, ow, oh, torch.int32, precision=FP32, use_nis=1, sharpness=0.6, radius=radius))
        assert (np.abs(gotp - unpack10(pack10(want)))[..., :3] * 1023 <= 1.01).mean() >= 0.99


def test_rgb10a2_ctx_owned_output_and_ppm(gpu, tmp_path):
    import ctypes as C
    import torch
    import openvr_fsr_amd as A
    iw, ih, ow, oh = 96, 80, 128, 107
    p = img10(iw, ih, 5)
    pp = A.PostProcessor(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.7, radius=2.0, precision=STRICT)
    out = pp.apply(0, torch.from_numpy(p).cuda())            # ctx-owned output keeps the 10-bit format (PostProcessor.cpp:63-74)
    assert out.dtype == torch.int32 and tuple(out.shape) == (oh, ow)
    want = oracle_fsr10(p, ow, oh, 0.7)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), pack10(want).view(np.uint32))
    from openvr_fsr_amd.postprocessor import image_of
    path = str(tmp_path / "ten.ppm")
    assert A.library().ovrfsr_save_ppm(C.byref(image_of(out)), path.encode(), None) == 0
    data = open(path, "rb").read()
    hdr = b"P6\n%d %d\n255\n" % (ow, oh)
    assert data.startswith(hdr) and len(data) == len(hdr) + ow * oh * 3
    rgb = np.frombuffer(data[len(hdr):], np.uint8).reshape(oh, ow, 3)
    assert np.abs(rgb.astype(np.float32) / 255.0 - unpack10(pack10(want))[..., :3]).max() <= 0.5 / 255 + 1e-6
    pp.close()


# ------------------------------------------------------------------------------------------------
# B8G8R8A8 submissions (input only): the reference views them through a typed SRV and writes R8G8B8A8
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nis,radius,prec", [(0, 2.0, STRICT), (0, 0.5, FP32), (1, 2.0, STRICT), (1, 0.5, FP32)])
def test_bgra8_input_equals_rgba8(gpu, nis, radius, prec):
    """A BGRA8 image is re-ordered by a copy kernel and then takes the RGBA8 pipeline: bit-identical to submitting the
    RGBA8 image, for single applies (ctx-owned output) and strided batches, FSR and NIS (whose luma weights are not symmetric
    in R and B), every build."""
    import torch
    import openvr_fsr_amd as A
    iw, ih, ow, oh = 150, 120, 200, 160
    imgs = np.stack([synth.structured_u8(iw, ih, 40 + i) for i in range(3)])
    bgra = np.ascontiguousarray(imgs[..., [2, 1, 0, 3]])
    kw = dict(fsr_enabled=1, use_nis=nis, out_width=ow, out_height=oh, sharpness=0.8, radius=radius, precision=prec, debug_mode=1)
    pp = A.PostProcessor(**kw)
    want = torch.empty((3, oh, ow, 4), dtype=torch.uint8, device="cuda")
    pp.apply_batch(torch.from_numpy(imgs).cuda(), want, first_eye=1, alternate_eyes=True)
    pad = torch.zeros((3, ih, iw + 5, 4), dtype=torch.uint8, device="cuda")     # row pitch wider than the image
    pad[:, :, :iw] = torch.from_numpy(bgra).cuda()
    got = torch.zeros_like(want)
    pp.apply_batch(pad[:, :, :iw], got, first_eye=1, alternate_eyes=True, in_format=A.FORMAT_BGRA8)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    one = pp.apply(1, torch.from_numpy(bgra[0]).cuda(), in_format=A.FORMAT_BGRA8)   # ctx-owned output: R8G8B8A8
    assert one.dtype == torch.uint8 and torch.equal(one, want[0])
    with pytest.raises(A.OvrFsrError):
        from openvr_fsr_amd.postprocessor import image_of
        import ctypes as C
        o = image_of(got[0], A.FORMAT_BGRA8)
        i = image_of(torch.from_numpy(imgs[0]).cuda())
        pp._check(pp._lib.ovrfsr_apply(pp._ctx, 0, C.byref(i), None, C.byref(o), None))   # BGRA8 as a destination
    pp.close()


# ------------------------------------------------------------------------------------------------
# RGBA16F with values above 1 (HDR): the half near-tie guard's band follows the binade (round 4)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 6.0, 40.0])
def test_half_pipeline_hdr_values(gpu, scale):
    """EASU -> half intermediate -> RCAS on RGBA16F images whose values reach `scale`.  The strict build is bit-exact against the
    oracle at every magnitude (the filters are homogeneous only up to RCAS's peak constant, so this is a real case, not a rescaled
    one); the product build's error stays within 1e-3 RELATIVE to the image's magnitude -- the re-association error it guards
    against is relative, and since round 4 so is the band of the half near-tie guard (rounds 2-3 used an absolute 2^-17: no cover
    at all above 2.0, where the half spacing outgrows it)."""
    from tests.util import run_gpu
    iw, ih, ow, oh = 237, 180, 316, 240
    base = synth.structured_u8(iw, ih, 91).astype(np.float32) / 255.0
    imgh = (base * np.float32(scale)).astype(np.float16)
    imgh[..., 3] = np.float16(1.0)
    centre, rad = O.mask_constants(ow, oh, 0.6)
    e = O.easu(imgh.astype(np.float32), ow, oh, O.easu_con(iw, ih, ow, oh), centre, rad)
    want = O.rcas(e.astype(np.float16).astype(np.float32), O.rcas_con(0.9), centre, rad).astype(np.float16)
    kw = dict(sharpness=0.9, radius=0.6)
    got = run_gpu(imgh, ow, oh, np.float16, precision=STRICT, **kw)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), scale
    for fused in (-1, 0, 1):
        got = run_gpu(imgh, ow, oh, np.float16, precision=FP32, fused=fused, **kw).astype(np.float32)
        w32 = want.astype(np.float32)
        ok = np.isfinite(w32)
        err = np.abs(got[ok] - w32[ok])
        assert err.max() <= 1e-3 * max(1.0, scale), (scale, fused, float(err.max()))
        assert np.array_equal(np.isfinite(got), ok)


def _hdr_image(iw, ih, seed, scale, kind):
    """RGBA16F eye image reaching `scale`: the structured generator scaled as a whole, or a DARK image (values <= 1) with sparse
    highlights at `scale` -- taps tens of times the output value, the case the binade-relative band of round 4 did not cover"""
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


@pytest.mark.parametrize("scale,kind", [(1.0, "scaled"), (6.0, "scaled"), (40.0, "scaled"), (6.0, "highlights"), (40.0, "highlights"), (400.0, "highlights")])
def test_half_intermediate_is_the_strict_builds_also_on_hdr(gpu, scale, kind):
    """Round 5 (VERDICT r4 Next #5): the HALF near-tie guard scales its band with the largest texel of the tile's footprint, so the
    product kernels' half intermediate equals the strict build's BIT FOR BIT for every channel >= xmin on HDR content too -- read here
    as the output of an EASU-only RGBA16F pass with the guard forced on from 0.5 (OVRFSR_TIE_HALF_MIN, the value the sharpness-0.9
    pipeline uses).  Channels below xmin are outside the guard's contract (a flipped half-ulp there stays under 1e-3 behind RCAS's
    largest gain): they may differ by one half-ulp, no more.
    Round 6: the shipped library no longer reads that environment variable -- only audit builds do (the same kernels plus the
    re-resolve that counts flips; what they STORE is the product's) -- so the body runs in a subprocess against ab/audit.so."""
    import os
    import subprocess
    import sys
    if os.environ.get("OVRFSR_HALF_GUARD_INNER") != "1":
        from tests.variants import ROOT, variant
        lib = variant("audit", "-DOVRFSR_TIE_AUDIT")
        env = dict(os.environ, OVRFSR_LIB=lib, OVRFSR_TIE_HALF_MIN="0.5", OVRFSR_HALF_GUARD_INNER="1", PYTHONPATH=ROOT)
        node = "%s::test_half_intermediate_is_the_strict_builds_also_on_hdr[%s-%s]" % (os.path.abspath(__file__), scale, kind)
        r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "-m", "gpu", node], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        assert r.returncode == 0 and "1 passed" in r.stdout, (r.stdout[-1500:], r.stderr[-500:])
        return
    from tests.util import run_gpu
    iw, ih, ow, oh = 474, 360, 632, 480
    for seed in (5, 6):
        imgh = _hdr_image(iw, ih, seed, scale, kind)
        kw = dict(stage_mask=1, radius=2.0)
        s = run_gpu(imgh, ow, oh, np.float16, precision=STRICT, **kw)
        p = run_gpu(imgh, ow, oh, np.float16, precision=FP32, **kw)
        s32, p32 = s[..., :3].astype(np.float32), p[..., :3].astype(np.float32)
        guarded = np.maximum(s32, p32) >= 0.5
        differ = s[..., :3].view(np.uint16) != p[..., :3].view(np.uint16)
        assert guarded.sum() > 1000, "the case must exercise the guard"
        assert not (differ & guarded).any(), "%d guarded half stores differ from the strict build (scale %g, %s)" % (int((differ & guarded).sum()), scale, kind)
        ulp = np.maximum(np.abs(s32), 2.0 ** -14) * 2.0 ** -10        # one half spacing (upper bound inside the binade)
        assert (np.abs(s32 - p32)[differ] <= ulp[differ] * 1.0001).all()


@pytest.mark.parametrize("dt", [np.uint8, np.float16, np.float32])
def test_capture_dds(gpu, tmp_path, dt):
    """ovrfsr_save_dds: the F7 capture in the reference's own container (SaveDDSTextureToFile, PostProcessor.cpp:640-657) -- DX10-extended
    DDS, the texels as they sit in the image (row pitch removed), parsed back here field by field."""
    import ctypes as C
    import struct
    import torch
    import openvr_fsr_amd as A
    from openvr_fsr_amd.postprocessor import image_of
    ow, oh, pad = 77, 45, 5
    tdt = {np.uint8: torch.uint8, np.float16: torch.float16, np.float32: torch.float32}[dt]
    big = (torch.rand((oh, ow + pad, 4), device="cuda") * (255 if dt == np.uint8 else 3.0)).to(tdt)   # a view with a row pitch wider than the image
    view = big[:, :ow]
    path = str(tmp_path / "cap.dds")
    assert A.library().ovrfsr_save_dds(C.byref(image_of(view)), path.encode(), None) == 0
    data = open(path, "rb").read()
    tb = np.dtype(dt).itemsize * 4
    assert len(data) == 4 + 124 + 20 + ow * oh * tb
    magic, size, flags, height, width, pitch = struct.unpack_from("<6I", data, 0)
    assert magic == 0x20534444 and size == 124 and flags == 0x100f and (height, width, pitch) == (oh, ow, ow * tb)
    pf_size, pf_flags, fourcc = struct.unpack_from("<3I", data, 4 + 72)
    assert pf_size == 32 and pf_flags == 4 and fourcc == struct.unpack("<I", b"DX10")[0]
    dxgi, dim, misc, array, misc2 = struct.unpack_from("<5I", data, 128)
    assert dxgi == {np.uint8: 28, np.float16: 10, np.float32: 2}[dt] and dim == 3 and array == 1
    px = np.frombuffer(data[148:], dt).reshape(oh, ow, 4)
    assert np.array_equal(px.view(np.uint8), view.contiguous().cpu().numpy().view(np.uint8))
    assert A.library().ovrfsr_save_dds(None, path.encode(), None) == 1


# ------------------------------------------------------------------------------------------------
# round 6: the DOMAIN of texel values the parity statements cover (header, "Texel values")
# ------------------------------------------------------------------------------------------------
_wild = synth.wild_f32   # the families live beside the other content generators


@pytest.mark.parametrize("kind", synth.WILD_KINDS)
def test_texel_value_domain(gpu, kind):
    """What the bit-identity of the strict build covers, probed with RGBA32F texels no colour image holds (header, "Texel values"):
      * every finite value whose fp32 products do not overflow -- the extremes of the half range, negative values, fp32 denormals, 1e18: bit for bit;
      * zeros of BOTH signs: IEEE 754 leaves min / max of a +0 and a -0 open and x86 (the oracle) and gfx950 choose differently, so a result that is
        a zero may carry the other sign -- and nothing else differs;
      * NaN / Inf texels and magnitudes whose products overflow (1e30): outside the contract -- but the same pixels are NaN in every build and in the
        oracle, the finite ones stay finite, and nothing hangs (memory safety: tools/debug/bounds_campaign.py runs these families)."""
    import torch
    import openvr_fsr_amd as A
    iw, ih, ow, oh = 150, 110, 200, 147
    centre, rad = O.mask_constants(ow, oh, 2.0)
    con = O.easu_con(iw, ih, ow, oh)
    for seed in range(4):
        img = _wild(kind, iw, ih, np.random.default_rng(50 + seed))
        t = torch.from_numpy(img).cuda()
        we = O.easu(img, ow, oh, con, centre, rad)
        wr = O.rcas(we, O.rcas_con(0.8, 0), centre, rad)
        for stage, want, kw in (("easu", we, dict(stage_mask=1)), ("easu+rcas", wr, dict(quantize_intermediate=0, fused=0))):
            for prec in (STRICT, FP32):
                pp = A.PostProcessor(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.8, radius=2.0, precision=prec, **kw)
                out = torch.zeros((oh, ow, 4), dtype=torch.float32, device="cuda")
                pp.apply_batch(t[None], out[None])
                torch.cuda.synchronize()
                pp.close()
                got, w3 = out.cpu().numpy()[..., :3], want[..., :3]
                if kind == "NaN / Inf / 1e30":
                    assert np.array_equal(np.isnan(got), np.isnan(w3)), (kind, stage, prec, seed)
                    continue
                assert np.isfinite(got).all()
                if prec != STRICT:
                    continue        # (the product build's tolerances are stated for colour content: tests/test_gpu_parity*.py)
                same = got.view(np.uint32) == w3.view(np.uint32)
                if kind == "zeros of both signs":
                    assert (same | ((got == 0) & (w3 == 0))).all(), (kind, stage, seed, int((~same).sum()))
                else:
                    assert same.all(), (kind, stage, seed, int((~same).sum()))
