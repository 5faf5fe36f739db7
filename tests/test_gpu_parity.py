"""GPU parity: the HIP path (through the C ABI) against the CPU oracle on identical inputs.

Tolerances (stated, then asserted):
  * FP32_STRICT build: BIT-EXACT -- float outputs compare equal as uint32 words, UNORM8 outputs as bytes.
  * FP32 product build (FMA contraction, v_rcp_f32, colours accumulated in the 0..255 byte domain):
      float outputs  max-abs <= 2e-5   (north_star allows 1e-3)
      UNORM8 output of the EASU pass: bit-identical (the near-tie guard re-resolves, in the reference's operator order,
      every pixel whose result lies within 2^-9 byte of a rounding boundary);
      UNORM8 outputs of every other single pass and of EASU -> UNORM8 -> RCAS <= 1 LSB, and at most 0.1 % of the
      channel values differ at all.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import synth
from tests.util import run_gpu, lsb_stats

pytestmark = pytest.mark.gpu

STRICT = 2
FP32 = 0

SHAPES = [
    # inW, inH, outW, outH, generator
    (96, 80, 128, 107, synth.structured_u8),     # ragged: 107 = 6*16+11
    (61, 47, 80, 63, synth.random_u8),           # odd everything
    (64, 64, 83, 83, synth.extremes_u8),         # 0/255 content: RCAS 0*inf paths, EASU zero-gradient guard
    (33, 17, 64, 33, synth.random_u8),           # ~2x, one tile tall + 1 row
    (200, 120, 260, 156, synth.structured_u8),   # renderScale 1.3 style ratio (not a rational 3/4)
    (16, 16, 17, 17, synth.random_u8),           # tiny: every tap clamps somewhere
    (100, 80, 105, 84, synth.structured_u8),     # scale 0.95: LDS pitch 40 instantiation of the product kernel
    (120, 100, 100, 84, synth.random_u8),        # scale 1.2 (minification): generic runtime-pitch kernel
]



def _consts(iw, ih, ow, oh, radius, proj, eye):
    centre, rad = O.mask_constants(ow, oh, radius, proj, True, eye)
    return O.easu_con(iw, ih, ow, oh), centre, rad


def _oracle_easu(img8, ow, oh, radius=2.0, proj=(0.5, 0.5, 0.5, 0.5), eye=0):
    ih, iw = img8.shape[:2]
    con, centre, rad = _consts(iw, ih, ow, oh, radius, proj, eye)
    return O.easu(O.unorm8_to_float(img8), ow, oh, con, centre, rad)


def _oracle_rcas(img8, sharpness=0.9, radius=2.0, proj=(0.5, 0.5, 0.5, 0.5), eye=0, debug=0):
    h, w = img8.shape[:2]
    centre, rad = O.mask_constants(w, h, radius, proj, True, eye)
    return O.rcas(O.unorm8_to_float(img8), O.rcas_con(sharpness, debug), centre, rad)


# ------------------------------------------------------------------------------------------------
# strict build: bit-exact
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iw,ih,ow,oh,gen", SHAPES)
def test_easu_strict_bit_exact(gpu, iw, ih, ow, oh, gen):
    img8 = gen(iw, ih, 7)
    want = _oracle_easu(img8, ow, oh)
    got = run_gpu(img8, ow, oh, np.float32, precision=STRICT, stage_mask=1)
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "max abs diff %g" % np.abs(got - want).max()


@pytest.mark.parametrize("w,h,gen", [(128, 107, synth.structured_u8), (83, 83, synth.extremes_u8), (17, 40, synth.random_u8)])
def test_rcas_strict_bit_exact(gpu, w, h, gen):
    img8 = gen(w, h, 11)
    want = _oracle_rcas(img8, 0.9)
    got = run_gpu(img8, w, h, np.float32, precision=STRICT, render_scale=1.0, sharpness=0.9)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "max abs diff %g" % np.nanmax(np.abs(got - want))


@pytest.mark.parametrize("iw,ih,ow,oh,gen", SHAPES)
@pytest.mark.parametrize("quant", [1, 0])
def test_pipeline_strict_bit_exact(gpu, iw, ih, ow, oh, gen, quant):
    img8 = gen(iw, ih, 3)
    want8, wantf = O.fsr_pipeline_u8(img8, ow, oh, sharpness=0.9, quantize_intermediate=bool(quant), want_float=True)
    got8 = run_gpu(img8, ow, oh, np.uint8, precision=STRICT, sharpness=0.9, quantize_intermediate=quant, fused=0)
    gotf = run_gpu(img8, ow, oh, np.float32, precision=STRICT, sharpness=0.9, quantize_intermediate=quant, fused=0)
    assert np.array_equal(got8, want8)
    assert np.array_equal(gotf.view(np.uint32), wantf.view(np.uint32))


@pytest.mark.parametrize("radius,proj,eye,debug", [(0.5, (0.5, 0.5, 0.5, 0.5), 0, 0), (0.6, (0.42, 0.55, 0.61, 0.47), 1, 1),
                                                   (0.2, (0.9, 0.1, 0.1, 0.9), 0, 1)])
def test_masked_pipeline_strict_bit_exact(gpu, radius, proj, eye, debug):
    iw, ih, ow, oh = 150, 120, 200, 160
    img8 = synth.structured_u8(iw, ih, 5)
    want8 = O.fsr_pipeline_u8(img8, ow, oh, sharpness=0.7, radius=radius, proj=proj, eye=eye, debug=debug)
    got8 = run_gpu(img8, ow, oh, np.uint8, eye=eye, precision=STRICT, sharpness=0.7, radius=radius, proj_centre=proj,
                   debug_mode=debug, fused=0)
    assert np.array_equal(got8, want8)


# ------------------------------------------------------------------------------------------------
# product (FP32) build: stated tolerances
# ------------------------------------------------------------------------------------------------
FLOAT_TOL = 2e-5
LSB_FRACTION = 1e-3
RCAS_LSB = 1   # UNORM8 outputs within 1 LSB (rounds 1-2: 5, flipped ties of the 8-bit intermediate x RCAS gain 4)
NIS_FLOAT_TOL = 1e-3   # north_star's max-abs; measured values are recorded by tests/test_gpu_parity_report.py


@pytest.mark.parametrize("iw,ih,ow,oh,gen", SHAPES)
def test_easu_fp32_tolerance(gpu, iw, ih, ow, oh, gen):
    img8 = gen(iw, ih, 7)
    want = _oracle_easu(img8, ow, oh)
    got = run_gpu(img8, ow, oh, np.float32, precision=FP32, stage_mask=1)
    err = np.abs(got - want).max()
    assert err <= FLOAT_TOL, err
    got8 = run_gpu(img8, ow, oh, np.uint8, precision=FP32, stage_mask=1)
    assert np.array_equal(got8, O.float_to_unorm8(want)), lsb_stats(got8, O.float_to_unorm8(want))  # near-tie guard


@pytest.mark.parametrize("iw,ih,ow,oh,gen", SHAPES)
def test_pipeline_fp32_tolerance(gpu, iw, ih, ow, oh, gen):
    img8 = gen(iw, ih, 3)
    want8, wantf = O.fsr_pipeline_u8(img8, ow, oh, sharpness=0.9, quantize_intermediate=False, want_float=True)
    gotf = run_gpu(img8, ow, oh, np.float32, precision=FP32, sharpness=0.9, quantize_intermediate=0, fused=0)
    err = np.nanmax(np.abs(gotf - wantf))
    assert err <= 1e-4, err   # RCAS divides by local contrast: EASU's 2e-5 can grow a few x
    # reference-faithful (8-bit intermediate): the intermediate is the oracle's (near-tie guard), RCAS adds <= 1 LSB
    want8q = O.fsr_pipeline_u8(img8, ow, oh, sharpness=0.9, quantize_intermediate=True)
    got8q = run_gpu(img8, ow, oh, np.uint8, precision=FP32, sharpness=0.9, quantize_intermediate=1, fused=0)
    mx, frac = lsb_stats(got8q, want8q)
    assert mx <= RCAS_LSB and frac <= LSB_FRACTION, (mx, frac)


def test_batch_matches_single(gpu):
    import torch
    import openvr_fsr_amd as A
    iw, ih, ow, oh = 96, 80, 128, 107
    imgs = np.stack([synth.structured_u8(iw, ih, synth.seed_for(p, e)) for p in range(3) for e in range(2)])
    proj = (0.4, 0.5, 0.6, 0.5)
    pp = A.PostProcessor(fsr_enabled=1, out_width=ow, out_height=oh, radius=0.6, sharpness=0.9, proj_centre=proj, fused=0)
    t = torch.from_numpy(imgs).cuda()
    outs = torch.empty((6, oh, ow, 4), dtype=torch.uint8, device="cuda")
    pp.apply_batch(t, outs, first_eye=0, alternate_eyes=True)
    torch.cuda.synchronize()
    got = outs.cpu().numpy()
    for i in range(6):
        single = run_gpu(imgs[i], ow, oh, np.uint8, eye=i & 1, radius=0.6, sharpness=0.9, proj_centre=proj, fused=0)
        assert np.array_equal(got[i], single), i
        want = O.fsr_pipeline_u8(imgs[i], ow, oh, sharpness=0.9, radius=0.6, proj=proj, eye=i & 1)
        mx, frac = lsb_stats(got[i], want)
        assert mx <= RCAS_LSB and frac <= LSB_FRACTION, (i, mx, frac)


# ------------------------------------------------------------------------------------------------
# NIS (NVScaler, NVSharpen)
# ------------------------------------------------------------------------------------------------
def _nis_oracle_upscale(img8, ow, oh, sharpness, radius=2.0, proj=(0.5, 0.5, 0.5, 0.5), eye=0, debug=0):
    import openvr_fsr_amd as A
    ih, iw = img8.shape[:2]
    cs, cu = A.nis_coefs()
    ok, cfg = A.nis_scaler_config(sharpness, iw, ih, ow, oh)
    assert ok
    centre, rad = O.mask_constants(ow, oh, radius, proj, True, eye)
    return O.nis_upscale(O.unorm8_to_float(img8), ow, oh, O.nis_block(cfg, centre, rad, debug), cs, cu)


def _nis_oracle_sharpen(img8, sharpness, radius=2.0, proj=(0.5, 0.5, 0.5, 0.5), eye=0, debug=0):
    import openvr_fsr_amd as A
    h, w = img8.shape[:2]
    ok, cfg = A.nis_sharpen_config(sharpness, w, h)
    centre, rad = O.mask_constants(w, h, radius, proj, True, eye)
    return O.nis_sharpen(O.unorm8_to_float(img8), O.nis_block(cfg, centre, rad, debug))


NIS_SHAPES = [(96, 80, 128, 107, synth.structured_u8), (61, 47, 80, 63, synth.random_u8), (64, 64, 83, 83, synth.extremes_u8),
              (50, 40, 100, 80, synth.structured_u8), (40, 33, 41, 34, synth.random_u8), (200, 120, 260, 156, synth.structured_u8)]


@pytest.mark.parametrize("iw,ih,ow,oh,gen", NIS_SHAPES)
def test_nis_scaler_strict_bit_exact(gpu, iw, ih, ow, oh, gen):
    img8 = gen(iw, ih, 21)
    want = _nis_oracle_upscale(img8, ow, oh, 0.9)
    got = run_gpu(img8, ow, oh, np.float32, precision=STRICT, use_nis=1, sharpness=0.9)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "max abs diff %g" % np.abs(got - want).max()
    got8 = run_gpu(img8, ow, oh, np.uint8, precision=STRICT, use_nis=1, sharpness=0.9)
    assert np.array_equal(got8, O.float_to_unorm8(want))


@pytest.mark.parametrize("radius,proj,eye,debug,sharp", [(0.5, (0.5, 0.5, 0.5, 0.5), 0, 0, 0.5), (0.7, (0.42, 0.55, 0.61, 0.47), 1, 1, 0.2)])
def test_nis_scaler_masked_strict_bit_exact(gpu, radius, proj, eye, debug, sharp):
    iw, ih, ow, oh = 150, 120, 200, 160
    img8 = synth.structured_u8(iw, ih, 5)
    want = _nis_oracle_upscale(img8, ow, oh, sharp, radius, proj, eye, debug)
    got = run_gpu(img8, ow, oh, np.float32, eye=eye, precision=STRICT, use_nis=1, sharpness=sharp, radius=radius,
                  proj_centre=proj, debug_mode=debug)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "max abs diff %g" % np.abs(got - want).max()


@pytest.mark.parametrize("w,h,gen,radius,debug", [(128, 107, synth.structured_u8, 2.0, 0), (83, 83, synth.extremes_u8, 0.6, 1),
                                                   (33, 70, synth.random_u8, 2.0, 0)])
def test_nis_sharpen_strict_bit_exact(gpu, w, h, gen, radius, debug):
    img8 = gen(w, h, 31)
    want = _nis_oracle_sharpen(img8, 0.75, radius, debug=debug)
    got = run_gpu(img8, w, h, np.float32, precision=STRICT, use_nis=1, render_scale=1.0, sharpness=0.75, radius=radius,
                  debug_mode=debug)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "max abs diff %g" % np.abs(got - want).max()


@pytest.mark.parametrize("w,h,gen,radius,debug", [(128, 107, synth.structured_u8, 2.0, 0), (83, 83, synth.extremes_u8, 0.6, 1),
                                                   (200, 150, synth.random_u8, 2.0, 0)])
def test_nis_sharpen_fp32_tolerance(gpu, w, h, gen, radius, debug):
    """NVSharpen, product build: exact wave-uniform skips of zero-weight directional terms + contraction.  The luma that feeds
    GetEdgeMap's thresholds is evaluated unfused in every build (nis_getY), so no edge decision can flip: north_star's
    max-abs 1e-3 on float outputs, <= 1 LSB on UNORM8 outputs."""
    img8 = gen(w, h, 31)
    want = _nis_oracle_sharpen(img8, 0.75, radius, debug=debug)
    got = run_gpu(img8, w, h, np.float32, precision=FP32, use_nis=1, render_scale=1.0, sharpness=0.75, radius=radius, debug_mode=debug)
    err = np.abs(got - want)
    assert err.max() <= NIS_FLOAT_TOL, float(err.max())
    got8 = run_gpu(img8, w, h, np.uint8, precision=FP32, use_nis=1, render_scale=1.0, sharpness=0.75, radius=radius, debug_mode=debug)
    d = np.abs(got8.astype(np.int16) - O.float_to_unorm8(want).astype(np.int16))
    assert d.max() <= 1, int(d.max())


@pytest.mark.parametrize("iw,ih,ow,oh,gen", NIS_SHAPES)
def test_nis_scaler_fp32_tolerance(gpu, iw, ih, ow, oh, gen):
    # NIS is full of hard thresholds (GetEdgeMap, phase quantisation).  Everything that feeds one -- the luma, the
    # source positions -- is evaluated unfused in the product build too, so none can flip; what remains is rounding
    # noise of the contracted filters: north_star's max-abs 1e-3 on float outputs, <= 1 LSB on UNORM8 outputs.
    img8 = gen(iw, ih, 21)
    want = _nis_oracle_upscale(img8, ow, oh, 0.9)
    got = run_gpu(img8, ow, oh, np.float32, precision=FP32, use_nis=1, sharpness=0.9)
    err = np.abs(got - want)
    assert err.max() <= NIS_FLOAT_TOL, float(err.max())
    got8 = run_gpu(img8, ow, oh, np.uint8, precision=FP32, use_nis=1, sharpness=0.9)
    d = np.abs(got8.astype(np.int16) - O.float_to_unorm8(want).astype(np.int16))
    assert d.max() <= 1, int(d.max())


@pytest.mark.parametrize("debug", [0, 1])
def test_masked_sorted_two_pass_float_out(gpu, debug):
    """auto policy on a masked RGBA8 pipeline = EASU and RCAS on the tile list touching the radius, ring tiles'
    intermediate, outside tiles in final form; here with a float32 destination (generic outside kernel) and the debug
    tint, against the oracle's un-rounded final values."""
    iw, ih, ow, oh = 330, 250, 440, 333
    img8 = synth.structured_u8(iw, ih, 91)
    proj = (0.45, 0.5, 0.55, 0.5)
    _, wantf = O.fsr_pipeline_u8(img8, ow, oh, sharpness=0.7, radius=0.55, proj=proj, eye=1, debug=debug, want_float=True)
    got = run_gpu(img8, ow, oh, np.float32, eye=1, precision=FP32, sharpness=0.7, radius=0.55, proj_centre=proj, debug_mode=debug)
    err = np.abs(got - wantf)
    # a 1-LSB flip of the UNORM8 intermediate (rare, see test_pipeline_fp32_tolerance) is amplified up to 4x by RCAS
    assert (err <= 1e-4).mean() >= 0.999 and err.max() <= RCAS_LSB / 255.0, (float((err <= 1e-4).mean()), float(err.max()))
    got8 = run_gpu(img8, ow, oh, np.uint8, eye=1, precision=FP32, sharpness=0.7, radius=0.55, proj_centre=proj, debug_mode=debug)
    same = run_gpu(img8, ow, oh, np.uint8, eye=1, precision=FP32, sharpness=0.7, radius=0.55, proj_centre=proj, debug_mode=debug, fused=0)
    assert np.array_equal(got8, same)   # sorted two-pass == plain two-pass with the same kernels


@pytest.mark.parametrize("radius,proj,debug", [(0.5, (0.5, 0.5, 0.5, 0.5), 0), (0.62, (0.42, 0.55, 0.61, 0.47), 1), (0.05, (0.5,) * 4, 0)])
def test_nis_scaler_masked_product_lists(gpu, radius, proj, debug):
    """Product build with a radius: mask-sorted group lists, LDS-free DirectCopy kernel on the auxiliary stream, and a
    batch whose eyes have different centres.  Outside groups must be bit-identical to the strict build (DirectCopy has
    no contraction-sensitive thresholds left after mad_unfused), inside groups within the NIS product tolerance."""
    import torch
    import openvr_fsr_amd as A
    iw, ih, ow, oh = 300, 240, 400, 320
    imgs = np.stack([synth.structured_u8(iw, ih, 80 + i) for i in range(4)])
    pp = A.PostProcessor(fsr_enabled=1, use_nis=1, out_width=ow, out_height=oh, sharpness=0.6, radius=radius,
                         proj_centre=proj, debug_mode=debug, precision=FP32)
    outs = torch.empty((4, oh, ow, 4), dtype=torch.float32, device="cuda")
    pp.apply_batch(torch.from_numpy(imgs).cuda(), outs, first_eye=1, alternate_eyes=True)
    torch.cuda.synchronize()
    got = outs.cpu().numpy()
    pp.close()
    for i in range(4):
        want = _nis_oracle_upscale(imgs[i], ow, oh, 0.6, radius, proj, 1 ^ (i & 1), debug)
        err = np.abs(got[i] - want)
        assert err.max() <= NIS_FLOAT_TOL, (i, float(err.max()))
    one = run_gpu(imgs[0], ow, oh, np.float32, eye=1, precision=FP32, use_nis=1, sharpness=0.6, radius=radius,
                  proj_centre=proj, debug_mode=debug)
    assert np.array_equal(one, got[0])


def test_nis_rejects_out_of_range_scale(gpu):
    import openvr_fsr_amd as A
    with pytest.raises(A.OvrFsrError):
        run_gpu(synth.random_u8(40, 40, 1), 100, 100, np.uint8, use_nis=1)   # scale 0.4: NVScalerUpdateConfig -> false


# ------------------------------------------------------------------------------------------------
# BASELINE.json's full sizes
# ------------------------------------------------------------------------------------------------
def test_c1_c2_full_size_strict_bit_exact(gpu):
    """C1 (EASU only, left eye) and C2 (EASU+RCAS) at 1683x1869 -> 2244x2492, bit-exact in the strict build."""
    iw, ih, ow, oh = 1683, 1869, 2244, 2492
    img8 = synth.structured_u8(iw, ih, synth.seed_for(0, 0))
    want_e = O.easu(O.unorm8_to_float(img8), ow, oh)
    got_e = run_gpu(img8, ow, oh, np.float32, precision=STRICT, stage_mask=1)
    assert np.array_equal(got_e.view(np.uint32), want_e.view(np.uint32))
    want8 = O.fsr_pipeline_u8(img8, ow, oh, sharpness=0.9)
    got8 = run_gpu(img8, ow, oh, np.uint8, precision=STRICT, sharpness=0.9)
    assert np.array_equal(got8, want8)
    # product build at full size: stated tolerances
    got_f = run_gpu(img8, ow, oh, np.float32, precision=FP32, stage_mask=1)
    assert np.abs(got_f - want_e).max() <= FLOAT_TOL
    got8p = run_gpu(img8, ow, oh, np.uint8, precision=FP32, sharpness=0.9)
    mx, frac = lsb_stats(got8p, want8)
    assert mx <= RCAS_LSB and frac <= LSB_FRACTION, (mx, frac)


def test_c3_full_size_nis(gpu):
    iw, ih, ow, oh = 1683, 1869, 2244, 2492
    img8 = synth.structured_u8(iw, ih, synth.seed_for(0, 1))
    want = _nis_oracle_upscale(img8, ow, oh, 0.9)
    got = run_gpu(img8, ow, oh, np.float32, eye=1, precision=STRICT, use_nis=1, sharpness=0.9)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    got = run_gpu(img8, ow, oh, np.float32, eye=1, precision=FP32, use_nis=1, sharpness=0.9)
    err = np.abs(got - want)
    assert err.max() <= NIS_FLOAT_TOL, float(err.max())


def test_c2_c3_full_size_shipped_radius(gpu):
    """C2 / C3 shapes with the reference's shipped radius 0.5 (openvr_mod.cfg), product build, auto policy: mask-sorted
    two-pass (FSR) / group lists (NIS) with the LDS-staged outside kernel on the auxiliary stream.  Pixels of mask groups
    outside the radius are bit-identical to the oracle, the frame meets the unmasked bounds."""
    from tests.test_gpu_fuzz import _outside_px
    iw, ih, ow, oh = 1683, 1869, 2244, 2492
    img8 = synth.structured_u8(iw, ih, synth.seed_for(1, 0))
    centre, rad = O.mask_constants(ow, oh, 0.5)
    want8 = O.fsr_pipeline_u8(img8, ow, oh, sharpness=0.9, radius=0.5)
    got8 = run_gpu(img8, ow, oh, np.uint8, precision=FP32, sharpness=0.9, radius=0.5)
    outside = _outside_px(ow, oh, centre, rad[1], 16, 16)
    assert 0.7 < outside.mean() < 0.85
    assert np.array_equal(got8[outside], want8[outside])
    mx, frac = lsb_stats(got8, want8)
    assert mx <= RCAS_LSB and frac <= LSB_FRACTION, (mx, frac)
    import openvr_fsr_amd as A
    cs, cu = A.nis_coefs()
    ok, cfg = A.nis_scaler_config(0.9, iw, ih, ow, oh)
    wantn = O.float_to_unorm8(O.nis_upscale(O.unorm8_to_float(img8), ow, oh, O.nis_block(cfg, centre, rad, 0), cs, cu))
    gotn = run_gpu(img8, ow, oh, np.uint8, precision=FP32, use_nis=1, sharpness=0.9, radius=0.5)
    outside = _outside_px(ow, oh, centre, rad[1], 32, 24)
    assert np.array_equal(gotn[outside], wantn[outside])
    d = np.abs(gotn.astype(np.int16) - wantn.astype(np.int16))
    assert d.max() <= 1, int(d.max())


def test_c4_c5_shapes_properties(gpu):
    """C4 (2244x2492 -> 2916x3240) and C5 (radius-masked 3160x3160, RGBA16F I/O): size-independent properties."""
    import torch
    import openvr_fsr_amd as A
    # constant image is a fixed point of EASU+RCAS away from the border (border taps of RCAS read 0)
    for (iw, ih, ow, oh, dt, radius) in [(2244, 2492, 2916, 3240, torch.uint8, 2.0), (2370, 2370, 3160, 3160, torch.float16, 0.5)]:
        const = torch.empty((ih, iw, 4), dtype=dt, device="cuda")
        if dt == torch.uint8:
            const[...] = torch.tensor([64, 128, 191, 255], dtype=dt, device="cuda")
        else:
            const[...] = torch.tensor([0.25, 0.5, 0.75, 1.0], dtype=dt, device="cuda")
        pp = A.PostProcessor(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, radius=radius)
        out = pp.apply(0, const, out_dtype=dt)
        torch.cuda.synchronize()
        inner = out[2:-2, 2:-2].float()
        ref = const[0, 0].float()
        tol = 1.0 if dt == torch.uint8 else 2e-3
        assert (inner - ref).abs().max().item() <= tol
        assert out.shape == (oh, ow, 4)
        pp.close()
    # C5 against the oracle on a half-float image: unit-domain path, masked, RGBA16F in and out
    iw, ih, ow, oh = 2370, 2370, 3160, 3160
    img8 = synth.structured_u8(iw, ih, 77)
    imgh = (img8.astype(np.float32) / 255.0).astype(np.float16)
    centre, rad = O.mask_constants(ow, oh, 0.5)
    e = O.easu(imgh.astype(np.float32), ow, oh, O.easu_con(iw, ih, ow, oh), centre, rad)
    e16 = e.astype(np.float16).astype(np.float32)                       # half-float intermediate texture
    want = O.rcas(e16, O.rcas_con(0.9), centre, rad)
    got = run_gpu(imgh, ow, oh, np.float16, precision=STRICT, sharpness=0.9, radius=0.5)
    assert np.array_equal(got, want.astype(np.float16))
    got = run_gpu(imgh, ow, oh, np.float16, precision=FP32, sharpness=0.9, radius=0.5).astype(np.float32)
    err = np.abs(got - want.astype(np.float16).astype(np.float32))
    # the contract (north_star): max-abs <= 1e-3 on every value, none above -- one half-ulp in [1, 2) is 9.77e-4, the largest a unit-range
    # half output can be off by when its intermediate is the strict build's (near-tie guard)
    assert err.max() <= 1e-3, (float(err.max()), int((err > 1e-3).sum()))


# ------------------------------------------------------------------------------------------------
# one side-by-side texture holding both eyes (PostProcessor.cpp:146,155-158,298-301)
# ------------------------------------------------------------------------------------------------
def test_shared_side_by_side_texture(gpu):
    import torch
    import openvr_fsr_amd as A
    iw, ih, ow, oh = 240, 100, 320, 133          # both eyes in one 240-wide texture
    proj = (0.42, 0.55, 0.61, 0.47)
    img8 = synth.structured_u8(iw, ih, 9)
    want = O.fsr_pipeline_u8(img8, ow, oh, sharpness=0.8, radius=0.7, proj=proj, one_eye_per_texture=False, eye=0, debug=1)
    pp = A.PostProcessor(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.8, radius=0.7, proj_centre=proj,
                         debug_mode=1, precision=STRICT)
    tex = torch.from_numpy(img8).cuda()
    left = A.Bounds(0.0, 0.0, 0.5, 1.0)           # |uMax-uMin| <= 0.5 -> texture contains both eyes
    right = A.Bounds(0.5, 0.0, 1.0, 1.0)
    out_l = pp.apply(A.EYE_LEFT, tex, bounds=left)
    torch.cuda.synchronize()
    got_l = out_l.cpu().numpy().copy()
    # poison the ctx-owned output: the second Submit of the same texture must NOT re-run the kernels (:155-158)
    out_l.fill_(7)
    out_r = pp.apply(A.EYE_RIGHT, tex, bounds=right)
    torch.cuda.synchronize()
    assert out_r.data_ptr() == out_l.data_ptr()
    assert (out_r.cpu().numpy() == 7).all()
    assert np.array_equal(got_l, want)
    # next frame (eyeCount wrapped to 0): processed again
    out_l2 = pp.apply(A.EYE_LEFT, tex, bounds=left)
    torch.cuda.synchronize()
    assert np.array_equal(out_l2.cpu().numpy(), want)
    # a size change rebuilds everything (PostProcessor.cpp:136-143)
    img2 = synth.structured_u8(120, 100, 10)
    pp2_want = O.fsr_pipeline_u8(img2, ow, oh, sharpness=0.8, radius=0.7, proj=proj, one_eye_per_texture=True, eye=1, debug=1)
    out2 = pp.apply(A.EYE_RIGHT, torch.from_numpy(img2).cuda())   # default bounds -> one eye per texture
    torch.cuda.synchronize()
    assert np.array_equal(out2.cpu().numpy(), pp2_want)
    pp.close()


def test_shared_texture_batch(gpu):
    """ovrfsr_apply_batch_shared: n side-by-side textures (both eyes each) in one launch == the oracle's shared-texture pipeline
    per image, strict bit-exact and product within 1 LSB, masked (two centres per image) and with a tile list."""
    import torch
    import openvr_fsr_amd as A
    iw, ih, ow, oh = 240, 100, 320, 133
    proj = (0.42, 0.55, 0.61, 0.47)
    imgs = np.stack([synth.structured_u8(iw, ih, 20 + i) for i in range(3)])
    want = [O.fsr_pipeline_u8(imgs[i], ow, oh, sharpness=0.8, radius=0.7, proj=proj, one_eye_per_texture=False, eye=0) for i in range(3)]
    for prec in (STRICT, FP32):
        pp = A.PostProcessor(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.8, radius=0.7, proj_centre=proj, precision=prec)
        t = torch.from_numpy(imgs).cuda()
        outs = torch.empty((3, oh, ow, 4), dtype=torch.uint8, device="cuda")
        pp.apply_batch(t, outs, shared=True)
        torch.cuda.synchronize()
        got = outs.cpu().numpy()
        for i in range(3):
            if prec == STRICT:
                assert np.array_equal(got[i], want[i]), i
            else:
                mx, frac = lsb_stats(got[i], want[i])
                assert mx <= RCAS_LSB and frac <= LSB_FRACTION, (i, mx, frac)
        # the one-eye-per-texture batch form on the same ctx afterwards: the ctx rebuilds its mask constants
        single = torch.empty((1, oh, ow, 4), dtype=torch.uint8, device="cuda")
        pp.apply_batch(t[:1], single, first_eye=A.EYE_RIGHT, alternate_eyes=False)
        torch.cuda.synchronize()
        w1 = O.fsr_pipeline_u8(imgs[0], ow, oh, sharpness=0.8, radius=0.7, proj=proj, one_eye_per_texture=True, eye=1)
        mx, frac = lsb_stats(single.cpu().numpy()[0], w1)
        assert mx <= (0 if prec == STRICT else RCAS_LSB), (mx, frac)
        pp.close()


def test_disabled_and_reset_behaviour(gpu):
    import torch
    import openvr_fsr_amd as A
    t = torch.from_numpy(synth.random_u8(40, 30, 1)).cuda()
    pp = A.PostProcessor(fsr_enabled=0)
    assert pp.apply(0, t).data_ptr() == t.data_ptr()           # fsr disabled: texture forwarded untouched (:135)
    pp.close()
    pp = A.PostProcessor(fsr_enabled=1, use_nis=1, out_width=100, out_height=75)   # NIS cannot do 2.5x -> ctx disables itself
    with pytest.raises(A.OvrFsrError) as e1:
        pp.apply(0, t, out_dtype=torch.uint8)
    assert e1.value.status == 2
    with pytest.raises(A.OvrFsrError) as e2:
        pp.apply(0, t, out_dtype=torch.uint8)
    assert e2.value.status == 5                                 # OVRFSR_ERR_DISABLED until reset (:148-151)
    pp.reset()
    pp.set_config(A.Config.default(fsr_enabled=1, out_width=53, out_height=40, sharpness=0.9, radius=2.0))
    out = pp.apply(0, t, out_dtype=torch.uint8)
    torch.cuda.synchronize()
    mx, frac = lsb_stats(out.cpu().numpy(), O.fsr_pipeline_u8(t.cpu().numpy(), 53, 40, sharpness=0.9))
    assert mx <= RCAS_LSB and frac <= 5e-3, (mx, frac)
    pp.close()


def test_in_place_apply_is_rejected(gpu):
    """RCAS / NVSharpen read neighbour texels that other workgroups write: an output overlapping the input is refused by
    ovrfsr_apply (sharpen-only, where the sizes agree and the mistake is plausible) exactly as by ovrfsr_apply_batch."""
    import torch
    import openvr_fsr_amd as A
    t = torch.from_numpy(synth.random_u8(64, 48, 5)).cuda()
    for nis in (0, 1):
        pp = A.PostProcessor(fsr_enabled=1, use_nis=nis, render_scale=1.0, sharpness=0.9, radius=2.0)
        with pytest.raises(A.OvrFsrError) as e:
            pp.apply(0, t, out=t)
        assert e.value.status == 1   # OVRFSR_ERR_INVALID_ARGUMENT
        out = torch.empty_like(t)
        pp.apply(0, t, out=out)      # the ctx is still usable
        torch.cuda.synchronize()
        # the same race through the ctx-owned output: chaining the previous ctx-owned result back in as `in` with out = NULL
        own = pp.apply(0, t)         # ctx-owned destination
        torch.cuda.synchronize()
        with pytest.raises(A.OvrFsrError) as e:
            pp.apply(0, own)         # would sharpen the ctx-owned image in place
        assert e.value.status == 1
        pp.close()


# ------------------------------------------------------------------------------------------------
# fused EASU -> RCAS (intermediate in LDS) == the two-kernel path, bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [STRICT, FP32])
@pytest.mark.parametrize("iw,ih,ow,oh,gen", SHAPES)
def test_fused_equals_two_pass(gpu, prec, iw, ih, ow, oh, gen):
    if ow < iw and prec == FP32:
        pytest.skip("minification: the product-build fused kernel only exists for the fixed-pitch (upscaling) footprints")
    img8 = gen(iw, ih, 3)
    for quant, dt in [(1, np.uint8), (0, np.float32)]:
        two = run_gpu(img8, ow, oh, dt, precision=prec, sharpness=0.9, quantize_intermediate=quant, fused=0)
        one = run_gpu(img8, ow, oh, dt, precision=prec, sharpness=0.9, quantize_intermediate=quant, fused=1)
        if prec == STRICT:
            assert np.array_equal(one.view(np.uint8), two.view(np.uint8)), quant
        else:
            # product build: the two paths run differently scheduled (differently contracted) RCAS code; the EASU
            # stage and the intermediate rounding are the same, so they agree to fp32 rounding noise
            d = np.abs(one.astype(np.float32) - two.astype(np.float32))
            if dt == np.uint8:
                assert d.max() <= 1 and (d > 0).mean() <= 1e-3, (quant, float(d.max()), float((d > 0).mean()))
            else:
                assert d.max() <= 2e-6, (quant, float(d.max()))
    if prec == STRICT:
        want8 = O.fsr_pipeline_u8(img8, ow, oh, sharpness=0.9)
        assert np.array_equal(run_gpu(img8, ow, oh, np.uint8, precision=STRICT, sharpness=0.9, fused=1), want8)


@pytest.mark.parametrize("radius,proj,eye,debug", [(0.5, (0.5, 0.5, 0.5, 0.5), 0, 0), (0.6, (0.42, 0.55, 0.61, 0.47), 1, 1),
                                                   (0.2, (0.9, 0.1, 0.1, 0.9), 0, 1)])
def test_fused_masked_strict_bit_exact(gpu, radius, proj, eye, debug):
    iw, ih, ow, oh = 150, 120, 200, 160
    img8 = synth.structured_u8(iw, ih, 5)
    want8 = O.fsr_pipeline_u8(img8, ow, oh, sharpness=0.7, radius=radius, proj=proj, eye=eye, debug=debug)
    got8 = run_gpu(img8, ow, oh, np.uint8, eye=eye, precision=STRICT, sharpness=0.7, radius=radius, proj_centre=proj,
                   debug_mode=debug, fused=1)
    assert np.array_equal(got8, want8)


def test_fused_half_float_and_full_size(gpu):
    iw, ih, ow, oh = 237, 237, 316, 316
    imgh = (synth.structured_u8(iw, ih, 77).astype(np.float32) / 255.0).astype(np.float16)
    two = run_gpu(imgh, ow, oh, np.float16, precision=STRICT, sharpness=0.9, radius=0.5, fused=0)
    one = run_gpu(imgh, ow, oh, np.float16, precision=STRICT, sharpness=0.9, radius=0.5, fused=1)
    assert np.array_equal(one.view(np.uint16), two.view(np.uint16))
    # product build: both forms guard the half intermediate's near-ties (near_tie_half3), so what is left between them is
    # the final half rounding of RCAS's output
    two = run_gpu(imgh, ow, oh, np.float16, precision=FP32, sharpness=0.9, radius=0.5, fused=0).astype(np.float32)
    one = run_gpu(imgh, ow, oh, np.float16, precision=FP32, sharpness=0.9, radius=0.5, fused=1).astype(np.float32)
    d = np.abs(one - two)
    assert d.max() <= 1e-3 and (d > 0).mean() <= 1e-3, (float(d.max()), float((d > 0).mean()))
    iw, ih, ow, oh = 1683, 1869, 2244, 2492
    img8 = synth.structured_u8(iw, ih, synth.seed_for(1, 0))
    assert np.array_equal(run_gpu(img8, ow, oh, np.uint8, precision=STRICT, sharpness=0.9, fused=1),
                          O.fsr_pipeline_u8(img8, ow, oh, sharpness=0.9))


def test_capture_ppm(gpu, tmp_path):
    import ctypes as C
    import torch
    import openvr_fsr_amd as A
    from openvr_fsr_amd.postprocessor import image_of
    img8 = synth.structured_u8(37, 21, 4)
    t = torch.from_numpy(img8).cuda()
    path = str(tmp_path / "cap.ppm")
    img = image_of(t)
    assert A.library().ovrfsr_save_ppm(C.byref(img), path.encode(), None) == 0
    raw = open(path, "rb").read()
    header = b"P6\n37 21\n255\n"
    assert raw.startswith(header) and raw[len(header):] == img8[..., :3].tobytes()


# ------------------------------------------------------------------------------------------------
# masked product-build pipeline: mask-sorted tile lists, LDS-free final-output kernel for tiles outside the radius
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius,proj,debug", [(0.5, (0.5, 0.5, 0.5, 0.5), 0), (0.6, (0.42, 0.55, 0.61, 0.47), 1), (0.25, (0.8, 0.2, 0.3, 0.7), 1)])
@pytest.mark.parametrize("fused", [-1, 0, 1])
def test_masked_product_paths_agree(gpu, radius, proj, debug, fused):
    """auto (fused + mask-sorted), two-pass mask-sorted and fused mask-sorted all within tolerance of the oracle,
    including a batch whose two eyes have different mask centres (separate per-eye launches)."""
    import torch
    import openvr_fsr_amd as A
    iw, ih, ow, oh = 330, 250, 440, 333
    imgs = np.stack([synth.structured_u8(iw, ih, 60 + i) for i in range(4)])
    pp = A.PostProcessor(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.8, radius=radius, proj_centre=proj,
                         debug_mode=debug, precision=FP32, fused=fused)
    outs = torch.empty((4, oh, ow, 4), dtype=torch.uint8, device="cuda")
    pp.apply_batch(torch.from_numpy(imgs).cuda(), outs, first_eye=1, alternate_eyes=True)
    torch.cuda.synchronize()
    got = outs.cpu().numpy()
    pp.close()
    for i in range(4):
        want = O.fsr_pipeline_u8(imgs[i], ow, oh, sharpness=0.8, radius=radius, proj=proj, eye=1 ^ (i & 1), debug=debug)
        mx, frac = lsb_stats(got[i], want)
        # outside the radius the pixel is a bilinear blend with 8-bit weights of byte texels: results land exactly on
        # UNORM8 rounding ties very often (5 % of bytes at scale 3/4), so the product build evaluates that blend
        # unfused, exactly as written (bilerp_unfused): those pixels are bit-identical to the oracle and the whole
        # frame meets the unmasked bound up to sampling noise (the inside region of this small frame is ~150 k values,
        # the bound a rate): 2x
        assert mx <= RCAS_LSB and frac <= 2 * LSB_FRACTION, (i, mx, frac)
    # single image through apply() as well
    one = run_gpu(imgs[0], ow, oh, np.uint8, eye=1, precision=FP32, sharpness=0.8, radius=radius, proj_centre=proj,
                  debug_mode=debug, fused=fused)
    assert np.array_equal(one, got[0])


@pytest.mark.parametrize("fused", [-1, 0])
@pytest.mark.parametrize("dt", [np.uint8, np.float16])
def test_masked_minification_product(gpu, fused, dt):
    """Explicit output size that minifies by 1.2x with the default radius: the tile footprint is wider than the
    fixed-pitch product kernels (40 cells), so the runtime-pitch kernel serves the mask-sorted launch and must take its
    tiles from the list (round 1 bug: it ignored the list and left most inside tiles unwritten)."""
    iw, ih, ow, oh = 360, 300, 300, 250
    img8 = synth.structured_u8(iw, ih, 17)
    img = img8 if dt == np.uint8 else (img8.astype(np.float32) / 255.0).astype(np.float16)
    want = run_gpu(img, ow, oh, dt, precision=STRICT, sharpness=0.8, radius=0.5, fused=0)
    got = run_gpu(img, ow, oh, dt, precision=FP32, sharpness=0.8, radius=0.5, fused=fused)
    if dt == np.uint8:
        assert np.array_equal(want, O.fsr_pipeline_u8(img8, ow, oh, sharpness=0.8, radius=0.5))
        mx, frac = lsb_stats(got, want)
        assert mx <= RCAS_LSB and frac <= 2 * LSB_FRACTION, (mx, frac)
    else:
        d = np.abs(got.astype(np.float32) - want.astype(np.float32))
        assert d.max() <= 1e-3, float(d.max())


@pytest.mark.parametrize("dtype,radius,nis", [(np.uint8, 2.0, 0), (np.uint8, 0.5, 0), (np.float16, 0.5, 0), (np.uint8, 0.5, 1)])
def test_hip_graph_capture_and_replay(gpu, dtype, radius, nis):
    """Once its lazy resources exist (one warm call), apply_batch is only kernel launches plus the event fork/join of the
    auxiliary stream, so it can be captured into a HIP graph on the caller's stream and replayed: same bytes as the
    direct call, for the unmasked, mask-sorted two-pass, fused + outside and NIS group-list pipelines."""
    import torch
    import openvr_fsr_amd as A
    iw, ih, ow, oh = 150, 120, 200, 160
    imgs8 = np.stack([synth.structured_u8(iw, ih, 30 + i) for i in range(4)])
    imgs = imgs8 if dtype == np.uint8 else (imgs8.astype(np.float32) / 255.0).astype(np.float16)
    tdt = torch.uint8 if dtype == np.uint8 else torch.float16
    t = torch.from_numpy(imgs).cuda()
    pp = A.PostProcessor(fsr_enabled=1, use_nis=nis, out_width=ow, out_height=oh, sharpness=0.8, radius=radius,
                         proj_centre=(0.45, 0.5, 0.55, 0.5))
    ref = torch.empty((4, oh, ow, 4), dtype=tdt, device="cuda")
    out = torch.zeros_like(ref)
    pp.apply_batch(t, ref, first_eye=0, alternate_eyes=True)      # also builds the lazy resources
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            pp.apply_batch(t, out, first_eye=0, alternate_eyes=True)
    torch.cuda.synchronize()
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    t.copy_(torch.flip(t, dims=[0]))                              # new input in the same buffers, replay again
    pp.apply_batch(t, ref, first_eye=0, alternate_eyes=True)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    pp.close()


@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
@pytest.mark.parametrize("radius,debug", [(2.0, 0), (0.5, 0), (0.5, 1)])
def test_a_call_that_must_build_is_refused_under_capture(gpu, radius, debug):
    """A capturing stream takes launches only.  A cold ctx (or a larger batch than any before) under capture used to fail inside the rebuild with
    "operation not permitted when stream is capturing": the caller's capture invalidated, the ctx DISABLED until reset.  Now the call is refused
    up front (INVALID_ARGUMENT, header `stream`): the capture survives, the ctx stays usable, and the same capture succeeds after one plain call
    -- also in debug mode, whose timing ring a captured call leaves alone."""
    import torch
    import openvr_fsr_amd as A
    iw, ih, ow, oh = 150, 120, 200, 160
    t = torch.from_numpy(np.stack([synth.structured_u8(iw, ih, 40 + i) for i in range(4)])).cuda()
    pp = A.PostProcessor(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.8, radius=radius, debug_mode=debug)
    out = torch.zeros((4, oh, ow, 4), dtype=torch.uint8, device="cuda")
    ref = torch.zeros_like(out)
    side = torch.cuda.Stream()

    def capture(n):
        g = torch.cuda.CUDAGraph()
        side.wait_stream(torch.cuda.current_stream())
        err = None
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):          # (leaving the block ends the capture: it must still be valid)
                try:
                    pp.apply_batch(t[:n], out[:n], first_eye=0, alternate_eyes=True)
                except A.OvrFsrError as e:
                    err = e
        torch.cuda.synchronize()
        return g, err

    g, err = capture(2)                                     # cold ctx
    assert err is not None and err.status == 1 and "capturing stream" in str(err), err
    pp.apply_batch(t[:2], ref[:2], first_eye=0, alternate_eyes=True)   # no reset needed: the refusal disabled nothing
    torch.cuda.synchronize()
    g, err = capture(2)                                     # warm: captured
    assert err is None
    out.zero_(); g.replay(); torch.cuda.synchronize()
    assert torch.equal(out[:2], ref[:2])
    g4, err = capture(4)                                    # a larger batch needs a larger intermediate: refused again (two-kernel pipelines)
    if err is not None:
        assert err.status == 1   # INVALID_ARGUMENT
    pp.apply_batch(t, ref, first_eye=0, alternate_eyes=True)
    torch.cuda.synchronize()
    g4, err = capture(4)
    assert err is None
    out.zero_(); g4.replay(); torch.cuda.synchronize()
    assert torch.equal(out, ref)
    if debug:
        assert pp.last_gpu_time_ms() > 0                    # the plain calls were timed, the captured ones left the ring alone
    pp.close()


def test_plain_c_caller(gpu, tmp_path):
    """examples/headless (plain C11, built by __graft_entry__.build()): create, apply both eyes with a ctx-owned output,
    debug-mode GPU time, PPM capture -- the C ABI end to end without Python in the loop."""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "headless")
    if not os.path.exists(exe):
        pytest.skip("examples/headless not built")
    ppm = str(tmp_path / "eye.ppm")
    r = subprocess.run([exe, "-", ppm], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("eye ")]
    assert len(lines) == 6 and all("1683x1869 -> 2244x2492" in l and " ms on the GPU" in l for l in lines), r.stdout
    data = open(ppm, "rb").read()
    assert data.startswith(b"P6\n2244 2492\n255\n") and len(data) == len(b"P6\n2244 2492\n255\n") + 2244 * 2492 * 3
    px = np.frombuffer(data[len(b"P6\n2244 2492\n255\n"):], np.uint8)
    assert px.std() > 10    # an image, not a constant
    # round 5 from plain C: cfg.pair_submit (LEFT recorded, RIGHT launches both eyes) gives the same right eye, and the DDS capture
    dds = str(tmp_path / "eye.dds")
    r2 = subprocess.run([exe, "-", dds, "--pair"], capture_output=True, text=True, timeout=120)
    assert r2.returncode == 0, r2.stderr
    cs = [l.split()[3] for l in r.stdout.splitlines() if l.startswith("right eye checksum")]
    cs2 = [l.split()[3] for l in r2.stdout.splitlines() if l.startswith("right eye checksum")]
    assert len(cs) == 1 and cs == cs2 and "(pair_submit)" in r2.stdout
    # the pair really forms (each eye has its own texture): three LEFT applies recorded, three RIGHT applies launching both -- ovrfsr_pair_pending
    assert r2.stdout.count("eye 0: recorded (pair_submit)") == 3 and r2.stdout.count("(both eyes, one batch of two)") == 3, r2.stdout
    # round 6 (ABI 5): a game that submits the right eye first pairs as well, same pixels
    r3 = subprocess.run([exe, "-", str(tmp_path / "eye_rl.dds"), "--pair-rl"], capture_output=True, text=True, timeout=120)
    assert r3.returncode == 0, r3.stderr
    cs3 = [l.split()[3] for l in r3.stdout.splitlines() if l.startswith("right eye checksum")]
    assert cs3 == cs and r3.stdout.count("eye 1: recorded (pair_submit)") == 3 and r3.stdout.count("eye 0: recorded") == 0, r3.stdout
    d = open(dds, "rb").read()
    assert d[:4] == b"DDS " and len(d) == 148 + 2244 * 2492 * 4 and np.array_equal(np.frombuffer(d[148:], np.uint8).reshape(2492, 2244, 4)[..., :3].reshape(-1), px)


def test_c_node_driver(gpu):
    """examples/bench_node (C11 + pthreads, built by __graft_entry__.build()): the multi-GPU loop of bench.py with no Python in
    it -- two shards (one thread, ctx and stream each; both on device 0 here: --oversubscribe), exactly K timed steps each, one
    JSON line with per-device times."""
    import json
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "bench_node")
    if not os.path.exists(exe):
        pytest.skip("examples/bench_node not built")
    r = subprocess.run([exe, "--gpus", "2", "--oversubscribe", "--pairs", "2", "--steps", "3", "--warmup", "1"], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["unit"] == "eye-pairs/s" and d["value"] > 0
    assert len(d["config"]["per_device_ms_per_step"]) == 2 and all(m > 0 for m in d["config"]["per_device_ms_per_step"])
    assert d["config"]["pairs_per_gpu_per_step"] == 2 and "oversubscribed" in d["config"]
    # self-verifying per device (round 5): image 0 of every shard's timed output against device 0 processing the same seed
    ps = d["parity_check"]["per_shard"]
    assert d["parity_check"]["ok"] is True and [p["shard"] for p in ps] == [0, 1] and all(p["matches_device0"] for p in ps)
    assert ps[0]["checksum"] != ps[1]["checksum"]          # different seeds, different images
    # ... and a shard whose output is wrong fails the run by name
    r = subprocess.run([exe, "--gpus", "2", "--oversubscribe", "--pairs", "2", "--steps", "2", "--warmup", "1", "--corrupt-shard", "1"],
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 1 and "shard 1 (device 0)" in r.stderr, (r.returncode, r.stderr)
    bad = json.loads(r.stdout.strip().splitlines()[-1])["parity_check"]
    assert bad["ok"] is False and [p["matches_device0"] for p in bad["per_shard"]] == [True, False]
    # the fused kernel (cfg.fused = 1) raises its dynamic-LDS attribute per (kernel, device): two ctxs, one process, masked tiles
    r = subprocess.run([exe, "--gpus", "2", "--oversubscribe", "--pairs", "2", "--steps", "2", "--warmup", "1", "--fused", "--radius", "0.5"],
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1])["value"] > 0


@pytest.mark.parametrize("launcher", ["direct", "torchrun"])
def test_driver_commands_on_real_shards(gpu, launcher):
    """The round driver's N > 1 commands -- `python bench.py --gpus 2 ...` and the same under `python -m torch.distributed.run --nproc-per-node 2` --
    on REAL shards (tests/test_bench_launcher.py runs them on mock shards on CPU): gpurun boxes have one GPU, so both shards sit on device 0
    (--oversubscribe; the line says so).  One JSON line, one per-device time and one parity record per shard (image 0 of each shard's own timed
    batch against the oracle, gathered over the ranks), value = 2 x pairs x steps / the slowest shard."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tail = ["bench.py", "--gpus", "2", "--oversubscribe", "--pairs", "4", "--steps", "3", "--warmup", "1", "--no-cpu", "--no-extras", "--pmc", "off"]
    cmd = [sys.executable] + tail if launcher == "direct" else \
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29533"] + tail
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["scaling"] == "weak" and "oversubscribed" in d["config"]
    per_dev = d["config"]["per_device_ms_per_step"]
    assert len(per_dev) == 2 and all(m > 0 for m in per_dev) and d["ms_per_step"] >= max(per_dev) * 0.95
    assert d["value"] == pytest.approx(2 * 4 / (d["ms_per_step"] * 1e-3), rel=1e-3)
    pc = d["parity_check"]
    assert pc["ok"] is True and pc["failed_shards"] == [] and [p["shard"] for p in pc["per_shard"]] == [0, 1] and all(p["ok"] for p in pc["per_shard"])
    assert ("one rank per GPU" in d["config"]["launcher"]) == (launcher == "torchrun"), d["config"]["launcher"]


# ------------------------------------------------------------------------------------------------
# round 2: the reference's averaged GPU-time log, and the two product RCAS kernels agree byte for byte
# ------------------------------------------------------------------------------------------------
def test_average_gpu_time_ring(gpu):
    """PostProcessor.cpp:605-626: a ring of 6 query pairs, the oldest read back after every apply, the mean of 500 readings
    published, doubled when each eye has its own texture (one reading = one eye, the figure = one frame)."""
    import torch
    import openvr_fsr_amd as A
    t = torch.from_numpy(synth.structured_u8(96, 80, 3)).cuda()
    pp = A.PostProcessor(fsr_enabled=1, out_width=128, out_height=107, sharpness=0.9, radius=2.0, debug_mode=1)
    out = torch.empty((107, 128, 4), dtype=torch.uint8, device="cuda")
    assert pp.average_gpu_time_ms() == (0.0, 0)
    for i in range(504):                       # the first reading comes from the 6th apply: 499 readings after 504 applies
        pp.apply(i & 1, t, out=out)
    assert pp.average_gpu_time_ms()[1] == 0
    pp.apply(0, t, out=out)                    # 500th reading -> one mean published
    avg, reports = pp.average_gpu_time_ms()
    one = pp.last_gpu_time_ms()
    assert reports == 1 and avg > 0.0
    assert 0.5 * (2 * one) < avg < 20 * (2 * one), (avg, one)     # per FRAME: twice a per-eye reading (loose: clocks, launch gaps)
    for i in range(500):
        pp.apply(i & 1, t, out=out)
    assert pp.average_gpu_time_ms()[1] == 2
    pp.close()


def test_rcas_dpp_kernel_equals_per_lane_loads_kernel(gpu):
    """rcas_dpp_kernel (side taps from neighbour lanes) and rcas_direct_kernel (every lane loads its own 14 taps) are the same
    arithmetic: identical bytes, including image borders and widths that are not a multiple of the 62-column wave tile -- on
    unmasked frames (regular 62 x 32 grid) and on the mask-sorted form of masked ones (segments of the inside runs, tinted copy
    in the groups outside the radius).  The per-lane-loads side is a measurement build of the library (-DOVRFSR_RCAS_NO_DPP, built on
    demand like the audit build), so each form runs in its own interpreter."""
    import hashlib
    import os
    import subprocess
    import sys
    from tests.variants import variant
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, hashlib, numpy as np; sys.path.insert(0, %r)\n"
            "from tests import synth; from tests.util import run_gpu\n"
            "h = hashlib.sha256()\n"
            "for (w, hgt, gen) in [(2244, 2492, synth.structured_u8), (125, 67, synth.random_u8), (61, 33, synth.extremes_u8), (63, 5, synth.random_u8)]:\n"
            "    h.update(run_gpu(gen(w, hgt, 5), w, hgt, np.uint8, render_scale=1.0, sharpness=0.9, radius=100.0).tobytes())\n"
            "    h.update(run_gpu(gen(w, hgt, 6), w, hgt, np.float32, render_scale=1.0, sharpness=0.3, radius=100.0).tobytes())\n"
            "# masked EASU+RCAS (mask-sorted form): rcas_dpp_kernel on 62-column segments of the inside runs vs rcas_direct_kernel on the tile list\n"
            "for (iw, ih, ow, oh, kw) in [(300, 260, 400, 347, dict(radius=0.5)), (250, 200, 333, 267, dict(radius=0.7, debug_mode=1, proj_centre=(0.4, 0.45, 0.6, 0.55))),\n"
            "                             (96, 80, 128, 107, dict(radius=0.3)), (1683, 1869, 2244, 2492, dict(radius=0.5)), (47, 300, 63, 400, dict(radius=1.2))]:\n"
            "    for dt in (np.uint8, np.float32):\n"
            "        for eye in (0, 1):\n"
            "            h.update(run_gpu(synth.structured_u8(iw, ih, 7 + eye), ow, oh, dt, eye=eye, out_width=ow, out_height=oh, sharpness=0.9, **kw).tobytes())\n"
            "print(h.hexdigest())\n") % root
    digests = []
    for env in (None, dict(os.environ, OVRFSR_LIB=variant("rcas_nodpp", "-DOVRFSR_RCAS_NO_DPP"))):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        digests.append(r.stdout.strip().splitlines()[-1])
    assert digests[0] == digests[1]


def test_two_ctxs_on_two_host_threads(gpu):
    """Distinct ctxs are independent (header: "one per device; not thread-safe; distinct ctxs are independent"): two host threads,
    each with its own ctx and its own stream on the same device, interleave applies of different configurations; every result
    equals the single-threaded one."""
    import threading
    import torch
    import openvr_fsr_amd as A
    imgs = [synth.structured_u8(150, 120, 40 + i) for i in range(6)]
    cfgs = [dict(fsr_enabled=1, out_width=200, out_height=160, sharpness=0.8, radius=0.6, proj_centre=(0.45, 0.5, 0.55, 0.5)),
            dict(fsr_enabled=1, use_nis=1, out_width=200, out_height=160, sharpness=0.5, radius=2.0)]
    want = [[run_gpu(im, 200, 160, np.uint8, eye=i & 1, **cfg) for i, im in enumerate(imgs)] for cfg in cfgs]
    got = [[None] * len(imgs) for _ in cfgs]
    errors = []

    def worker(ci):
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                pp = A.PostProcessor(**cfgs[ci])
                for rep in range(5):
                    for i, im in enumerate(imgs):
                        t = torch.from_numpy(im).cuda()
                        out = pp.apply(i & 1, t, out_dtype=torch.uint8)
                        stream.synchronize()
                        got[ci][i] = out.cpu().numpy()
                pp.close()
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(ci,)) for ci in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for ci in range(2):
        for i in range(len(imgs)):
            assert np.array_equal(got[ci][i], want[ci][i]), (ci, i)

