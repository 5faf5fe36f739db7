"""The per-axis scale regimes of the EASU kernels on the GPU: every row of the table of tests/scale_cases.py -- steep (8x, 6x, 3x), anisotropic,
one axis at 1:1, y minified under a fixed pitch (row pairs two rows apart, 37 to 52 staged rows), x minified (the generic kernel at 47, 72 and
100 cells across), isotropic minification at the 64 KiB line, and both sides of the accept / refuse line -- each frame against the ORACLE,
never against a twin ctx.  The unmasked forms run at the table's shapes, the masked ones (radius 0.5, unequal eye centres) at the doubled
shapes, whose class tests/scale_cases.class_property proves equal and whose inside, ring and outside tile sets are asserted non-empty through
tests/mask_ref.py before anything is compared.  Tolerances are those include/openvr_fsr_amd.h and tests/test_gpu_parity.py state:
    strict: bit for bit (EASU RGBA32F output and the UNORM8 pipeline); FP32_EXACT: the strict build's bytes, the oracle's where strict refuses;
    product: EASU RGBA8 identical to float_to_unorm8(oracle), EASU float <= FLOAT_TOL, UNORM8 pipelines <= 1 LSB, pixels of groups outside
    the radius the oracle's bytes in every RGBA8 form, mask-sorted == plain two-pass; half pipelines under test_masked_product_fuzz_half's
    bound (99.9 % of the values within 1e-3, none beyond 2e-2); NVScaler: strict bit for bit, product <= NIS_FLOAT_TOL and <= 1 LSB,
    DirectCopy groups identical.
Product-build distances go to reports/scale_regimes.json (ignored by git; OVRFSR_REPORT_DIR names another directory; committed copy:
profiles/scale_regimes.json): max LSB, max abs, the share of differing bytes -- recorded, not asserted."""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import mask_ref as MR
from tests import msaa
from tests import packedf
from tests import scale_cases as SC
from tests import synth
from tests.test_gpu_parity import FLOAT_TOL, NIS_FLOAT_TOL, RCAS_LSB, lsb_stats

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARP = 0.9
STRICT, EXACT = 2, 3
GENS = [synth.structured_u8, synth.random_u8, synth.extremes_u8, synth.structured_u8]   # image i of a call
UNMASKED = dict(radius=2.0)
MASKED = dict(radius=SC.MASK_RADIUS, proj_centre=SC.MASK_PROJ)
_RECORDS = []

PRODUCT_IDS = [c.id for c in SC.ACCEPTED]
STRICT_IDS = [c.id for c in SC.STRICT_ACCEPTED]
REFUSED_IDS = [c.id for c in SC.CASES if not c.product]


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    if not _RECORDS:
        return
    out_dir = os.environ.get("OVRFSR_REPORT_DIR") or os.path.join(ROOT, "reports")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "scale_regimes.json"), "w") as f:
        json.dump({"note": "per-axis scale regimes (tests/scale_cases.py), product build vs CPU oracle, the largest value over a call's images; "
                           "written by tests/test_gpu_scale_regimes.py", "records": _RECORDS}, f, indent=1)


def _record(case, form, shape, got, want):
    if got.dtype == np.uint8:
        mx, frac = lsb_stats(got, want)
        rec = dict(max_lsb=mx, max_abs=None, differing=frac)
    else:
        d = np.abs(got.astype(np.float32) - want.astype(np.float32))
        rec = dict(max_lsb=None, max_abs=float(d.max()), differing=float((d != 0).mean()))
    print((case, form), rec)
    _RECORDS.append(dict(case=case, form=form, shape=list(shape), **rec))
    return rec


# ---- inputs and oracle results, computed once ------------------------------------------------------------------------------------------------
def _shape(c, masked):
    return c.masked_shape if masked else c.shape


@functools.lru_cache(maxsize=None)
def _image8(iw, ih, i):
    return GENS[i & 3](iw, ih, synth.seed_for(41, i))


def _imageh(iw, ih, i):
    return (_image8(iw, ih, i).astype(np.float32) / np.float32(255)).astype(np.float16)


def _mask(shape, masked, eye):
    return O.mask_constants(shape[2], shape[3], SC.MASK_RADIUS, SC.MASK_PROJ, True, eye) if masked else O.mask_constants(shape[2], shape[3])


@functools.lru_cache(maxsize=None)
def _want_easu(shape, masked, i):
    """the oracle's EASU of image i (eye i & 1) from the UNORM8 texels: float32"""
    iw, ih, ow, oh = shape
    centre, rad = _mask(shape, masked, i & 1)
    return O.easu(O.unorm8_to_float(_image8(iw, ih, i)), ow, oh, O.easu_con(iw, ih, ow, oh), centre, rad)


@functools.lru_cache(maxsize=None)
def _want_pipeline(shape, masked, i):
    iw, ih, ow, oh = shape
    kw = dict(radius=SC.MASK_RADIUS, proj=SC.MASK_PROJ) if masked else {}
    return O.fsr_pipeline_u8(_image8(iw, ih, i), ow, oh, sharpness=SHARP, eye=i & 1, **kw)


@functools.lru_cache(maxsize=None)
def _want_half(shape, masked, i):
    """half in, half intermediate, half out (tests/test_gpu_fuzz.py, test_masked_product_fuzz_half): float16"""
    iw, ih, ow, oh = shape
    centre, rad = _mask(shape, masked, i & 1)
    e = O.easu(_imageh(iw, ih, i).astype(np.float32), ow, oh, O.easu_con(iw, ih, ow, oh), centre, rad)
    return O.rcas(e.astype(np.float16).astype(np.float32), O.rcas_con(SHARP), centre, rad).astype(np.float16)


def _inside(shape, masked, eye, kind="fsr"):
    if not masked:
        return np.ones((shape[3], shape[2]), bool)
    return MR.mask_ref(shape, SC.MASK_RADIUS, SC.MASK_PROJ, True, eye, kind).pixels


def _tile_sets_present(shape, kind="fsr"):
    """each eye's inside, ring and outside tile sets are non-empty (tests/mask_ref.py), and the eyes differ"""
    th = 24 if kind == "nvscaler" else 32
    refs = [MR.mask_ref(shape, SC.MASK_RADIUS, SC.MASK_PROJ, True, eye, kind) for eye in (0, 1)]
    for r in refs:
        inside, outside = r.tiles(32, th)
        assert r.mode == MR.MIXED and inside and r.ring(32, th) and outside - r.ring(32, th), (shape, kind)
    assert not np.array_equal(refs[0].centre, refs[1].centre)


# ---- calls -------------------------------------------------------------------------------------------------------------------------------------
def _cfg(shape, masked, **more):
    return dict(fsr_enabled=1, out_width=shape[2], out_height=shape[3], sharpness=SHARP, **dict(MASKED if masked else UNMASKED, **more))


_GOT = {}


def _frames(torch, shape, masked, src="rgba8", out=None, in_pad=0, out_pad=0, **more):
    """images 0 (left eye) and 1 (right eye) through single applies on one fresh ctx, into 0xA5-filled destinations -> numpy [2, oh, ow, 4];
    with out_pad also the pad columns' bytes.  Cached per argument set: several tests look at the same call"""
    import openvr_fsr_amd as A
    key = (shape, masked, src, out, in_pad, out_pad, tuple(sorted(more.items())))
    if key in _GOT:
        return _GOT[key]
    iw, ih, ow, oh = shape
    out = out or src
    tdt, size = {"rgba8": torch.uint8, "rgba16f": torch.float16, "rgba32f": torch.float32}, {"rgba8": 1, "rgba16f": 2, "rgba32f": 4}
    pp = A.PostProcessor(**_cfg(shape, masked, **more))
    try:
        got, pads = [], []
        for i in (0, 1):
            img = {"rgba8": _image8(iw, ih, i), "rgba16f": _imageh(iw, ih, i), "rgba32f": _imageh(iw, ih, i).astype(np.float32)}[src]
            tin = torch.zeros((ih, iw + in_pad, 4), dtype=tdt[src], device="cuda")
            tin[:, :iw] = torch.from_numpy(img).cuda()
            raw = torch.full((oh, (ow + out_pad) * 4 * size[out]), 0xA5, dtype=torch.uint8, device="cuda")
            tout = (raw if out == "rgba8" else raw.view(tdt[out])).reshape(oh, ow + out_pad, 4)
            pp.apply(i & 1, tin[:, :iw], out=tout[:, :ow])
            torch.cuda.synchronize()
            got.append(tout[:, :ow].cpu().numpy())
            pads.append(tout[:, ow:].contiguous().view(torch.uint8).cpu().numpy())
    finally:
        pp.close()
    _GOT[key] = (np.stack(got), np.stack(pads)) if out_pad else np.stack(got)
    return _GOT[key]


def _refused(torch, shape, src="rgba8", **more):
    """-> (status, text of ovrfsr_last_error) of an apply the planner refuses"""
    import openvr_fsr_amd as A
    with pytest.raises(A.OvrFsrError) as e:
        _frames(torch, shape, False, src, **more)
    return e.value.status, str(e.value).split("): ", 1)[1]


# ---- the strict build ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [0, 1], ids=["unmasked", "masked"])
@pytest.mark.parametrize("cid", STRICT_IDS)
def test_strict_bit_identical(gpu, cid, masked):
    c = SC.BY_ID[cid]
    SC.class_property(c)
    shape = _shape(c, masked)
    if masked:
        _tile_sets_present(shape)
    easu = _frames(gpu, shape, masked, out="rgba32f", precision=STRICT, stage_mask=1)
    pipe = _frames(gpu, shape, masked, precision=STRICT)
    for i in (0, 1):
        want = _want_easu(shape, masked, i)
        assert np.array_equal(easu[i].view(np.uint32), want.view(np.uint32)), (cid, i, float(np.abs(easu[i] - want).max()))
        assert np.array_equal(pipe[i], _want_pipeline(shape, masked, i)), (cid, i, lsb_stats(pipe[i], _want_pipeline(shape, masked, i)))


# ---- the product build -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [0, 1], ids=["unmasked", "masked"])
@pytest.mark.parametrize("cid", PRODUCT_IDS)
def test_product_easu(gpu, cid, masked):
    """the EASU pass alone: RGBA8 -> RGBA8 identical to float_to_unorm8(oracle) (the near-tie guard), RGBA8 -> RGBA32F within FLOAT_TOL"""
    c = SC.BY_ID[cid]
    SC.class_property(c)
    shape = _shape(c, masked)
    if masked:
        _tile_sets_present(shape)
    got8 = _frames(gpu, shape, masked, stage_mask=1)
    gotf = _frames(gpu, shape, masked, out="rgba32f", stage_mask=1)
    want = np.stack([_want_easu(shape, masked, i) for i in (0, 1)])
    _record(cid, "easu-rgba8" + "-masked" * masked, shape, got8, O.float_to_unorm8(want))
    rec = _record(cid, "easu-float" + "-masked" * masked, shape, gotf, want)
    assert np.array_equal(got8, O.float_to_unorm8(want)), (cid, lsb_stats(got8, O.float_to_unorm8(want)))
    assert rec["max_abs"] <= FLOAT_TOL, (cid, rec)


def _pipeline_forms(c, masked):
    return [("auto", {})] + ([("fused-0", dict(fused=0))] if masked else []) + ([("fused-1", dict(fused=1))] if c.fused else [])


@pytest.mark.parametrize("masked", [0, 1], ids=["unmasked", "masked"])
@pytest.mark.parametrize("cid", PRODUCT_IDS)
def test_product_pipeline(gpu, cid, masked):
    """EASU -> UNORM8 -> RCAS in every form the planner accepts: <= 1 LSB; outside the radius the oracle's bytes; mask-sorted == two-pass;
    `fused = 1` refused with the table's text exactly where the table says"""
    c = SC.BY_ID[cid]
    SC.class_property(c)
    shape = _shape(c, masked)
    want = np.stack([_want_pipeline(shape, masked, i) for i in (0, 1)])
    outside = np.stack([~_inside(shape, masked, i) for i in (0, 1)])
    got = {}
    for form, cfg in _pipeline_forms(c, masked):
        got[form] = _frames(gpu, shape, masked, **cfg)
        rec = _record(cid, form + "-masked" * masked, shape, got[form], want)
        assert np.array_equal(got[form][outside], want[outside]), (cid, form, "a pixel of a group outside the radius differs from the oracle's")
        assert rec["max_lsb"] <= RCAS_LSB, (cid, form, rec)
    if masked:
        assert np.array_equal(got["auto"], got["fused-0"]), cid        # mask-sorted == plain two-pass
    if not c.fused:
        assert _refused(gpu, shape, fused=1) == SC.REFUSED_FUSED, cid


@pytest.mark.parametrize("cid", PRODUCT_IDS)
def test_exact_stores(gpu, cid):
    """FP32_EXACT == the strict build's bytes where strict plans, == the oracle's bytes at iso-min-* where it does not"""
    c = SC.BY_ID[cid]
    assert c.strict or c.klass == "iso-minify"
    for masked in (0, 1):
        shape = _shape(c, masked)
        got = _frames(gpu, shape, masked, precision=EXACT)
        want = _frames(gpu, shape, masked, precision=STRICT) if c.strict else np.stack([_want_pipeline(shape, masked, i) for i in (0, 1)])
        assert np.array_equal(got, want), (cid, masked, lsb_stats(got, want))


@pytest.mark.parametrize("cid", SC.PITCHED_IDS)
def test_padded_row_pitches(gpu, cid):
    """rows of the source and of the destination longer than the image: the same bytes, the destination's pad bytes untouched"""
    c = SC.BY_ID[cid]
    for masked in (0, 1):
        shape = _shape(c, masked)
        for cfg in ({}, dict(stage_mask=1)):
            got, pads = _frames(gpu, shape, masked, in_pad=3, out_pad=5, **cfg)
            assert np.array_equal(got, _frames(gpu, shape, masked, **cfg)), (cid, masked, cfg)
            assert pads.size and (pads == 0xA5).all(), (cid, masked, cfg, "wrote outside the output image")


# ---- half and float sources ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", SC.HALF_IDS)
def test_half_pipelines(gpu, cid):
    """RGBA16F in and out, masked, auto and `fused = 1`: strict bit-identical where planned, product under test_masked_product_fuzz_half's bound"""
    c = SC.BY_ID[cid]
    SC.class_property(c)
    shape = c.masked_shape
    _tile_sets_present(shape)
    want = np.stack([_want_half(shape, 1, i) for i in (0, 1)])
    if c.strict:
        got = _frames(gpu, shape, 1, src="rgba16f", precision=STRICT)
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), cid
    else:
        assert _refused(gpu, shape, src="rgba16f", precision=STRICT) == SC.REFUSED_LDS, cid
    for form, cfg in [("half-auto", {})] + ([("half-fused-1", dict(fused=1))] if c.fused else []):
        got = _frames(gpu, shape, 1, src="rgba16f", **cfg)
        _record(cid, form, shape, got, want)
        err = np.abs(got.astype(np.float32) - want.astype(np.float32))
        assert (err <= 1e-3).mean() >= 0.999 and err.max() <= 2e-2, (cid, form, float((err <= 1e-3).mean()), float(err.max()))
    if not c.fused:
        assert _refused(gpu, shape, src="rgba16f", fused=1) == SC.REFUSED_FUSED, cid


@pytest.mark.parametrize("cid", ["wide-100", "tall-32-deep"])
def test_float_source(gpu, cid):
    """an RGBA32F source (the 16-byte colour plane of the generic layout; the fast kernel's float staging): EASU strict bit for bit, product
    within FLOAT_TOL"""
    c = SC.BY_ID[cid]
    iw, ih, ow, oh = shape = c.shape
    want = np.stack([O.easu(_imageh(iw, ih, i).astype(np.float32), ow, oh) for i in (0, 1)])
    got = _frames(gpu, shape, 0, src="rgba32f", precision=STRICT, stage_mask=1)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), cid
    got = _frames(gpu, shape, 0, src="rgba32f", stage_mask=1)
    rec = _record(cid, "easu-rgba32f-source", shape, got, want)
    assert rec["max_abs"] <= FLOAT_TOL, (cid, rec)


def test_float_source_refused_at_the_isotropic_line(gpu):
    c = SC.BY_ID["iso-min-46"]
    assert SC.RGBA32F not in c.product and SC.RGBA8 in c.product
    assert _refused(gpu, c.shape, src="rgba32f") == SC.REFUSED_LDS


@pytest.mark.parametrize("cid", ["tall-32", "wide-47"])
def test_batch_of_four(gpu, cid):
    """four images, alternating eyes, one call, masked: each image against the oracle"""
    torch = gpu
    import openvr_fsr_amd as A
    c = SC.BY_ID[cid]
    iw, ih, ow, oh = shape = c.masked_shape
    _tile_sets_present(shape)
    texs = torch.from_numpy(np.stack([_image8(iw, ih, i) for i in range(4)])).cuda()
    outs = torch.full((4, oh, ow, 4), 0xA5, dtype=torch.uint8, device="cuda")
    pp = A.PostProcessor(**_cfg(shape, 1))
    try:
        pp.apply_batch(texs, outs, first_eye=0, alternate_eyes=True)
        torch.cuda.synchronize()
    finally:
        pp.close()
    got = outs.cpu().numpy()
    want = np.stack([_want_pipeline(shape, 1, i) for i in range(4)])
    outside = np.stack([~_inside(shape, 1, i & 1) for i in range(4)])
    rec = _record(cid, "batch-of-4-masked", shape, got, want)
    assert np.array_equal(got[outside], want[outside]), cid
    assert rec["max_lsb"] <= RCAS_LSB, (cid, rec)
    assert np.array_equal(got[:2], _frames(gpu, shape, 1)), cid      # (the single applies of the same images)


# ---- NVScaler ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _want_nis(shape, masked, i):
    import openvr_fsr_amd as A
    iw, ih, ow, oh = shape
    cs, cu = A.nis_coefs()
    ok, cfg = A.nis_scaler_config(SHARP, iw, ih, ow, oh)
    assert ok, shape
    centre, rad = _mask(shape, masked, i & 1)
    return O.nis_upscale(O.unorm8_to_float(_image8(iw, ih, i)), ow, oh, O.nis_block(cfg, centre, rad, 0), cs, cu)


@pytest.mark.parametrize("masked", [0, 1], ids=["unmasked", "masked"])
@pytest.mark.parametrize("shape", SC.NIS_SHAPES, ids=["%dx%d-%dx%d" % s for s in SC.NIS_SHAPES])
def test_nvscaler(gpu, shape, masked):
    tag = "nis-%dx%d-%dx%d" % shape
    if masked:
        shape = tuple(2 * v for v in shape)
        _tile_sets_present(shape, "nvscaler")
    want = np.stack([_want_nis(shape, masked, i) for i in (0, 1)])
    want8 = O.float_to_unorm8(want)
    outside = np.stack([~_inside(shape, masked, i, "nvscaler") for i in (0, 1)])
    got = _frames(gpu, shape, masked, out="rgba32f", use_nis=1, precision=STRICT)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (shape, float(np.abs(got - want).max()))
    assert np.array_equal(_frames(gpu, shape, masked, use_nis=1, precision=STRICT), want8), shape
    gotf, got8 = _frames(gpu, shape, masked, out="rgba32f", use_nis=1), _frames(gpu, shape, masked, use_nis=1)
    recf = _record(tag, "nis-float" + "-masked" * masked, shape, gotf, want)
    rec8 = _record(tag, "nis-rgba8" + "-masked" * masked, shape, got8, want8)
    assert recf["max_abs"] <= NIS_FLOAT_TOL and rec8["max_lsb"] <= 1, (shape, recf, rec8)
    assert np.array_equal(got8[outside], want8[outside]) and np.array_equal(gotf[outside].view(np.uint32), want[outside].view(np.uint32)), shape   # DirectCopy


# ---- small things only these ratios reach ------------------------------------------------------------------------------------------------------
def _apply_once(torch, shape, tex, out_dtype, in_format=None, hdr=None, **more):
    import openvr_fsr_amd as A
    pp = A.PostProcessor(**_cfg(shape, 0, **more))
    try:
        if hdr is not None:
            pp.set_hdr_domain(hdr)
        out = torch.full((shape[3], shape[2], 4), 0, dtype=out_dtype, device="cuda")
        pp.apply(0, tex, out=out, in_format=in_format)
        torch.cuda.synchronize()
        return out.cpu().numpy()
    finally:
        pp.close()


@pytest.mark.parametrize("cid", ["wide-47", "steep-3x"])
def test_packed_float_submission(gpu, cid):
    """R11G11B10F at wide-47 (more than 40 cells: the resolve pass) and at steep-3x (decoded in staging) == the RGBA16F apply of its decoded
    values, byte for byte, which in turn is within the half bound of the oracle"""
    torch = gpu
    import openvr_fsr_amd as A
    c = SC.BY_ID[cid]
    iw, ih, ow, oh = c.shape
    assert (c.pitch == 0) == (cid == "wide-47")
    packed = packedf.make(iw, ih, "structured", synth.seed_for(43, 0))
    decoded = packedf.unpack(packed)
    got = _apply_once(torch, c.shape, torch.from_numpy(packed.view(np.int32)).cuda(), torch.float16, in_format=A.FORMAT_R11G11B10F)
    want = _apply_once(torch, c.shape, torch.from_numpy(decoded).cuda(), torch.float16)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), cid
    e = O.easu(decoded.astype(np.float32), ow, oh)
    ref = O.rcas(e.astype(np.float16).astype(np.float32), O.rcas_con(SHARP)).astype(np.float16)
    err = np.abs(got.astype(np.float32) - ref.astype(np.float32))
    assert (err <= 1e-3).mean() >= 0.999 and err.max() <= 2e-2, (cid, float(err.max()))


@pytest.mark.parametrize("cid", ["steep-3x", "wide-47"])
def test_multisampled_submission(gpu, cid):
    """4x RGBA8 at steep-3x (resolved in staging) and wide-47 (the resolve pass) == the apply of its resolved image == within 1 LSB of the oracle"""
    torch = gpu
    c = SC.BY_ID[cid]
    iw, ih, ow, oh = c.shape
    ms = msaa.make_ms(iw, ih, 4, "rgba8", "structured", synth.seed_for(44, 0))
    resolved = msaa.resolve_unorm8(ms)
    got = _apply_once(torch, c.shape, torch.from_numpy(ms).cuda(), torch.uint8)
    want = _apply_once(torch, c.shape, torch.from_numpy(resolved).cuda(), torch.uint8)
    assert np.array_equal(got, want), (cid, lsb_stats(got, want))
    mx, _ = lsb_stats(got, O.fsr_pipeline_u8(resolved, ow, oh, sharpness=SHARP))
    assert mx <= RCAS_LSB, (cid, mx)


def test_hdr_domain_is_not_applied_where_the_float_twin_is_refused(gpu):
    """ovrfsr_set_hdr_domain(SRTM) on a half submission at iso-min-46: the RGBA32F plan it would run is refused, so the setting is not
    applied (header, "HDR domain") -- the bytes of the apply without it"""
    torch = gpu
    from openvr_fsr_amd import _capi as K
    c = SC.BY_ID["iso-min-46"]
    iw, ih, _, _ = c.shape
    assert SC.RGBA16F in c.product and SC.RGBA32F not in c.product
    tex = torch.from_numpy((_imageh(iw, ih, 0).astype(np.float32) * np.float32(3)).astype(np.float16)).cuda()   # values up to 3: the mapping would show
    with_setting = _apply_once(torch, c.shape, tex, torch.float16, hdr=K.HDR_DOMAIN_SRTM)
    without = _apply_once(torch, c.shape, tex, torch.float16)
    assert np.array_equal(with_setting.view(np.uint16), without.view(np.uint16)) and without.any()


@pytest.mark.parametrize("cid", REFUSED_IDS)
def test_refusals_through_the_c_abi(gpu, cid):
    """each refusal of the table: the planned status and text from ovrfsr_apply; after ovrfsr_reset and an accepted size the ctx works again"""
    torch = gpu
    import openvr_fsr_amd as A
    c = SC.BY_ID[cid]
    iw, ih = c.shape[:2]
    ok = SC.BY_ID["steep-3x"]
    pp = A.PostProcessor(**_cfg(c.shape, 0))
    try:
        with pytest.raises(A.OvrFsrError) as e:
            pp.apply(0, torch.from_numpy(_image8(iw, ih, 0)).cuda(), out_dtype=torch.uint8)
        assert (e.value.status, str(e.value).split("): ", 1)[1]) == SC.REFUSED_LDS, cid
        with pytest.raises(A.OvrFsrError) as e:
            pp.apply(0, torch.from_numpy(_image8(iw, ih, 0)).cuda(), out_dtype=torch.uint8)
        assert e.value.status == 5, cid       # disabled after the failure
        pp.reset()
        pp.set_config(A.Config.default(**_cfg(ok.shape, 0)))
        got = pp.apply(0, torch.from_numpy(_image8(ok.shape[0], ok.shape[1], 0)).cuda(), out_dtype=torch.uint8)
        torch.cuda.synchronize()
        mx, _ = lsb_stats(got.cpu().numpy(), _want_pipeline(ok.shape, 0, 0))
        assert mx <= RCAS_LSB, (cid, mx)
    finally:
        pp.close()
    if c.strict:   # the asymmetry: the strict build plans what the product build refuses (tests/test_scale_regimes.py)
        assert cid in STRICT_IDS


# ---- the checked build -------------------------------------------------------------------------------------------------------------------------
def run_accepted_cases(torch):
    """the accepted cases through the product forms, unmasked and masked -> [(name, bytes equal to the contract)]: the child's work"""
    out = []
    for c in SC.ACCEPTED:
        for masked in (0, 1):
            shape = _shape(c, masked)
            want8 = O.float_to_unorm8(np.stack([_want_easu(shape, masked, i) for i in (0, 1)]))
            out.append(("%s/%d/easu" % (c.id, masked), np.array_equal(_frames(torch, shape, masked, stage_mask=1), want8)))
            want = np.stack([_want_pipeline(shape, masked, i) for i in (0, 1)])
            for form, cfg in _pipeline_forms(c, masked):
                out.append(("%s/%d/%s" % (c.id, masked, form), lsb_stats(_frames(torch, shape, masked, **cfg), want)[0] <= RCAS_LSB))
        if c.id in SC.HALF_IDS:
            got = _frames(torch, c.masked_shape, 1, src="rgba16f")
            err = np.abs(got.astype(np.float32) - np.stack([_want_half(c.masked_shape, 1, i) for i in (0, 1)]).astype(np.float32))
            out.append(("%s/half" % c.id, bool((err <= 1e-3).mean() >= 0.999 and err.max() <= 2e-2)))
    return out


_CHILD = r"""
import ctypes, sys
sys.path.insert(0, %r)
import numpy as np
import torch
import openvr_fsr_amd as A
from tests import test_gpu_scale_regimes as T
lib = A.library()
n = lib.ovrfsr_debug_bounds_slots()
buf = (ctypes.c_ulonglong * n)()
lib.ovrfsr_debug_bounds.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.c_int]
assert lib.ovrfsr_debug_bounds(buf, n, 1) == 0
results = T.run_accepted_cases(torch)
bad = [name for name, ok in results if not ok]
torch.cuda.synchronize()
assert lib.ovrfsr_debug_bounds(buf, n, 0) == 0
nk = (n - 5) // 3
v = list(buf)
print("scale regimes checked: calls %%d, mismatches %%d %%s, checked %%d, out of bounds %%d" %% (len(results), len(bad), bad, sum(v[2 * nk:3 * nk]), sum(v[:nk])))
"""


def test_checked_build(gpu):
    """the accepted cases against the -DOVRFSR_BOUNDS build -- the largest LDS planes any test stages: every access through the checked
    accessors, 0 out of bounds, and the bytes still within their contract (a wrongly redirected access would corrupt them)"""
    from tests.variants import variant
    lib = variant("bounds", "-DOVRFSR_BOUNDS")
    env = dict(os.environ, OVRFSR_LIB=lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    m = re.search(r"scale regimes checked: calls (\d+), mismatches (\d+) .*, checked (\d+), out of bounds (\d+)", r.stdout)
    assert r.returncode == 0 and m, (r.stdout[-1500:], r.stderr[-1500:])
    assert int(m.group(1)) >= 4 * len(SC.ACCEPTED) and int(m.group(2)) == 0 and int(m.group(3)) > 1e6 and int(m.group(4)) == 0, m.group(0)
