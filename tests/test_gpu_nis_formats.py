"""NVScaler and NVSharpen on FLOAT eye images (RGBA16F, RGBA32F, R11G11B10F) against the CPU oracle.

A float source takes code an RGBA8 source never runs: nis_scaler_kernel's clamped per-texel staging loop, its generic chroma tap
(bilinear_uv<IN_FMT> from global memory) and its luma correction in the unit domain; nis_outside_kernel for the groups outside a radius;
the load_unit / store_unit branch of nis_sharpen_kernel's no-edge shortcut.  Every other NIS test on a float source compares one GPU path
with another (packed against RGBA16F, multisampled against resolved, rule on against rule off); the comparisons here end at the oracle, and
tests/test_oracle_nis.py pins the oracle to the reference's compiled NVScaler / NVSharpen on the very images used here.

Content (tests/nis_cases.py, synth.hdr_f32): unit range, sparse highlights at 40, signed values in [-2, 2] -- texels exactly representable in
half, so one image is both an RGBA16F and an RGBA32F submission against one oracle result.  NIS clamps every output to [0, 1]: each
comparison first asserts that at least a quarter of the ORACLE's colour values lie strictly inside (0, 1).

Contract:
  strict build   bit-exact: RGBA32F = the oracle's words, RGBA16F = oracle.astype(float16), RGBA8 = float_to_unorm8(oracle)
  product build  RGBA32F within NIS_FLOAT_TOL * max(1, scale of the content); RGBA16F the same plus one half spacing; RGBA8 within 1 LSB;
                 no NaN; pixels of DirectCopy groups (wholly outside the radius) bit-identical to the oracle
Every product-build comparison is recorded in reports/nis_float_formats.json at the repository root (git ignores reports/; OVRFSR_REPORT_DIR
names another directory, for a run whose outputs are collected elsewhere) and held against a regression alarm derived from that record.
The committed copy of the measuring run is profiles/nis_float_formats.json."""
import functools
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import nis_cases as N
from tests import packedf, synth
from tests.test_gpu_fuzz import _outside_px
from tests.test_gpu_parity import NIS_FLOAT_TOL

pytestmark = pytest.mark.gpu
STRICT, FP32 = 2, 0
BUILDS = (("strict", STRICT), ("product", FP32))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = {"rgba16f": np.float16, "rgba32f": np.float32}
DESTS = (("rgba8", np.uint8), ("rgba16f", np.float16), ("rgba32f", np.float32))
HALF_SPACING = 2.0 ** -11    # of the largest binade a clamped output occupies, [0.5, 1)

# Regression alarms, NOT the contract (the asserts beside them are): 8x the largest value the first MI355X run of this file recorded for
# the product build against the oracle (profiles/nis_float_formats.json, 244 records) -- inside the 4-10x band of
# tests/test_gpu_parity_report.py, towards its upper end because these images hold ~1e4 pixels and their maxima are noisier than a
# full-size image's.
#   float alarm, per content kind, from the RGBA32F destinations.  Measured largest max_abs: unit 4.17e-7, highlights 9.54e-7,
#     signed 3.28e-7 (NVScaler; NVSharpen 1.2e-7, masked NVScaler 4.8e-7).  An RGBA16F destination adds its rounding on top (measured
#     2.44e-4 = 2^-12 for every kind, the rounding alone): it is held to the same alarm plus HALF_SPACING, as the contract is.
#   differing-byte alarm, from the RGBA8 destinations.  Measured largest n_diff / n_total: 9.92e-5 (2 of the 20 160 bytes of an 80 x 63
#     image; 0 for NVSharpen and for the masked 200 x 160 cases); max_lsb 1.
MEASURED_FLOAT = {"unit": 4.2e-7, "highlights": 9.6e-7, "signed": 3.3e-7}
MEASURED_DIFF_BYTES = 1.0e-4
FLOAT_ALARM = {k: 8 * v for k, v in MEASURED_FLOAT.items()}      # 3.4e-6, 7.7e-6, 2.6e-6: 130-380 times inside the contract
DIFF_BYTES_ALARM = 8 * MEASURED_DIFF_BYTES                       # 8e-4 of an image's bytes
_RECORDS = []


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    if not _RECORDS:
        return
    out_dir = os.environ.get("OVRFSR_REPORT_DIR") or os.path.join(ROOT, "reports")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "nis_float_formats.json"), "w") as f:
        json.dump({"note": "NVScaler / NVSharpen on float sources, product build vs CPU oracle; written by tests/test_gpu_nis_formats.py",
                   "measured": _maxima(_RECORDS),
                   "alarms": {"rule": "8x the maxima of the first MI355X run (MEASURED_* in the test file)", "float_rgba32f": FLOAT_ALARM,
                              "float_rgba16f": {k: v + HALF_SPACING for k, v in FLOAT_ALARM.items()},
                              "float_rgba16f_rule": "the RGBA32F alarm plus one half spacing (2^-11), as the contract adds it",
                              "differing_bytes": DIFF_BYTES_ALARM},
                   "records": _RECORDS}, f, indent=1)


def _maxima(records):
    """what the alarms are derived from: per kind the largest RGBA32F and RGBA16F max_abs, and the largest share of differing bytes"""
    out = {"float_rgba32f": {}, "float_rgba16f": {}, "differing_bytes": 0.0, "max_lsb": 0}
    for r in records:
        if r["max_abs"] is not None:
            d = out["float_" + r["destination"]]
            d[r["kind"]] = max(d.get(r["kind"], 0.0), r["max_abs"])
        else:
            out["differing_bytes"] = max(out["differing_bytes"], r["n_diff"] / r["n_total"])
            out["max_lsb"] = max(out["max_lsb"], r["max_lsb"])
    return out


def _run(src, ow, oh, out_dt, eye=0, in_format=None, **cfg):
    """one ovrfsr_apply on a fresh ctx, caller-owned output -> numpy"""
    import torch
    import openvr_fsr_amd as A
    kw = dict(fsr_enabled=1, use_nis=1, out_width=ow, out_height=oh, radius=2.0)
    kw.update(cfg)
    pp = A.PostProcessor(**kw)
    try:
        tdt = {np.uint8: torch.uint8, np.float16: torch.float16, np.float32: torch.float32}[out_dt]
        out = pp.apply(eye, torch.from_numpy(np.ascontiguousarray(src)).cuda(), out_dtype=tdt, in_format=in_format)
        torch.cuda.synchronize()
        return out.cpu().numpy()
    finally:
        pp.close()


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _image(kind, w, h, seed=N.SEED):
    return _frozen(N.image(kind, w, h, seed))


@functools.lru_cache(maxsize=None)
def _want_scaler(kind, iw, ih, ow, oh, sharp, radius, proj, eye, debug, seed=N.SEED):
    want = N.want_scaler(_image(kind, iw, ih, seed), ow, oh, sharp, radius, proj, eye, debug)
    N.assert_informative(want, "NVScaler %s %dx%d -> %dx%d" % (kind, iw, ih, ow, oh))
    return _frozen(want)


@functools.lru_cache(maxsize=None)
def _want_sharpen(kind, w, h, sharp, radius, proj, eye, debug):
    want = N.want_sharpen(_image(kind, w, h), sharp, radius, proj, eye, debug)
    N.assert_informative(want, "NVSharpen %s %dx%d" % (kind, w, h))
    return _frozen(want)


def _same_words(got, want):
    u = {1: np.uint8, 2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    return np.ascontiguousarray(got).view(u) == np.ascontiguousarray(want).view(u)


def _compare(test, kind, source, dest, shape, build, got, want, exact=None, config=""):
    """One output against the oracle's float result `want`, by the module's contract; `exact`: bool [H, W] of pixels that must be
    bit-identical in the product build too (DirectCopy groups).  Product-build comparisons are recorded."""
    dt = got.dtype.type
    assert got.shape == want.shape, (got.shape, want.shape)
    ref = O.float_to_unorm8(want) if dt == np.uint8 else want.astype(dt)
    same = _same_words(got, ref)
    tag = (test, kind, source, dest, shape, build, config)
    if build == "strict":
        assert same.all(), (tag, "%d values differ from the oracle" % int((~same).sum()))
        return
    r = {"test": test, "config": config, "kind": kind, "source": source, "destination": dest, "shape": list(shape),
         "max_abs": None, "max_lsb": None, "n_diff": int((~same).sum()), "n_total": int(same.size)}
    scale = max(1.0, N.KINDS[kind])
    if dt == np.uint8:
        d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
        r["max_lsb"] = int(d.max())
    else:
        g32 = got.astype(np.float32)
        assert not np.isnan(g32).any(), tag
        r["max_abs"] = float(np.abs(g32 - want).max())     # against the oracle's fp32 result: an RGBA16F output's includes its rounding
    _RECORDS.append(r)
    print("nis float formats:", json.dumps(r))
    if exact is not None:
        assert same[exact].all(), (tag, "%d values of DirectCopy groups differ from the oracle" % int((~same[exact]).sum()))
    if dt == np.uint8:
        assert r["max_lsb"] <= 1, r
        assert r["n_diff"] <= DIFF_BYTES_ALARM * r["n_total"], ("regression alarm", r)
    else:
        extra = HALF_SPACING if dt == np.float16 else 0.0
        assert r["max_abs"] <= NIS_FLOAT_TOL * scale + extra, r
        assert r["max_abs"] <= FLOAT_ALARM[kind] + extra, ("regression alarm", r)


def _all_builds_and_dests(test, kind, source, shape, want, run, exact=None, config=""):
    for dest, ddt in DESTS:
        for build, prec in BUILDS:
            _compare(test, kind, source, dest, shape, build, run(ddt, prec), want, exact, config)


# ---- (a) NVScaler, unmasked -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("iw,ih,ow,oh", N.SHAPES)
@pytest.mark.parametrize("kind", list(N.KINDS))
@pytest.mark.parametrize("source", list(SOURCES))
def test_nvscaler_float_source(gpu, source, kind, iw, ih, ow, oh):
    """Pitch 32 with a ragged right / bottom edge, 2x (the 6x6 form without the V plane in every build), pitch 40, odd sizes: the oracle
    result is the one tests/test_oracle_nis.py pins to the reference (sharpness 0.6, off-centre projection, right eye)."""
    want = _want_scaler(kind, iw, ih, ow, oh, 0.6, 2.0, N.PROJ, 1, 0)
    src = _image(kind, iw, ih).astype(SOURCES[source])
    _all_builds_and_dests("NVScaler", kind, source, (iw, ih, ow, oh), want,
                          lambda ddt, prec: _run(src, ow, oh, ddt, eye=1, precision=prec, sharpness=0.6, proj_centre=N.PROJ))


# ---- (b) NVSharpen ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("w,h", [(128, 107), (83, 83), (96, 40)])
@pytest.mark.parametrize("kind", list(N.KINDS))
@pytest.mark.parametrize("source", list(SOURCES))
def test_nvsharpen_float_source(gpu, source, kind, w, h):
    """Render scale 1.  Every size here holds synth.FLAT_RECT, so waves of the product build take the no-edge shortcut on a float source
    (tests/test_oracle_nis.py::test_flat_rectangle_reaches_the_no_edge_shortcut checks the condition at these sizes); for the `signed` kind
    the rectangle holds a value below 0 and one above 1, so the clamp of the shortcut's own store is compared too.  With radius 0.6 the
    groups outside take DirectCopy with the debug tint."""
    src = _image(kind, w, h).astype(SOURCES[source])
    for radius, debug in ((2.0, 0), (0.6, 1)):
        want = _want_sharpen(kind, w, h, 0.75, radius, N.PROJ, 1, debug)
        _all_builds_and_dests("NVSharpen", kind, source, (w, h, w, h), want,
                              lambda ddt, prec: _run(src, w, h, ddt, eye=1, precision=prec, render_scale=1.0, sharpness=0.75, radius=radius,
                                                     proj_centre=N.PROJ, debug_mode=debug),
                              config="radius %g debug %d" % (radius, debug))


# ---- (c) NVScaler with a radius ------------------------------------------------------------------------------------------------

MASKED = (150, 120, 200, 160)
MASKS = ((0.5, (0.5,) * 4, 0, 0), (0.62, (0.42, 0.55, 0.61, 0.47), 1, 1))   # radius, proj, eye, debug


@pytest.mark.parametrize("radius,proj,eye,debug", MASKS, ids=["radius 0.5 centred", "radius 0.62 off-centre debug"])
@pytest.mark.parametrize("kind", ["highlights", "signed"])
@pytest.mark.parametrize("source", list(SOURCES))
def test_nvscaler_float_source_masked(gpu, source, kind, radius, proj, eye, debug):
    """A masked float submission is, with R10G10B10A2, the only user of nis_outside_kernel<I, O> (the staged outside kernel takes RGBA8
    sources only).  DirectCopy has no contraction-sensitive step and the kernel blends with bilerp_unfused: the pixels of 32 x 24 groups
    wholly outside the radius are the oracle's bit for bit in the product build too, for every destination."""
    iw, ih, ow, oh = MASKED
    want = _want_scaler(kind, iw, ih, ow, oh, 0.6, radius, proj, eye, debug)
    centre, rad = O.mask_constants(ow, oh, radius, proj, True, eye)
    outside = _outside_px(ow, oh, centre, rad[1], 32, 24)
    assert 0.2 <= outside.mean() <= 0.9, "the case must hold both kinds of group"
    src = _image(kind, iw, ih).astype(SOURCES[source])
    _all_builds_and_dests("NVScaler masked", kind, source, MASKED, want,
                          lambda ddt, prec: _run(src, ow, oh, ddt, eye=eye, precision=prec, sharpness=0.6, radius=radius, proj_centre=proj,
                                                 debug_mode=debug),
                          exact=outside, config="radius %g debug %d" % (radius, debug))


@pytest.mark.parametrize("source", list(SOURCES))
def test_nvscaler_float_source_masked_batch(gpu, source):
    """ovrfsr_apply_batch of four float images, eyes alternating R, L, R, L with unequal eye centres (each eye its own group lists): every
    image against the oracle, and image 0 equal to the same image submitted on its own."""
    import torch
    import openvr_fsr_amd as A
    iw, ih, ow, oh = MASKED
    radius, proj, _, debug = MASKS[1]
    kinds = ["highlights", "signed", "signed", "highlights"]
    imgs = [_image(k, iw, ih, N.SEED + i) for i, k in enumerate(kinds)]
    src = torch.from_numpy(np.stack(imgs).astype(SOURCES[source])).cuda()
    for dest, ddt in DESTS:
        tdt = {np.uint8: torch.uint8, np.float16: torch.float16, np.float32: torch.float32}[ddt]
        for build, prec in BUILDS:
            pp = A.PostProcessor(fsr_enabled=1, use_nis=1, out_width=ow, out_height=oh, sharpness=0.6, radius=radius, proj_centre=proj,
                                 debug_mode=debug, precision=prec)
            try:
                outs = torch.zeros((4, oh, ow, 4), dtype=tdt, device="cuda")
                pp.apply_batch(src, outs, first_eye=A.EYE_RIGHT, alternate_eyes=True)
                torch.cuda.synchronize()
                got = outs.cpu().numpy()
                one = pp.apply(A.EYE_RIGHT, src[0], out_dtype=tdt)
                torch.cuda.synchronize()
                assert _same_words(one.cpu().numpy(), got[0]).all(), (dest, build, "image 0 of the batch differs from its single apply")
            finally:
                pp.close()
            for i, k in enumerate(kinds):
                eye = 1 ^ (i & 1)
                want = _want_scaler(k, iw, ih, ow, oh, 0.6, radius, proj, eye, debug, N.SEED + i)
                centre, rad = O.mask_constants(ow, oh, radius, proj, True, eye)
                _compare("NVScaler masked batch", k, source, dest, MASKED, build, got[i], want, _outside_px(ow, oh, centre, rad[1], 32, 24),
                         "image %d of 4, eye %d" % (i, eye))


# ---- (d) the chains that ended at a GPU-to-GPU equality ---------------------------------------------------------------------------


@pytest.mark.parametrize("iw,ih,ow,oh", [(96, 80, 128, 107), (61, 47, 80, 63)])
def test_packed_float_source_and_reference_formats(gpu, iw, ih, ow, oh):
    """R11G11B10F holding the `highlights` values (truncated to the format's codes): NVScaler against the oracle of the DECODED values --
    tests/test_gpu_packed_float.py only shows it equal to the RGBA16F route.  Then the same submission under cfg.reference_formats = 1 with
    a ctx-owned output: the output is RGBA8 and holds the oracle's bytes (tests/test_gpu_reference_formats.py compares NIS rule on against
    rule off only)."""
    import openvr_fsr_amd as A
    from tests import test_gpu_reference_formats as T
    packed = packedf.encode(_image("highlights", iw, ih))
    decoded = packedf.unpack(packed).astype(np.float32)
    cs, cu = A.nis_coefs()
    ok, cfg = A.nis_scaler_config(0.6, iw, ih, ow, oh)
    assert ok
    for radius in (2.0, 0.5):
        centre, rad = O.mask_constants(ow, oh, radius, N.PROJ, True, 1)
        want = O.nis_upscale(decoded, ow, oh, O.nis_block(cfg, centre, rad, 0), cs, cu)
        N.assert_informative(want, "NVScaler on the decoded R11G11B10F image")
        outside = _outside_px(ow, oh, centre, rad[1], 32, 24)
        kw = dict(sharpness=0.6, radius=radius, proj_centre=N.PROJ)
        _all_builds_and_dests("NVScaler R11G11B10F", "highlights", "r11g11b10f", (iw, ih, ow, oh), want,
                              lambda ddt, prec: _run(packed, ow, oh, ddt, eye=1, in_format=A.FORMAT_R11G11B10F, precision=prec, **kw),
                              exact=outside, config="radius %g" % radius)
        for build, prec in BUILDS:
            fmt, dt, own = T._apply_owned(packed, ow, oh, eye=1, use_nis=1, reference_formats=1, precision=prec, **kw)
            assert fmt == A.FORMAT_RGBA8 and own.dtype == np.uint8, (fmt, dt)
            _compare("NVScaler R11G11B10F, reference_formats, ctx-owned output", "highlights", "r11g11b10f", "rgba8", (iw, ih, ow, oh), build,
                     own, want, outside, "radius %g" % radius)


# ---- (e) the texel-value domain ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", synth.WILD_FINITE)
def test_nis_texel_value_domain(gpu, kind):
    """The finite families of test_gpu_formats.py::test_texel_value_domain -- half extremes, negative values, fp32 denormals, 1e18, zeros of
    both signs -- through NVScaler and NVSharpen as RGBA32F: the strict build bit-identical to the oracle (for the family with zeros of both
    signs, and for it only, a result that is a zero may carry the other sign: min / max of +0 and -0 is open in IEEE 754), the product build
    finite.
    On the CPU NVScaler's oracle output for these families has NO colour value strictly inside (0, 1), and NVSharpen's has 0-19 %: this case
    guards the clamp and sign decisions and little else -- the power is in the tests above.  The NaN / Inf family is left out: the header
    puts it outside the parity contract, and whether a NaN saturates to 0 is not something the two sides must agree on."""
    iw, ih, ow, oh = 150, 110, 200, 147
    for seed in (50, 51):
        img = synth.wild_f32(kind, iw, ih, np.random.default_rng(seed))
        cases = (("NVScaler", N.want_scaler(img, ow, oh, 0.6), dict(sharpness=0.6), ow, oh),
                 ("NVSharpen", N.want_sharpen(img, 0.75), dict(sharpness=0.75, render_scale=1.0), iw, ih))
        for name, want, kw, w, h in cases:
            assert np.isfinite(want).all()
            got = _run(img, w, h, np.float32, precision=STRICT, **kw)
            same = _same_words(got, want)
            if kind == "zeros of both signs":
                same |= (got == 0) & (want == 0)
            assert same.all(), (kind, name, seed, int((~same).sum()))
            assert np.isfinite(_run(img, w, h, np.float32, precision=FP32, **kw)).all(), (kind, name, seed)
