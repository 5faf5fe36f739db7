"""The NIS CPU oracle (oracle/nis_oracle.c) against the reference's own NIS_Scaler.h.  No GPU needed."""
import json
import os

import numpy as np
import pytest

import openvr_fsr_amd as A
from oracle import oracle as O
from tests import nis_cases, refgold, synth

HERE = os.path.dirname(os.path.abspath(__file__))
V = np.load(os.path.join(HERE, "golden", "nis_vectors.npz"))
META = json.loads(bytes(V["meta"]).decode())


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("m", META, ids=lambda m: m["name"])
def test_nis_oracle_matches_golden(m):
    name = m["name"]
    img = O.unorm8_to_float(V[name + "_in"])
    cs, cu = A.nis_coefs()            # the product's committed tables (checked against the reference elsewhere)
    ow, oh = m["out"]
    # the constant block is rebuilt by the PRODUCT's host code and must equal what the reference uploaded
    ok, cfg = A.nis_scaler_config(m["sharpness"], m["in"][0], m["in"][1], ow, oh)
    centre, rad = O.mask_constants(ow, oh, m["radius"], m["proj"], True, m["eye"])
    blk = O.nis_block(cfg, centre, rad, m["debug"])
    assert np.array_equal(blk, V[name + "_blk_upscale"])
    assert same_bits(O.nis_upscale(img, ow, oh, blk, cs, cu), V[name + "_upscale"])
    ok2, cfg2 = A.nis_sharpen_config(m["sharpness"], m["in"][0], m["in"][1])
    c2, r2 = O.mask_constants(m["in"][0], m["in"][1], m["radius"], m["proj"], True, m["eye"])
    blk2 = O.nis_block(cfg2, c2, r2, m["debug"])
    assert np.array_equal(blk2, V[name + "_blk_sharpen"])
    assert same_bits(O.nis_sharpen(img, blk2), V[name + "_sharpen"])


@pytest.mark.parametrize("seed", range(5))
def test_nis_oracle_matches_reference_random(seed):
    rng = np.random.default_rng(100 + seed)
    cs, cu = refgold.ref_nis_coefs()
    w, h = int(rng.integers(16, 90)), int(rng.integers(16, 90))
    gen = [synth.structured_u8, synth.random_u8, synth.extremes_u8][seed % 3]
    src = O.unorm8_to_float(gen(w, h, seed))
    sharp = float(rng.uniform(0, 1))
    s = rng.uniform(0.5, 1.0)
    ow, oh = int(w / s), int(h / s)
    ok, cfg = refgold.ref_nis_scaler_config(sharp, w, h, ow, oh)
    assert ok
    centre, rad = O.mask_constants(ow, oh, float(rng.uniform(0.3, 1.5)), tuple(rng.uniform(0.3, 0.7, 4)), True, seed & 1)
    blk = O.nis_block(cfg, centre, rad, seed & 1)
    key = "nis_random/%d/" % seed
    assert refgold.same_as_reference(key + "nis_upscale", O.nis_upscale(src, ow, oh, blk, cs, cu), lambda: O.ref_nis_upscale(src, ow, oh, blk, cs, cu))
    ok, cfg = refgold.ref_nis_scaler_config(sharp, w, h, w, h)
    centre, rad = O.mask_constants(w, h, float(rng.uniform(0.3, 1.5)), tuple(rng.uniform(0.3, 0.7, 4)), True, seed & 1)
    blk = O.nis_block(cfg, centre, rad, seed & 1)
    assert refgold.same_as_reference(key + "nis_sharpen", O.nis_sharpen(src, blk), lambda: O.ref_nis_sharpen(src, blk, cs, cu))


def test_nis_invariants():
    cs, cu = A.nis_coefs()
    w, h, ow, oh = 40, 30, 60, 45
    ok, cfg = A.nis_scaler_config(0.9, w, h, ow, oh)
    centre, rad = O.mask_constants(ow, oh, 2.0)
    blk = O.nis_block(cfg, centre, rad)
    # constant image is a fixed point (polyphase rows sum to 1, USM rows to 0, edge maps all zero)
    const = np.empty((h, w, 4), np.float32)
    const[...] = np.array([0.25, 0.5, 0.75, 1.0], np.float32)
    out = O.nis_upscale(const, ow, oh, blk, cs, cu)
    np.testing.assert_allclose(out, np.broadcast_to(const[0, 0], out.shape), atol=3e-3)
    # outputs are clamped to [0,1] by the unorm UAV; alpha is the sampled alpha
    img = O.unorm8_to_float(synth.extremes_u8(w, h, 2))
    out = O.nis_upscale(img, ow, oh, blk, cs, cu)
    assert out.min() >= 0.0 and out.max() <= 1.0 and (out[..., 3] == 1.0).all()


@pytest.mark.parametrize("seed", [6, 13, 20])
def test_oracle_matches_reference_on_non_finite_texels(seed):
    """NaN / +-Inf / 1e30 texels (outside the parity contract of the LIBRARY, header "TEXEL VALUES") still have one answer in the reference's
    arithmetic, and the restatement gives it: the round-6 pin campaign (tests/debug/oracle_pin_campaign.py) found the single shortcut only such
    texels can see -- NIS luma tiles loaded as texels instead of through SampleLevel at texel centres, where a NaN neighbour enters as 0 x NaN --
    and this keeps it closed, for EASU / RCAS / NVScaler / NVSharpen.  Two NaNs compare equal whatever their payload."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "debug"))
    import oracle_pin_campaign as P
    rng = np.random.default_rng(seed)
    iw, ih = int(rng.integers(20, 90)), int(rng.integers(20, 90))
    ow, oh = int(iw / 0.75), int(ih / 0.75)
    img = P.content(6, iw, ih, seed, rng)
    assert np.isnan(img).any() and np.isinf(img).any()
    cs, cu = refgold.ref_nis_coefs()
    centre, rad = O.mask_constants(ow, oh, 2.0)
    con = O.easu_con(iw, ih, ow, oh)
    a = O.easu(img, ow, oh, con, centre, rad)
    key = "non_finite/%d/" % seed
    assert refgold.same_as_reference(key + "easu", a, lambda: O.ref_easu(img, ow, oh, con, centre, rad), nan_equal=True)
    rcon = O.rcas_con(0.6, 0)
    assert refgold.same_as_reference(key + "rcas", O.rcas(a, rcon, centre, rad), lambda: O.ref_rcas(a, rcon, centre, rad), nan_equal=True)
    ok, cfg = refgold.ref_nis_scaler_config(0.5, iw, ih, ow, oh)
    assert ok
    blk = O.nis_block(cfg, centre, rad, 0)
    assert refgold.same_as_reference(key + "nis_upscale", O.nis_upscale(img, ow, oh, blk, cs, cu), lambda: O.ref_nis_upscale(img, ow, oh, blk, cs, cu),
                                     nan_equal=True)
    ok, cfg = refgold.ref_nis_scaler_config(0.5, iw, ih, iw, ih)
    c2, r2 = O.mask_constants(iw, ih, 2.0)
    blk = O.nis_block(cfg, c2, r2, 0)
    assert refgold.same_as_reference(key + "nis_sharpen", O.nis_sharpen(img, blk), lambda: O.ref_nis_sharpen(img, blk, cs, cu), nan_equal=True)


def _pin_float(key, img, ow, oh, radius, debug, check_share):
    """NVScaler to ow x oh and NVSharpen at the input size on one float image: the restatement against the reference's compiled code"""
    ih, iw = img.shape[:2]
    cs, cu = refgold.ref_nis_coefs()
    ok, cfg = refgold.ref_nis_scaler_config(0.6, iw, ih, ow, oh)
    assert ok
    centre, rad = O.mask_constants(ow, oh, radius, nis_cases.PROJ, True, 1)
    blk = O.nis_block(cfg, centre, rad, debug)
    up = O.nis_upscale(img, ow, oh, blk, cs, cu)
    assert not np.isnan(up).any()
    if check_share:
        nis_cases.assert_informative(up, key + "nis_upscale")
    assert refgold.same_as_reference(key + "nis_upscale", up, lambda: O.ref_nis_upscale(img, ow, oh, blk, cs, cu))
    ok, cfg = refgold.ref_nis_scaler_config(0.6, iw, ih, iw, ih)
    assert ok
    centre, rad = O.mask_constants(iw, ih, radius, nis_cases.PROJ, True, 1)
    blk = O.nis_block(cfg, centre, rad, debug)
    sh = O.nis_sharpen(img, blk)
    assert not np.isnan(sh).any()
    if check_share:
        nis_cases.assert_informative(sh, key + "nis_sharpen")
    assert refgold.same_as_reference(key + "nis_sharpen", sh, lambda: O.ref_nis_sharpen(img, blk, cs, cu))


@pytest.mark.parametrize("radius,debug", [(2.0, 0), (0.5, 1)])
@pytest.mark.parametrize("iw,ih,ow,oh", nis_cases.SHAPES)
@pytest.mark.parametrize("kind", list(nis_cases.KINDS))
def test_nis_oracle_matches_reference_on_float_content(kind, iw, ih, ow, oh, radius, debug):
    """Finite texels outside the unit range -- highlights tens of times their neighbours, negative values -- through NVScaler and NVSharpen:
    where the [0, 1] clamp of the `unorm` store, GetEdgeMap's thresholds and the USM limit see something colour content never shows them.
    The images are the ones tests/test_gpu_nis_formats.py submits as RGBA16F / RGBA32F, so the yardstick of those GPU comparisons is itself
    pinned to the reference here.  At least a quarter of the oracle's colour values must lie strictly inside (0, 1): a clamped value says
    nothing about the arithmetic in front of the clamp."""
    img = nis_cases.image(kind, iw, ih)
    _pin_float("nis_float/%s/%dx%d-%dx%d/r%gd%d/" % (kind, iw, ih, ow, oh, radius, debug), img, ow, oh, radius, debug, True)


@pytest.mark.parametrize("kind", synth.WILD_FINITE)
def test_nis_oracle_matches_reference_on_wild_finite_texels(kind):
    """The finite families of tests/test_gpu_formats.py::test_texel_value_domain (half extremes, negative values, fp32 denormals, 1e18, zeros
    of both signs): nearly every output is clamped, so this guards the clamp and sign decisions of the restatement and little else."""
    iw, ih, ow, oh = 61, 47, 80, 63
    img = synth.wild_f32(kind, iw, ih, np.random.default_rng(50))
    _pin_float("nis_wild/%s/" % kind, img, ow, oh, 2.0, 0, False)


@pytest.mark.parametrize("w,h", [(128, 107), (83, 83), (96, 40)])
def test_flat_rectangle_reaches_the_no_edge_shortcut(w, h):
    """The condition tests/test_gpu_nis_formats.py::test_nvsharpen_float_source rests on, checked on the oracle's side (reference tables and
    constant block: no product library involved): inside synth.FLAT_RECT, away from its border, NVSharpen's output IS the input clamped to
    [0, 1] (no edge in the 3 x 3 map of a flat 5 x 5 neighbourhood, so no USM term) -- over whole aligned 32 x 2 spans, which is what a wave
    of the product build needs to take its no-edge shortcut.  The "signed" rectangle holds a value below 0 and one above 1: the shortcut's
    clamp has something to do."""
    rx, ry, rw, rh = synth.FLAT_RECT
    assert rx == 0 and rw >= 66 and ry % 2 == 0 and rh >= 6 and w >= rw and h >= ry + rh
    span = (slice(ry + 2, ry + rh - 2), slice(0, 64))      # columns 0..63 read columns 0..65, these rows read rows ry .. ry + rh - 1
    ok, cfg = refgold.ref_nis_scaler_config(0.75, w, h, w, h)
    assert ok
    centre, rad = O.mask_constants(w, h, 2.0)
    blk = O.nis_block(cfg, centre, rad, 0)
    for kind in nis_cases.KINDS:
        img = nis_cases.image(kind, w, h)
        flat = img[span][..., :3].reshape(-1, 3)
        assert len(np.unique(flat, axis=0)) == 1
        assert ((flat.min() < 0) and (flat.max() > 1)) == (kind == "signed")
        assert same_bits(O.nis_sharpen(img, blk)[span], np.clip(img[span], np.float32(0), np.float32(1))), kind
