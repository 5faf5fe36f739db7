"""The radius mask with its disc on the image's edge, on a corner, half off it or off it altogether (ovrfsr_set_gaze accepts [-1, 2]), without a
GPU: the planner's mask modes, tile sets, ring and RCAS spans against tests/mask_ref.py -- the per-group rule restated once in numpy from the
ORACLE's mask constants -- for every row of the case table there and every variant of tests/test_pipeline_plan.py.  The plans are read through
tests/debug/hidden_probe.cpp with no mesh: a stand-alone program, compiled on the fly with the planner units under ASan + UBSan and run as a
child process.  mask_ref itself is checked against the oracle's own pixels first: the pixels a mask changes all lie in groups it calls outside,
and the debug tint the oracle restates marks exactly its outside pixels."""
import shutil

import numpy as np
import pytest

from oracle import oracle as O
from tests import hidden_ref as R
from tests import mask_ref as MR
from tests import synth
from tests import test_pipeline_plan as TP

CASE_IDS = [c.id for c in MR.CASES]


@pytest.fixture(scope="module")
def plans():
    """{(case id, variant name): the probe's record} for the whole table, one run of the probe"""
    run = R.build_probe()
    try:
        keys, lines = [], []
        for c in MR.CASES:
            iw, ih, ow, oh = c.shape
            for name, fmt, one_eye, cfg in TP.VARIANTS:
                keys.append((c.id, name))
                line = TP._line("%s/%s" % (c.id, name), fmt, iw, ih, one_eye, -1, fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, radius=c.radius,
                                proj_centre=c.proj, **cfg)
                lines.append(R.with_mesh(line))
        return dict(zip(keys, run(lines)))
    finally:
        shutil.rmtree(run.tmp, ignore_errors=True)


# ---- the table is what it says it is ---------------------------------------------------------------------------------------------------
def test_every_class_of_the_table_is_present():
    assert {c.klass for c in MR.CASES} == {"corner", "negative", "sliver", "one-group", "all-outside", "one-eye-out", "nearly-all", "one-group-fsr",
                                           "radius-0", "shared"}
    assert len(set(CASE_IDS)) == len(CASE_IDS)
    for klass in {c.klass for c in MR.CASES}:
        assert any(c.shape == MR.S3 for c in MR.CASES if c.klass == klass), klass   # every class at the shape with partial tiles and groups


@pytest.mark.parametrize("cid", CASE_IDS)
def test_class_property(cid):
    MR.class_property(MR.BY_ID[cid])


def test_the_uint32_arithmetic_wraps():
    """a centre left of a group centre gives a difference near 2^32 whose square, modulo 2^32, is the square of the distance; a distance of
    65536 squares to 0 and is `inside` any radius: the rule as the shader computes it, not as geometry would"""
    g = MR.group_map([0, 0, 0, 0], [3, 9, 32, 32], 16, 16)       # distance^2 = 128 > 9 everywhere, although (0 - 8) wraps
    assert not g.any()
    g = MR.group_map([65544, 8, 65544, 8], [0, 0, 16, 16], 16, 16)   # dx = 65536: dx^2 = 2^32 = 0 (mod 2^32) <= 0
    assert g.all()


# ---- mask_ref against the oracle's own pixels ------------------------------------------------------------------------------------------
ORACLE_CHECKED = ["corner-11-10-S3", "sliver-S3", "one-group-S3", "all-outside-S2", "radius-0-S1", "nearly-all-S2", "shared-left-2-S3"]


def _float_image(iw, ih, seed):
    """colour values in [0.2, 1]: a tint of 0.7 changes every pixel it touches"""
    return np.float32(0.2) + np.float32(0.8) * O.unorm8_to_float(synth.structured_u8(iw, ih, seed))


@pytest.mark.parametrize("cid", ORACLE_CHECKED)
def test_mask_ref_against_the_oracles_pixels(cid):
    import openvr_fsr_amd as A
    c = MR.BY_ID[cid]
    iw, ih, ow, oh = c.shape
    src = _float_image(iw, ih, 31)
    mid = _float_image(ow, oh, 32)
    cs, cu = A.nis_coefs()
    ok, ncfg = A.nis_scaler_config(0.9, iw, ih, ow, oh)
    assert ok
    ucentre, urad = O.mask_constants(ow, oh)       # the unmasked call: radius 2 about the middle
    assert MR.MaskRef(ucentre, urad, 16, 16).mode == MR.ALL_INSIDE and MR.MaskRef(ucentre, urad, 32, 24).mode == MR.ALL_INSIDE
    for eye in c.eyes():
        fsr, nis = c.ref(eye), c.ref(eye, "nvscaler")
        centre, rad = MR.constants(c.shape, c.radius, c.proj, c.one_eye, eye)
        # 1. what the mask changes lies in outside groups (single passes: RCAS's taps would carry an outside neighbour into an inside pixel)
        changed = (O.easu(src, ow, oh, None, centre, rad) != O.easu(src, ow, oh, None, ucentre, urad)).any(axis=2)
        assert not (changed & fsr.pixels).any() and (changed.any() or fsr.mode == MR.ALL_INSIDE), (cid, eye)
        changed = (O.rcas(mid, O.rcas_con(0.9), centre, rad) != O.rcas(mid, O.rcas_con(0.9), ucentre, urad)).any(axis=2)
        assert not (changed & fsr.pixels).any() and changed.any(), (cid, eye)
        changed = (O.nis_upscale(src, ow, oh, O.nis_block(ncfg, centre, rad), cs, cu) != O.nis_upscale(src, ow, oh, O.nis_block(ncfg, ucentre, urad), cs, cu)).any(axis=2)
        assert not (changed & nis.pixels).any() and (changed.any() or nis.mode != MR.MIXED), (cid, eye)
        # 2. the debug tint marks exactly the outside pixels
        tinted = (O.rcas(mid, O.rcas_con(0.9, 1), centre, rad) != O.rcas(mid, O.rcas_con(0.9, 0), centre, rad)).any(axis=2)
        assert np.array_equal(tinted, ~fsr.pixels), (cid, eye, int(tinted.sum()), int((~fsr.pixels).sum()))
        tinted = (O.nis_upscale(src, ow, oh, O.nis_block(ncfg, centre, rad, 1), cs, cu) != O.nis_upscale(src, ow, oh, O.nis_block(ncfg, centre, rad, 0), cs, cu)).any(axis=2)
        assert np.array_equal(tinted, ~nis.pixels), (cid, eye, int(tinted.sum()), int((~nis.pixels).sum()))


# ---- the planner against mask_ref ------------------------------------------------------------------------------------------------------
def _span_columns(spans, bands, ow):
    """[bands, outW] bool from [x0, band, xEnd] segments; no column covered twice"""
    cover = np.zeros((bands, ow), bool)
    for x0, band, x_end in spans:
        assert 0 <= x0 < x_end <= ow and band < bands and x_end - x0 <= 62, (x0, band, x_end)
        assert not cover[band, x0:x_end].any(), (x0, band, x_end)
        cover[band, x0:x_end] = True
    return cover


def test_every_variant_plans(plans):
    refused = sorted(k for k, p in plans.items() if p["status"] != 0)
    assert refused == [], refused


@pytest.mark.parametrize("cid", CASE_IDS)
def test_planner_lists_equal_mask_ref(plans, cid):
    c = MR.BY_ID[cid]
    iw, ih, ow, oh = c.shape
    compared = 0
    for name, fmt, one_eye, cfg in TP.VARIANTS:
        p = plans[(cid, name)]
        if p["status"] != 0:
            continue
        kind = "nvscaler" if cfg.get("use_nis") else "fsr"
        tw, th = (32, 24) if kind == "nvscaler" else (32, 32)
        refs = [MR.mask_ref(c.shape, c.radius, c.proj, bool(one_eye), eye, kind) for eye in (0, 1)]
        assert p["out"] == [ow, oh] and p["no_mesh_equal"] == 1 and p["hidden_area"] == 0, (cid, name)
        for eye in (0, 1):
            assert p["centre"][eye] == [int(v) for v in refs[eye].centre], (cid, name, eye, p["centre"])
        assert p["mask_mode"] == [r.mode for r in refs], (cid, name, p["mask_mode"])
        # the strict build tests the mask per group and has no lists; everything else has them exactly when some eye is mixed
        lists = cfg.get("precision") != 2 and any(r.mode == MR.MIXED for r in refs)
        assert p["tile_lists"] == int(lists), (cid, name, p["tile_lists"])
        compared += 1
        if not lists:
            assert all(p[k] == [[], []] for k in ("inside", "ring", "outside", "rcas", "spans")), (cid, name)
            continue
        assert p["tile"] == [tw, th] and p["tiles"] == refs[0].tile_grid(tw, th)[0] * refs[0].tile_grid(tw, th)[1], (cid, name, p["tile"], p["tiles"])
        assert p["skipped"] == [0, 0]
        for eye, r in enumerate(refs):
            inside, outside = r.tiles(tw, th)
            where = (cid, name, eye)
            for key, want in (("inside", inside), ("outside", outside), ("ring", r.ring(tw, th)), ("rcas", inside)):
                got = p[key][eye]
                assert len(set(got)) == len(got), where + (key, "an entry twice")
                assert set(got) == want, where + (key, sorted(set(got) - want), sorted(want - set(got)))
            if (tw, th) == (32, 32):
                assert np.array_equal(_span_columns(p["spans"][eye], r.tile_grid(32, 32)[1], ow), r.rcas_columns()), where
            else:
                assert p["spans"][eye] == [], where   # (NVScaler's 24-row tiles are not the span kernel's)
        assert p["lists_shared"] == int(refs[0].tiles(tw, th) == refs[1].tiles(tw, th)), (cid, name)   # (equal tile sets: ring and spans follow)
    assert compared == len(TP.VARIANTS), (cid, compared)
