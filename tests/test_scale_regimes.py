"""The per-axis scale regimes of the EASU kernels without a GPU: the table of tests/scale_cases.py -- steep, anisotropic, one axis at 1:1,
one axis minified, footprints of 47 to 100 cells across and of 37 to 52 rows, the accept / refuse line on both sides -- (a) each case against
its class property, (b) the ORACLE against the reference's compiled FsrEasuF / FsrRcasF / NVScaler at every shape the GPU test submits
(live where oracle/_ref is built, else through the SHA-256 digests of tests/golden/ref_digests.json): the judge is valid at these ratios,
(c) every case through the planner (tests/debug/plan_probe.cpp, stand-alone under ASan + UBSan, a child process) for the RGBA8 / RGBA16F /
RGBA32F product builds, the strict build, `fused = 1`, the masked auto forms, FP32_EXACT and NVScaler: cells, kernel pitch, form, overlap,
status and text of every refusal equal to the table and to the restatement of scale_cases.

Two asymmetries of the accept / refuse line are pinned AS THEY ARE.  easu_lds_bytes sizes a product plan by the fast kernel's pitch wherever
the footprint's width has one, so a narrow, tall footprint (refuse-tall-*) is refused by the product build although the strict build,
which always takes the generic layout, plans it; and a wide isotropic minification (iso-min-*) fits the generic layout's 8-byte colour
plane of a byte or half source, so the product build plans it for those, and refuses it for RGBA32F sources as the strict build does.
Letting the planner fall back to the generic kernel would remove the first; that is a product change, and these tests will then say so."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import mask_ref as MR
from tests import refgold
from tests import scale_cases as SC
from tests import synth
from tests import test_pipeline_plan as TP
from tests.test_pipeline_plan import probe  # noqa: F401  (the fixture: the probe under the host sanitizers)

CASE_IDS = [c.id for c in SC.CASES]
KINDS = {"structured": synth.structured_u8, "random": synth.random_u8, "extremes": synth.extremes_u8}
SHARP = 0.9


# ---- (a) the table is what it says it is -------------------------------------------------------------------------------------------------
def test_every_class_of_the_table_is_present():
    assert {c.klass for c in SC.CASES} == SC.CLASSES
    assert len(set(CASE_IDS)) == len(CASE_IDS)
    assert len(SC.ACCEPTED) == 17 and len(SC.NIS_SHAPES) == 6
    assert set(SC.HALF_IDS) | set(SC.PITCHED_IDS) <= {c.id for c in SC.ACCEPTED}


@pytest.mark.parametrize("cid", CASE_IDS)
def test_class_property(cid):
    SC.class_property(SC.BY_ID[cid])


@pytest.mark.parametrize("cid", [c.id for c in SC.GPU_CASES])
def test_masked_shape_shows_every_tile_class(cid):
    """radius 0.5 about unequal centres at the doubled shape: each eye has inside tiles, a ring and outside tiles beyond the ring"""
    c = SC.BY_ID[cid]
    for eye in (0, 1):
        r = MR.mask_ref(c.masked_shape, SC.MASK_RADIUS, SC.MASK_PROJ, True, eye)
        inside, outside = r.tiles(32, 32)
        assert r.mode == MR.MIXED and inside and r.ring(32, 32) and outside - r.ring(32, 32), (cid, eye, len(inside), len(outside))
    refs = [MR.mask_ref(c.masked_shape, SC.MASK_RADIUS, SC.MASK_PROJ, True, eye) for eye in (0, 1)]
    assert not np.array_equal(refs[0].centre, refs[1].centre), cid


# ---- (b) the oracle against the compiled reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in SC.GPU_CASES])
def test_oracle_equals_the_reference(cid):
    c = SC.BY_ID[cid]
    for masked, shape in ((0, c.shape), (1, c.masked_shape)):
        iw, ih, ow, oh = shape
        con = O.easu_con(iw, ih, ow, oh)
        centre, rad = O.mask_constants(ow, oh, SC.MASK_RADIUS, SC.MASK_PROJ, True, 1) if masked else O.mask_constants(ow, oh)
        rcon = O.rcas_con(SHARP)
        for kind, gen in KINDS.items():
            img = O.unorm8_to_float(gen(iw, ih, 7))
            key = "scale_regimes/%s/%d/%s/" % (cid, masked, kind)
            a = O.easu(img, ow, oh, con, centre, rad)
            assert refgold.same_as_reference(key + "easu", a, lambda: O.ref_easu(img, ow, oh, con, centre, rad)), key
            q = O.unorm8_to_float(O.float_to_unorm8(a))       # the composition: RCAS on the UNORM8 intermediate
            assert refgold.same_as_reference(key + "rcas", O.rcas(q, rcon, centre, rad), lambda: O.ref_rcas(q, rcon, centre, rad)), key


@pytest.mark.parametrize("shape", SC.NIS_SHAPES, ids=["%dx%d-%dx%d" % s for s in SC.NIS_SHAPES])
def test_nis_oracle_equals_the_reference(shape):
    cs, cu = refgold.ref_nis_coefs()
    for masked, (iw, ih, ow, oh) in ((0, shape), (1, tuple(2 * v for v in shape))):
        ok, cfg = refgold.ref_nis_scaler_config(SHARP, iw, ih, ow, oh)
        assert ok, (iw, ih, ow, oh)       # NVScalerUpdateConfig accepts all six
        centre, rad = O.mask_constants(ow, oh, SC.MASK_RADIUS, SC.MASK_PROJ, True, 1) if masked else O.mask_constants(ow, oh)
        blk = O.nis_block(cfg, centre, rad, 0)
        for kind, gen in KINDS.items():
            img = O.unorm8_to_float(gen(iw, ih, 7))
            key = "scale_regimes/nis/%dx%d-%dx%d/%s/" % (iw, ih, ow, oh, kind)
            assert refgold.same_as_reference(key + "nis_upscale", O.nis_upscale(img, ow, oh, blk, cs, cu),
                                             lambda: O.ref_nis_upscale(img, ow, oh, blk, cs, cu)), key


# ---- (c) the planner against the table ----------------------------------------------------------------------------------------------------
MASK = dict(radius=SC.MASK_RADIUS, proj_centre=SC.MASK_PROJ)
# name -> (source format, source name, masked, configuration)
BUILDS = {
    "rgba8": (TP.RGBA8, SC.RGBA8, False, dict(radius=2.0)),
    "rgba16f": (TP.RGBA16F, SC.RGBA16F, False, dict(radius=2.0)),
    "rgba32f": (TP.RGBA32F, SC.RGBA32F, False, dict(radius=2.0)),
    "strict": (TP.RGBA8, SC.RGBA8, False, dict(radius=2.0, precision=2)),
    "fused": (TP.RGBA8, SC.RGBA8, False, dict(radius=2.0, fused=1)),
    "exact": (TP.RGBA8, SC.RGBA8, False, dict(radius=2.0, precision=3)),
    "nis": (TP.RGBA8, SC.RGBA8, False, dict(radius=2.0, use_nis=1)),
    "masked": (TP.RGBA8, SC.RGBA8, True, MASK),
    "masked-half": (TP.RGBA16F, SC.RGBA16F, True, MASK),
    "masked-fused": (TP.RGBA8, SC.RGBA8, True, dict(MASK, fused=1)),
    "masked-exact": (TP.RGBA8, SC.RGBA8, True, dict(MASK, precision=3)),
    "masked-strict": (TP.RGBA8, SC.RGBA8, True, dict(MASK, precision=2)),
}


@pytest.fixture(scope="module")
def plans(probe):  # noqa: F811
    keys, lines = [], []
    for c in SC.CASES:
        for name, (fmt, _, masked, cfg) in BUILDS.items():
            iw, ih, ow, oh = c.masked_shape if masked else c.shape
            keys.append((c.id, name))
            lines.append(TP._line("%s/%s" % (c.id, name), fmt, iw, ih, 1, -1, fsr_enabled=1, out_width=ow, out_height=oh, sharpness=SHARP, **cfg))
    for shape in SC.NIS_SHAPES:
        for masked in (0, 1):
            iw, ih, ow, oh = tuple(2 * v for v in shape) if masked else shape
            keys.append((shape, masked))
            lines.append(TP._line("nis-%dx%d-%dx%d/%d" % (iw, ih, ow, oh, masked), TP.RGBA8, iw, ih, 1, -1, fsr_enabled=1, out_width=ow, out_height=oh,
                                  sharpness=SHARP, use_nis=1, **(MASK if masked else dict(radius=2.0))))
    return dict(zip(keys, TP._plan(probe, lines)))


def _outside_span(out_n, in_n, tile):
    """the bilinear fallback's taps per tile (csrc/pipeline_plan.cpp tap_tables, the oracle's bilinear_uv): last tap + 2 - first tap, >= 2"""
    o = np.arange(out_n)
    u = (o.astype(np.float32) / np.float32(out_n)).astype(np.float32)
    t = ((u * np.float32(in_n)).astype(np.float32) + np.float32(-0.5)).astype(np.float32)
    s = np.floor(((t * np.float32(256)).astype(np.float32) + np.float32(0.5)).astype(np.float32))
    i0 = np.floor((s * np.float32(1 / 256)).astype(np.float32)).astype(np.int64)
    o0 = np.arange(0, out_n, tile)
    return int(max(2, (i0[np.minimum(o0 + tile - 1, out_n - 1)] + 2 - i0[o0]).max()))


@pytest.mark.parametrize("cid", CASE_IDS)
def test_planner_agrees_with_the_table(plans, cid):
    c = SC.BY_ID[cid]
    for name, (_, src, masked, cfg) in BUILDS.items():
        p = plans[(cid, name)]
        shape = c.masked_shape if masked else c.shape
        iw, ih, ow, oh = shape
        where = (cid, name, p)
        strict, fused, nis = cfg.get("precision") == 2, cfg.get("fused") == 1, bool(cfg.get("use_nis"))
        # status and text
        if nis:
            want = (0, "") if SC.nis_accepted(shape) else SC.REFUSED_NIS
        elif not c.plans(src, strict):
            want = SC.REFUSED_LDS
        elif fused and not c.fused:
            want = SC.REFUSED_FUSED
        else:
            want = (0, "")
        assert (p["status"], p["text"]) == want, where
        if p["status"]:
            continue
        assert p["invariants"] == "ok" and p["out"] == [ow, oh], where
        assert p["outside_cols"] == _outside_span(ow, iw, 32) and p["outside_rows"] == [_outside_span(oh, ih, 32), _outside_span(oh, ih, 24)], where
        if nis:
            assert p["form"] == "upscale only", where
            continue
        # cells and the kernel they pick
        cw, ch, fw, fh = SC.footprint(shape)
        assert p["cells"] == [cw, ch] and p["fused_cells"] == [fw, fh], where + ((cw, ch, fw, fh),)
        if not masked:
            assert tuple(p["cells"]) == c.cells, where
        assert SC.kernel_pitch(p["cells"][0]) == c.pitch, where
        # the form
        lists = masked and not strict
        assert p["tile_lists"] == int(lists), where
        if fused:
            form = "fused with masked outside tiles" if lists else "fused"
        elif masked and not strict and src == SC.RGBA8:
            form = "mask-sorted"
        elif name == "masked-half":     # auto: the fused kernel where its ring fits a fixed pitch, else two kernels over the lists
            form = "fused with masked outside tiles" if c.fused else "two-pass"
        else:
            form = "two-pass"
        assert p["form"] == form, where
        # the outside tiles: the staged kernel in order where no axis minifies and the source is RGBA8, else per-pixel on the auxiliary stream
        assert p["overlap"] == int(lists and not (src == SC.RGBA8 and c.staged)), where
        if lists:
            for eye in (0, 1):
                r = MR.mask_ref(shape, SC.MASK_RADIUS, SC.MASK_PROJ, True, eye)
                inside, outside = r.tiles(32, 32)
                assert (p["inside"][eye], p["ring"][eye], p["outside"][eye]) == (len(inside), len(r.ring(32, 32)), len(outside)), where
            assert p["lists_shared"] == 0, where


def test_nis_shapes_plan(plans):
    for shape in SC.NIS_SHAPES:
        for masked in (0, 1):
            p = plans[(shape, masked)]
            assert p["status"] == 0 and p["form"] == "upscale only" and p["invariants"] == "ok" and p["tile_lists"] == masked, (shape, masked, p)
            if masked:
                for eye in (0, 1):
                    r = MR.mask_ref(tuple(2 * v for v in shape), SC.MASK_RADIUS, SC.MASK_PROJ, True, eye, "nvscaler")
                    inside, outside = r.tiles(32, 24)
                    assert inside and outside and (p["inside"][eye], p["outside"][eye]) == (len(inside), len(outside)), (shape, eye, p)


def test_the_two_asymmetries(plans):
    """product refused where strict plans (refuse-tall-*), and the reverse (iso-min-*): see the module docstring"""
    for cid in ("refuse-tall-28", "refuse-tall-40"):
        assert plans[(cid, "rgba8")]["status"] == 2 and plans[(cid, "strict")]["status"] == 0, cid
        assert plans[(cid, "strict")]["cells"] == list(SC.BY_ID[cid].cells), cid
    for cid in ("iso-min-46", "iso-min-47"):
        assert [plans[(cid, n)]["status"] for n in ("rgba8", "rgba16f", "rgba32f", "strict", "exact")] == [0, 0, 2, 2, 0], cid
    # the fused kernel under y-minification: planned, a form the isotropic fuzz shapes never reach
    for cid in ("tall-32", "tall-32-deep", "tall-28-limit"):
        assert plans[(cid, "fused")]["status"] == 0 and plans[(cid, "masked-fused")]["form"] == "fused with masked outside tiles", cid
