"""The radius mask with its disc on the image's edge, on the GPU: every row of the case table of tests/mask_ref.py through every masked form,
each frame against the ORACLE at the effective centres -- never against a twin ctx, which runs the same mask_constants, classify_tiles,
ring_tiles, rcas_spans, tile_record and kernels and shares their errors.  (a) every case x every form on a fresh ctx with the centres in
cfg.proj_centre; (b) one ctx per form walking the table's centres with ovrfsr_set_gaze: re-aims in place, a rebuild at the all-outside step
and back -- the first independent check of tile_records_kernel's records at edge tiles; (c) the hidden-area meshes of tests/hidden_ref.py with
the disc on the corner (1, 1).  Every case asserts its class property and the promised number of inside pixels from mask_ref before anything
is compared.  Tolerances are those of tests/test_gpu_parity.py for the same form:
    strict: bit for bit; exact: the strict build's bytes; EASU-only RGBA8: identical to float_to_unorm8(oracle);
    RGBA8 pipelines: <= 1 LSB on <= 0.1 % of the bytes; half pipelines: <= 1e-3; NVScaler: max-abs <= 1e-3 and <= 1 LSB;
    pixels of outside groups: the oracle's bytes in every RGBA8 form; mask-sorted == plain two-pass.
Product-build distances go to reports/mask_edges.json (ignored by git; OVRFSR_REPORT_DIR names another directory; committed copy:
profiles/mask_edges.json): max LSB, the share of differing bytes over the image and over the inside pixels only, max abs.  The inside-only
share is recorded, not asserted: with one group inside, 0.1 % of the image is a looser bound than it looks."""
import functools
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import hidden_ref as R
from tests import mask_ref as MR
from tests import synth
from tests.test_gpu_hidden_area import _launch, _outputs, _source
from tests.test_gpu_parity import LSB_FRACTION, NIS_FLOAT_TOL, RCAS_LSB, lsb_stats, run_gpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARP = 0.9
HALF_TOL = 1e-3          # tests/test_gpu_parity.py, test_c4_c5_shapes_properties: the half pipeline's contract
STRICT, EXACT = 2, 3
# id -> source, call, configuration, what it is compared with
FORMS = {
    "mask-sorted": ("rgba8", "apply", {}, "pipeline"),
    "two-pass": ("rgba8", "apply", dict(fused=0), "pipeline"),
    "fused": ("rgba8", "apply", dict(fused=1), "pipeline"),
    "easu-only": ("rgba8", "apply", dict(stage_mask=1), "easu"),
    "half": ("rgba16f", "apply", {}, "half"),
    "nis": ("rgba8", "apply", dict(use_nis=1), "nis"),
    "strict": ("rgba8", "apply", dict(precision=STRICT), "exact-bytes"),
    "exact": ("rgba8", "apply", dict(precision=EXACT), "exact-bytes"),
    "batch": ("rgba8", "batch", {}, "pipeline"),
}
SHARED_FORMS = {
    "shared": ("rgba8", "shared", {}, "pipeline"),
    "shared-strict": ("rgba8", "shared", dict(precision=STRICT), "exact-bytes"),
    "shared-nis": ("rgba8", "shared", dict(use_nis=1), "nis"),
}
ALL_FORMS = dict(FORMS, **SHARED_FORMS)
CASE_FORMS = [pytest.param(c.id, f, id="%s-%s" % (c.id, f)) for c in MR.CASES for f in (FORMS if c.one_eye else SHARED_FORMS)]
RGBA8_PIPELINES = ["mask-sorted", "two-pass", "fused", "strict", "exact", "batch"]
_RECORDS = []


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    if not _RECORDS:
        return
    out_dir = os.environ.get("OVRFSR_REPORT_DIR") or os.path.join(ROOT, "reports")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "mask_edges.json"), "w") as f:
        json.dump({"note": "masked forms with the disc at the image edge, product and strict builds vs CPU oracle, the largest value over a call's images; "
                           "written by tests/test_gpu_mask_edges.py", "records": _RECORDS}, f, indent=1)


# ---- inputs and oracle results, computed once ------------------------------------------------------------------------------------------
def _seed(i):
    return synth.seed_for(31, i)


@functools.lru_cache(maxsize=None)
def _image(src, iw, ih, i):
    img8 = synth.structured_u8(iw, ih, _seed(i))
    return img8 if src == "rgba8" else (img8.astype(np.float32) / np.float32(255)).astype(np.float16)


@functools.lru_cache(maxsize=None)
def _want(what, shape, radius, proj, one_eye, eye, i):
    """the oracle's frame for image i: "pipeline" / "exact-bytes" uint8, "easu" uint8, "half" float32 (half values), "nis" float32"""
    iw, ih, ow, oh = shape
    centre, rad = MR.constants(shape, radius, proj, one_eye, eye)
    if what in ("pipeline", "exact-bytes"):
        return O.fsr_pipeline_u8(_image("rgba8", iw, ih, i), ow, oh, sharpness=SHARP, radius=radius, proj=proj, eye=eye, one_eye_per_texture=one_eye)
    if what == "easu":
        return O.float_to_unorm8(O.easu(O.unorm8_to_float(_image("rgba8", iw, ih, i)), ow, oh, O.easu_con(iw, ih, ow, oh), centre, rad))
    if what == "half":    # half intermediate texture, half destination (tests/test_gpu_parity.py, test_c4_c5_shapes_properties)
        e = O.easu(_image("rgba16f", iw, ih, i).astype(np.float32), ow, oh, O.easu_con(iw, ih, ow, oh), centre, rad)
        return O.rcas(e.astype(np.float16).astype(np.float32), O.rcas_con(SHARP), centre, rad).astype(np.float16).astype(np.float32)
    import openvr_fsr_amd as A
    cs, cu = A.nis_coefs()
    ok, cfg = A.nis_scaler_config(SHARP, iw, ih, ow, oh)
    assert ok
    return O.nis_upscale(O.unorm8_to_float(_image("rgba8", iw, ih, i)), ow, oh, O.nis_block(cfg, centre, rad, 0), cs, cu)


def _kind(form):
    return "nvscaler" if ALL_FORMS[form][2].get("use_nis") else "fsr"


def _images(call):
    return 4 if call == "batch" else 2


def _eye_of(call, i):
    return 0 if call == "shared" else i & 1


def _make(A, shape, radius, proj, cfg):
    return A.PostProcessor(fsr_enabled=1, out_width=shape[2], out_height=shape[3], sharpness=SHARP, radius=radius, proj_centre=proj, **cfg)


def _frames(torch, pp, form, shape, dtype=None):
    """one call of the form on pp into 0xA5-filled destinations -> numpy [n, oh, ow, 4] (uint8, float16 or, with dtype, float32)"""
    src, call, cfg, what = ALL_FORMS[form]
    iw, ih, ow, oh = shape
    n = _images(call)
    built = [_source(torch, src, iw, ih, _seed(i)) for i in range(n)]
    texs, (in_format, own, bpp) = [b[0] for b in built], built[0][1:]
    outs, raw = _outputs(torch, n, oh, ow, *((dtype, 16) if dtype is not None else (own, bpp)))
    _launch(torch, pp, call, texs, in_format, outs)
    got = outs.cpu().numpy()
    assert (raw.cpu().numpy() != 0xA5).any()
    return got


def _compare(form, got, want, inside, where):
    """one image under the form's tolerance.  `inside`: [oh, ow] bool, mask_ref's inside pixels.  -> the record's fields"""
    what = ALL_FORMS[form][3]
    outside = ~inside
    if got.dtype == np.uint8:
        want8 = want if want.dtype == np.uint8 else O.float_to_unorm8(want)
        d = np.abs(got.astype(np.int16) - want8.astype(np.int16))
        mx, frac = lsb_stats(got, want8)
        rec = dict(max_lsb=mx, differing=frac, differing_inside=float((d[inside] != 0).mean()) if inside.any() else 0.0, max_abs=None)
        print(where, rec)
        assert np.array_equal(got[outside], want8[outside]), where + ("a pixel of an outside group differs from the oracle's",)
        if what in ("exact-bytes", "easu"):
            assert np.array_equal(got, want8), where + (mx, frac)
        elif what == "nis":
            assert mx <= 1, where + (mx, frac)
        else:
            assert mx <= RCAS_LSB and frac <= LSB_FRACTION, where + (mx, frac)
    else:
        d = np.abs(got.astype(np.float32) - want)
        rec = dict(max_lsb=None, differing=float((d != 0).mean()), differing_inside=float((d[inside] != 0).mean()) if inside.any() else 0.0,
                   max_abs=float(d.max()))
        print(where, rec)
        assert d.max() <= (HALF_TOL if what == "half" else NIS_FLOAT_TOL), where + (float(d.max()),)
    return rec


def _merge(records):
    out = dict(records[0])
    for r in records[1:]:
        for k, v in r.items():
            out[k] = v if out[k] is None else out[k] if v is None else max(out[k], v)
    return out


def _check_call(form, frames, shape, radius, proj, one_eye, where, tag):
    """every image of one call against the oracle; appends the call's record"""
    call, what = ALL_FORMS[form][1], ALL_FORMS[form][3]
    recs = []
    for i in range(frames.shape[0]):
        eye = _eye_of(call, i)
        inside = MR.mask_ref(shape, radius, proj, one_eye, eye, _kind(form)).pixels
        recs.append(_compare(form, frames[i], _want(what, shape, radius, tuple(proj), one_eye, eye, i), inside, where + (i,)))
    _RECORDS.append(dict(case=tag, form=form + ("/float32" if frames.dtype == np.float32 else ""), out=list(shape[2:]), images=int(frames.shape[0]), **_merge(recs)))


def _promised(c, form):
    """class property first, then the inside-pixel count the table promises for the form's group size"""
    MR.class_property(c)
    for eye in c.eyes():
        r = c.ref(eye, _kind(form))
        assert int(r.pixels.sum()) == c.promised_pixels(eye, _kind(form)), (c.id, form, eye, int(r.pixels.sum()))


# ---- (a) every case x every form, fresh ctx -------------------------------------------------------------------------------------------
_GOT = {}


def _case_frames(torch, A, c, form):
    if (c.id, form) not in _GOT:
        pp = _make(A, c.shape, c.radius, c.proj, ALL_FORMS[form][2])
        try:
            _GOT[(c.id, form)] = _frames(torch, pp, form, c.shape)
        finally:
            pp.close()
    return _GOT[(c.id, form)]


@pytest.mark.parametrize("cid,form", CASE_FORMS)
def test_case_against_the_oracle(gpu, cid, form):
    torch = gpu
    import openvr_fsr_amd as A
    c = MR.BY_ID[cid]
    _promised(c, form)
    frames = _case_frames(torch, A, c, form)
    _check_call(form, frames, c.shape, c.radius, c.proj, c.one_eye, (cid, form), cid)
    if ALL_FORMS[form][3] == "nis":   # the max-abs half of NVScaler's bound: a float destination
        pp = _make(A, c.shape, c.radius, c.proj, ALL_FORMS[form][2])
        try:
            _check_call(form, _frames(torch, pp, form, c.shape, torch.float32), c.shape, c.radius, c.proj, c.one_eye, (cid, form, "float32"), cid)
        finally:
            pp.close()


@pytest.mark.parametrize("cid", [c.id for c in MR.CASES if c.one_eye])
def test_forms_of_a_case_agree(gpu, cid):
    """mask-sorted == plain two-pass, byte for byte; the pixels of outside groups identical across the RGBA8 pipeline forms"""
    torch = gpu
    import openvr_fsr_amd as A
    c = MR.BY_ID[cid]
    MR.class_property(c)
    got = {f: _case_frames(torch, A, c, f) for f in RGBA8_PIPELINES}
    assert np.array_equal(got["mask-sorted"], got["two-pass"]), cid
    assert np.array_equal(got["batch"][:2], got["mask-sorted"]), cid           # (a batch's images: the single applies')
    assert np.array_equal(got["exact"], got["strict"]), cid
    for eye in (0, 1):
        outside = ~c.ref(eye).pixels
        for f in RGBA8_PIPELINES[1:]:
            assert np.array_equal(got[f][eye][outside], got["mask-sorted"][eye][outside]), (cid, f, eye)


@pytest.mark.parametrize("form", ["mask-sorted", "fused", "half", "nis", "easu-only"])
@pytest.mark.parametrize("cid", [c.id for c in MR.CASES if c.klass == "all-outside"])
def test_all_outside_by_another_route(gpu, cid, form):
    """the disc off the image to the right == a centred disc of radius 0 that meets no group centre, on the same ctx: byte for byte"""
    torch = gpu
    import openvr_fsr_amd as A
    c = MR.BY_ID[cid]
    _promised(c, form)
    other = dict(radius=0.0, proj=(0.5, 0.5, 0.5, 0.5))
    modes = [MR.mask_ref(c.shape, c.radius, c.proj, True, e, _kind(form)).mode for e in (0, 1)]
    assert [MR.mask_ref(c.shape, other["radius"], other["proj"], True, e, _kind(form)).mode for e in (0, 1)] == [MR.ALL_OUTSIDE] * 2, cid
    pp = _make(A, c.shape, c.radius, c.proj, ALL_FORMS[form][2])
    try:
        first = _frames(torch, pp, form, c.shape)
        pp.set_config(A.Config.default(fsr_enabled=1, out_width=c.shape[2], out_height=c.shape[3], sharpness=SHARP, radius=other["radius"],
                                       proj_centre=other["proj"], **ALL_FORMS[form][2]))
        second = _frames(torch, pp, form, c.shape)
    finally:
        pp.close()
    _check_call(form, second, c.shape, other["radius"], other["proj"], True, (cid, form, "radius 0"), cid + "/radius-0-route")
    if modes == [MR.ALL_OUTSIDE] * 2:    # (at 200 x 147 two of NVScaler's groups are inside: see the table)
        assert np.array_equal(first.view(np.uint8), second.view(np.uint8)), (cid, form)
    else:
        assert form == "nis" and cid == "all-outside-S2", (cid, form, modes)


def test_a_negative_gaze_gives_the_bytes_of_zero(gpu):
    c = MR.BY_ID["negative-S3"]
    MR.class_property(c)
    iw, ih, ow, oh = c.shape
    img8 = _image("rgba8", iw, ih, 0)
    for cfg in ({}, dict(use_nis=1), dict(precision=STRICT)):
        a = run_gpu(img8, ow, oh, np.uint8, eye=0, sharpness=SHARP, radius=c.radius, proj_centre=c.proj, **cfg)
        b = run_gpu(img8, ow, oh, np.uint8, eye=0, sharpness=SHARP, radius=c.radius, proj_centre=(0.0, 0.0, 0.0, 0.0), **cfg)
        assert np.array_equal(a, b), cfg


# ---- (b) the gaze path against the oracle ----------------------------------------------------------------------------------------------
# (left, right) gazes: the table's centres at S3 and radius 0.5, every step sets both eyes.  The all-outside step is (0.5, 1.4) on both eyes,
# below the image: the table's (1.2, 0.5) puts a shared texture's left centre into its right half, where the disc is on the image
WALK = [((0.0, 0.0), (1.0, 1.0)), ((1.0, 1.0), (1.0, 0.0)), ((-1.0, -1.0), (0.0, 0.0)), ((1.2, 0.5), (0.8, 0.7)), ((0.5, 1.4), (0.5, 1.4)),
        ((0.8, 0.7), (1.25, 1.25)), ((0.999, 0.999), (0.03, 0.03)), ((0.5, 0.5), (2.0, 0.5)), ((-0.5, 0.5), (0.5, 1.25))]
WALK_RADIUS, WALK_SHAPE = 0.5, MR.S3
WALK_FORMS = ["mask-sorted", "half", "nis", "shared"]


def _walk_modes(form, step):
    one_eye = ALL_FORMS[form][1] != "shared"
    return [MR.mask_ref(WALK_SHAPE, WALK_RADIUS, step[0] + step[1], one_eye, eye, _kind(form)).mode for eye in ((0, 1) if one_eye else (0,))]


def test_the_walk_visits_what_it_should():
    """from mask_ref: at least three re-aims between mixed masks, a step with one eye all-outside, a step with every eye all-outside (the
    rebuild) and a mixed step after it (the way back), for every form of the walk"""
    for form in WALK_FORMS:
        modes = [_walk_modes(form, s) for s in WALK]
        mixed = [MR.MIXED in m for m in modes]
        assert not any(MR.ALL_INSIDE in m for m in modes), form
        gone = [i for i, m in enumerate(mixed) if not m]
        assert gone and 0 < gone[0] < len(WALK) - 1 and mixed[gone[-1] + 1], (form, modes)
        assert sum(1 for a, b in zip(mixed, mixed[1:]) if a and b) >= 3, (form, modes)
        if form != "shared":
            assert any(sorted(m) == [MR.ALL_OUTSIDE, MR.MIXED] for m in modes), (form, modes)


@pytest.mark.parametrize("form", WALK_FORMS)
def test_every_gaze_of_the_walk_against_the_oracle(gpu, form):
    torch = gpu
    import openvr_fsr_amd as A
    one_eye = ALL_FORMS[form][1] != "shared"
    pp = _make(A, WALK_SHAPE, WALK_RADIUS, (0.5, 0.5, 0.5, 0.5), ALL_FORMS[form][2])
    try:
        stats, lists = (0, 0), None
        for i, step in enumerate(WALK):
            for eye in (0, 1):
                pp.set_gaze(eye, *step[eye])
            frames = _frames(torch, pp, form, WALK_SHAPE)
            _check_call(form, frames, WALK_SHAPE, WALK_RADIUS, step[0] + step[1], one_eye, ("walk", form, i), "walk-%d" % i)
            # the planner's rule (pipeline_plan.h, reaim_pipeline): tile lists exist where some eye is mixed; a step that keeps that is a
            # re-aim in place, one that changes it a rebuild -- predicted from mask_ref's modes, not from the planner
            now = pp.gaze_stats()
            has = MR.MIXED in _walk_modes(form, step)
            want = (0, 0) if lists is None else (1, 0) if has == lists else (0, 1)
            assert (now[0] - stats[0], now[1] - stats[1]) == want, (form, i, now, stats, want)
            stats, lists = now, has
        assert stats[0] >= 3 and stats[1] >= 2, stats
    finally:
        pp.close()


# ---- (c) mesh plus edge ------------------------------------------------------------------------------------------------------------------
MESH_RADIUS, MESH_PROJ = 0.9, (1.0, 1.0, 1.0, 1.0)    # (radius 0.5 about (1, 1) lies wholly under the meshes' bottom-right rectangle and band)


@pytest.mark.parametrize("form", ["mask-sorted", "two-pass"])
def test_mesh_with_the_disc_on_a_corner(gpu, form):
    torch = gpu
    import openvr_fsr_amd as A
    shape = MR.S3
    iw, ih, ow, oh = shape
    hidden = [R.hidden_tiles(R.MESH[eye], ow, oh, 32, 32).astype(bool) for eye in (0, 1)]
    for eye in (0, 1):     # the class property: the disc is on the corner, and the mesh hides some of its tiles and shows others
        r = MR.mask_ref(shape, MESH_RADIUS, MESH_PROJ, True, eye)
        assert [int(v) for v in r.centre[:2]] == [ow, oh] and r.mode == MR.MIXED
        inside, outside = r.tiles(32, 32)
        flat = hidden[eye].reshape(-1)
        assert any(flat[t] for t in inside) and any(not flat[t] for t in inside) and any(flat[t] for t in outside) and any(not flat[t] for t in outside), eye
    pp = _make(A, shape, MESH_RADIUS, MESH_PROJ, ALL_FORMS[form][2])
    try:
        for eye in (0, 1):
            pp.set_hidden_area(eye, R.MESH[eye])
        frames = _frames(torch, pp, form, shape)
        skipped = [pp.hidden_area_stats(eye) for eye in (0, 1)]
    finally:
        pp.close()
    recs = []
    for eye in (0, 1):
        assert skipped[eye] == (hidden[eye].size, int(hidden[eye].sum())), (eye, skipped[eye])
        skip = np.repeat(np.repeat(hidden[eye], 32, axis=0), 32, axis=1)[:oh, :ow]
        want = _want("pipeline", shape, MESH_RADIUS, MESH_PROJ, True, eye, eye)
        got = frames[eye]
        assert (got[skip] == 0xA5).all(), (form, eye, "a skipped tile was written")
        inside = MR.mask_ref(shape, MESH_RADIUS, MESH_PROJ, True, eye).pixels
        d = np.abs(got.astype(np.int16) - want.astype(np.int16))[~skip]
        rec = dict(max_lsb=int(d.max()), differing=float((d != 0).mean()), differing_inside=float((d[inside[~skip]] != 0).mean()), max_abs=None)
        print(form, eye, rec)
        recs.append(rec)
        assert np.array_equal(got[~skip & ~inside], want[~skip & ~inside]), (form, eye)
        assert rec["max_lsb"] <= RCAS_LSB and rec["differing"] <= LSB_FRACTION, (form, eye, rec)
    _RECORDS.append(dict(case="mesh-corner-11-S3", form=form, out=[ow, oh], images=2, **_merge(recs)))
