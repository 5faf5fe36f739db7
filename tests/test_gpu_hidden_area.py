"""The hidden-area mesh on the GPU (include/openvr_fsr_amd.h, "hidden-area mesh").  Every case applies twice on one ctx, into caller-owned
destinations pre-filled with 0xA5 bytes: with the meshes of tests/hidden_ref.py (SYNTHETIC: no headset mesh exists here) and again with
the meshes cleared.  Asserted: outside the skipped tiles the two results are equal byte for byte; inside them every byte is still 0xA5;
the tiles_skipped that ovrfsr_hidden_area_stats reports is the CPU classification's count (tests/hidden_ref.py, the numpy restatement of
the rule) in the forms that skip, 0 in those that do not.  From the planner probe (tests/debug/hidden_probe.cpp) each case first asserts
that its mesh gives each eye a hidden tile edge-adjacent to a processed tile, a partly covered tile and a visible tile -- and, where there
is a mask, a hidden tile outside the radius and a visible outside tile --, so that none of them can silently drop out."""
import shutil

import numpy as np
import pytest

from openvr_fsr_amd import _capi as K
from tests import hidden_ref as R
from tests import msaa, packedf, synth
from tests import test_pipeline_plan as TP

pytestmark = pytest.mark.gpu

S1, S2, S3 = (80, 64, 160, 128), (150, 110, 200, 147), (240, 200, 320, 267)
M, U = dict(radius=0.5, proj_centre=(0.2, 0.3, 0.8, 0.7)), dict(radius=2.0)
# id, source, call, configuration, mask (None: both on S1, the matrix mask on the ragged and the large shape)
FORMS = [
    ("two-pass", "rgba8", "apply", {}, U),
    ("mask-sorted", "rgba8", "apply", {}, M),
    ("easu-only", "rgba8", "apply", dict(stage_mask=1), None),
    ("fused", "rgba8", "apply", dict(fused=1), None),
    ("half-fused-outside", "rgba16f", "apply", {}, M),
    ("nis-masked", "rgba8", "apply", dict(use_nis=1), M),
    ("nis-unmasked", "rgba8", "apply", dict(use_nis=1), U),
    ("exact", "rgba8", "apply", dict(precision=3), M),
    ("bgra8", "bgra8", "apply", {}, None),
    ("ms4", "ms4", "apply", {}, U),
    ("r11g11b10f", "r11", "apply", {}, None),
    ("batch", "rgba8", "batch", {}, None),
    ("shared", "rgba8", "shared", {}, None),
    ("pair", "rgba8", "pair", dict(pair_submit=1), None),
]
CASES = []
for _name, _src, _call, _cfg, _mask in FORMS:
    for _shape, _masks in ((S1, (M, U)), (S2, (M,)), (S3, (M,))):
        for _m in (_masks if _mask is None else (_mask,)):
            CASES.append(pytest.param(_src, _call, dict(_cfg, **_m), _shape,
                                      id="%s-%dx%d-%s" % (_name, _shape[2], _shape[3], "masked" if _m is M else "unmasked")))

PLAN_FORMAT = {"rgba8": TP.RGBA8, "rgba16f": TP.RGBA16F, "bgra8": TP.BGRA8, "ms4": TP.MS4_RGBA8, "r11": TP.R11G11B10F}


@pytest.fixture(scope="module")
def probe():
    run = R.build_probe()
    yield run
    shutil.rmtree(run.tmp, ignore_errors=True)


def _source(torch, src, iw, ih, seed):
    """-> (device tensor, in_format, output torch dtype, output bytes per pixel)"""
    if src == "rgba8":
        return torch.from_numpy(synth.structured_u8(iw, ih, seed)).cuda(), None, torch.uint8, 4
    if src == "bgra8":
        return torch.from_numpy(synth.structured_u8(iw, ih, seed)).cuda(), K.FORMAT_BGRA8, torch.uint8, 4
    if src == "rgba16f":
        return torch.from_numpy((synth.structured_u8(iw, ih, seed).astype(np.float32) / np.float32(255)).astype(np.float16)).cuda(), None, torch.float16, 8
    if src == "ms4":
        return torch.from_numpy(msaa.make_ms(iw, ih, 4, "rgba8", "structured", seed)).cuda(), None, torch.uint8, 4
    if src == "r11":
        return torch.from_numpy(packedf.make(iw, ih, "structured", seed).view(np.int32)).cuda(), K.FORMAT_R11G11B10F, torch.float16, 8
    raise ValueError(src)


def _outputs(torch, n, oh, ow, dtype, bpp):
    """n destinations of 0xA5 bytes: (the tensors the library writes, the same memory as [n, oh, ow * bpp] bytes)"""
    raw = torch.full((n, oh, ow * bpp), 0xA5, dtype=torch.uint8, device="cuda")
    return (raw if dtype == torch.uint8 else raw.view(dtype)).reshape(n, oh, ow, 4), raw


def _launch(torch, pp, call, texs, in_format, outs):
    if call == "apply":
        for eye in (0, 1):
            pp.apply(eye, texs[eye], out=outs[eye], in_format=in_format)
    elif call == "pair":
        pp.apply(0, texs[0], out=outs[0], in_format=in_format)
        assert pp.pair_pending()
        pp.apply(1, texs[1], out=outs[1], in_format=in_format)
        assert not pp.pair_pending()
    elif call == "batch":   # four alternating eyes, a different mesh per eye
        pp.apply_batch(torch.stack(texs), outs, first_eye=0, alternate_eyes=True, in_format=in_format)
    else:
        pp.apply_batch(torch.stack(texs), outs, shared=True, in_format=in_format)
    torch.cuda.synchronize()


def _pixel_mask(tiles, tw, th, oh, ow, bpp):
    return np.repeat(np.kron(tiles, np.ones((th, tw), np.uint8))[:oh, :ow].astype(bool), bpp, axis=1)


def _assert_mesh_covers_the_cases(probe, src, call, cfg, shape, masked):
    iw, ih, ow, oh = shape
    line = TP._line("case", PLAN_FORMAT[src], iw, ih, call != "shared", -1, fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, **cfg)
    plain, p = probe([R.with_mesh(line), R.with_mesh(line, R.MESH[0], R.MESH[1])])
    assert p["status"] == 0 and p["hidden_area"] == 1 and p["form"] == plain["form"]
    tw, th = p["tile"]
    tx = (ow + tw - 1) // tw
    ty = p["tiles"] // tx
    for eye in (0, 1):
        hid = set(np.flatnonzero(np.asarray(p["hidden"][eye])).tolist())
        processed = set(p["inside"][eye]) | set(p["outside"][eye])
        rcas = set(p["rcas"][eye]) if p["form"] in ("two-pass", "mask-sorted") else set(p["inside"][eye])

        def touches(t, tiles):
            x, y = t % tx, t // tx
            return any(0 <= nx < tx and 0 <= ny < ty and ny * tx + nx in tiles for nx, ny in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)))
        assert any(touches(t, rcas) for t in hid), "no hidden tile next to a tile RCAS (or the form's main kernel) processes"
        if p["form"] in ("two-pass", "mask-sorted"):
            assert set(p["ring"][eye]) & hid, "no hidden tile in the ring"
        mesh_eye = R.hidden_pixels(R.MESH[eye], ow, oh) if call != "shared" else \
            R.hidden_pixels(R.MESH[0], ow, oh, 0, ow // 2) | R.hidden_pixels(R.MESH[1], ow, oh, ow // 2, ow)
        part = (R.tiles_of(mesh_eye, tw, th) == 0) & (R.tiles_of(~mesh_eye, tw, th) == 0)
        assert part.any(), "no partly covered tile"
        assert processed - hid, "no visible tile"
        if masked:
            assert set(plain["outside"][eye]) & hid, "no hidden tile outside the radius"
            assert p["outside"][eye], "no visible outside tile"
    return p


@pytest.mark.parametrize("src,call,cfg,shape", CASES)
def test_skipped_tiles_are_not_written_and_the_rest_is_unchanged(gpu, probe, src, call, cfg, shape):
    torch = gpu
    import openvr_fsr_amd as A
    iw, ih, ow, oh = shape
    plan = _assert_mesh_covers_the_cases(probe, src, call, cfg, shape, cfg["radius"] < 2.0)
    tw, th = plan["tile"]
    n = {"apply": 2, "pair": 2, "batch": 4, "shared": 2}[call]
    built = [_source(torch, src, iw, ih, synth.seed_for(3, i)) for i in range(n)]
    texs, (in_format, dtype, bpp) = [b[0] for b in built], built[0][1:]
    pp = A.PostProcessor(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, **cfg)
    try:
        for eye in (0, 1):
            pp.set_hidden_area(eye, R.MESH[eye])
        outs, raw = _outputs(torch, n, oh, ow, dtype, bpp)
        _launch(torch, pp, call, texs, in_format, outs)
        stats = [pp.hidden_area_stats(eye) for eye in (0, 1)]
        for eye in (0, 1):
            pp.set_hidden_area(eye, None)          # clearing the mesh restores the full result
        full, full_raw = _outputs(torch, n, oh, ow, dtype, bpp)
        _launch(torch, pp, call, texs, in_format, full)
        assert [pp.hidden_area_stats(eye)[1] for eye in (0, 1)] == [0, 0]
    finally:
        pp.close()
    got, want = raw.cpu().numpy(), full_raw.cpu().numpy()
    if call == "shared":
        tiles = [R.hidden_tiles_shared(R.MESH[0], R.MESH[1], ow, oh, tw, th)] * 2
    else:
        tiles = [R.hidden_tiles(R.MESH[eye], ow, oh, tw, th) for eye in (0, 1)]
    for eye in (0, 1):
        print("eye %d: %d of %d tiles skipped (CPU classification: %d)" % (eye, stats[eye][1], stats[eye][0], int(tiles[eye].sum())))
        assert stats[eye] == (tiles[eye].size, int(tiles[eye].sum())) and 0 < stats[eye][1] < stats[eye][0]
    for i in range(n):
        skip = _pixel_mask(tiles[0 if call == "shared" else i & 1], tw, th, oh, ow, bpp)
        assert (want[i] != 0xA5).any() and np.array_equal(got[i][~skip], want[i][~skip]), "image %d differs outside the skipped tiles" % i
        assert (got[i][skip] == 0xA5).all(), "image %d: a skipped tile was written" % i


NON_SKIPPING = [
    pytest.param("rgba8", dict(precision=2, **M), S1, id="strict-masked"),
    pytest.param("rgba8", dict(precision=2, **U), S2, id="strict-unmasked"),
    pytest.param("rgba8", dict(stage_mask=2, **M), (160, 128, 160, 128), id="rcas-only"),
    pytest.param("rgba8", dict(use_nis=1, render_scale=1.0, **M), (160, 128, 160, 128), id="nvsharpen"),
]


@pytest.mark.parametrize("src,cfg,shape", NON_SKIPPING)
def test_forms_that_ignore_the_mesh(gpu, src, cfg, shape):
    torch = gpu
    import openvr_fsr_amd as A
    iw, ih, ow, oh = shape
    tex, in_format, dtype, bpp = _source(torch, src, iw, ih, synth.seed_for(5, 0))
    size = {} if "render_scale" in cfg else dict(out_width=ow, out_height=oh)
    pp = A.PostProcessor(fsr_enabled=1, sharpness=0.9, **size, **cfg)
    try:
        results = []
        for mesh in (R.MESH[0], None):
            pp.set_hidden_area(0, mesh)
            outs, raw = _outputs(torch, 1, oh, ow, dtype, bpp)
            pp.apply(0, tex, out=outs[0], in_format=in_format)
            torch.cuda.synchronize()
            assert pp.hidden_area_stats(0)[1] == 0
            results.append(raw.cpu().numpy())
    finally:
        pp.close()
    assert (results[0] != 0xA5).any() and np.array_equal(results[0], results[1])


def test_ctx_owned_output_has_zeros_in_skipped_tiles(gpu):
    torch = gpu
    import openvr_fsr_amd as A
    iw, ih, ow, oh = S2
    tex = _source(torch, "rgba8", iw, ih, synth.seed_for(6, 0))[0]
    pp = A.PostProcessor(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, **M)
    try:
        pp.set_hidden_area(0, R.MESH[0])
        got = pp.apply(0, tex).cpu().numpy()     # (the ctx-owned image: allocated by this call, under the mesh)
        again = pp.apply(0, tex).cpu().numpy()   # (not cleared again, not written there either)
        pp.set_hidden_area(0, None)
        want = pp.apply(0, tex).cpu().numpy()
    finally:
        pp.close()
    skip = _pixel_mask(R.hidden_tiles(R.MESH[0], ow, oh), 32, 32, oh, ow, 1)
    assert skip.any() and (got[skip] == 0).all() and np.array_equal(got[~skip], want[~skip]) and np.array_equal(got, again)
    assert (want[skip][..., 3] == 255).all()     # (the full result has no zero alpha there: the zeros above are the fill)


def test_a_mesh_that_hides_everything_writes_nothing(gpu):
    torch = gpu
    import openvr_fsr_amd as A
    iw, ih, ow, oh = S1
    for cfg in (dict(M), dict(U), dict(M, fused=1), dict(U, use_nis=1), dict(M, stage_mask=1)):
        pp = A.PostProcessor(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, **cfg)
        try:
            texs = [_source(torch, "rgba8", iw, ih, synth.seed_for(7, i))[0] for i in range(2)]
            for eye in (0, 1):
                pp.set_hidden_area(eye, R.EVERYTHING)
            outs, raw = _outputs(torch, 2, oh, ow, torch.uint8, 4)
            _launch(torch, pp, "apply", texs, None, outs)      # returns OK (a failure raises)
            pp.apply_batch(torch.stack(texs), outs)
            torch.cuda.synchronize()
            total, skipped = pp.hidden_area_stats(0)
            assert total == skipped > 0
            assert (raw.cpu().numpy() == 0xA5).all(), cfg
        finally:
            pp.close()


def test_set_hidden_area_between_the_eyes_of_a_pair(gpu):
    """a recorded first eye is dropped, as ovrfsr_set_config drops it: its destination is never written, and the eyes submitted afterwards
    are processed without it, under the new mesh"""
    torch = gpu
    import openvr_fsr_amd as A
    iw, ih, ow, oh = S1
    texs = [_source(torch, "rgba8", iw, ih, synth.seed_for(8, i))[0] for i in range(2)]
    pp = A.PostProcessor(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, pair_submit=1, **M)
    ref = A.PostProcessor(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, **M)
    try:
        dropped, dropped_raw = _outputs(torch, 1, oh, ow, torch.uint8, 4)
        pp.apply(0, texs[0], out=dropped[0])
        assert pp.pair_pending()
        pp.set_hidden_area(1, R.MESH[1])
        assert not pp.pair_pending()
        outs, raw = _outputs(torch, 2, oh, ow, torch.uint8, 4)
        pp.apply(1, texs[1], out=outs[1])
        pp.apply(0, texs[0], out=outs[0])
        torch.cuda.synchronize()
        assert not pp.pair_pending()
        want, want_raw = _outputs(torch, 2, oh, ow, torch.uint8, 4)
        for eye in (0, 1):
            ref.apply(eye, texs[eye], out=want[eye])
        torch.cuda.synchronize()
    finally:
        pp.close()
        ref.close()
    assert (dropped_raw.cpu().numpy() == 0xA5).all()
    got, want = raw.cpu().numpy(), want_raw.cpu().numpy()
    skip = _pixel_mask(R.hidden_tiles(R.MESH[1], ow, oh), 32, 32, oh, ow, 4)
    assert np.array_equal(got[0], want[0])                     # the left eye has no mesh
    assert np.array_equal(got[1][~skip], want[1][~skip]) and (got[1][skip] == 0xA5).all()
