"""The hidden-area mesh without a GPU (include/openvr_fsr_amd.h, "hidden-area mesh"): (a) the classification rule, ovrfsr_hidden_tiles through
the built library against a numpy brute-force restatement (tests/hidden_ref.py) and known answers; (b) the planner under a mesh,
tests/debug/hidden_probe.cpp linked from the planner's three sources under AddressSanitizer and UBSan as a stand-alone program: list
structure, spans, RCAS neighbours, the plan without a mesh unchanged, the form unchanged, and every plan's digest the one recorded before the
tile lists were built in steps (tests/golden/plan_digests_parent.json); (c) the C boundary: symbols and refusals."""
import ctypes as C
import shutil

import numpy as np
import pytest

import openvr_fsr_amd as A
from openvr_fsr_amd import _capi as K
from tests import hidden_ref as R
from tests import test_pipeline_plan as TP

f32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)


# ---- (a) the rule ------------------------------------------------------------------------------------------------------------------------
def random_mesh(rng, W, H, tw, th):
    """1..8 triangles: free vertices in [-0.3, 1.3] (either winding), large ones that hide whole tiles, vertices exactly on pixel centres and
    tile corners, degenerate triangles (a repeated vertex, three collinear ones), a copy of an earlier triangle (overlap), far-out vertices
    (beyond the [-4, 4] clamp)"""
    tris = []
    for _ in range(int(rng.integers(1, 9))):
        kind = int(rng.integers(0, 8))
        if kind == 0:      # large: most of a half plane
            t = rng.uniform(-0.5, 1.5, (3, 2))
            t[int(rng.integers(0, 3))] = rng.uniform(-3.0, 4.0, 2)
        elif kind == 1:    # vertices on pixel centres
            t = np.stack([(rng.integers(0, W, 3) + 0.5) / W, (rng.integers(0, H, 3) + 0.5) / H], 1)
        elif kind == 2:    # vertices on tile corners
            t = np.stack([rng.integers(0, (W + tw - 1) // tw + 1, 3) * tw / W, rng.integers(0, (H + th - 1) // th + 1, 3) * th / H], 1)
        elif kind == 3:    # degenerate: a repeated vertex or three collinear ones
            t = rng.uniform(0.0, 1.0, (3, 2))
            if rng.integers(0, 2):
                t[2] = t[0]
            else:
                t[2] = t[0] + 2.0 * (t[1] - t[0])
        elif kind == 4 and tris:   # overlapping: an earlier triangle again, slightly moved and with the other winding
            t = tris[int(rng.integers(0, len(tris)))][::-1] + rng.uniform(-0.05, 0.05, 2)
        elif kind == 5:    # far out: clamped to [-4, 4]
            t = rng.uniform(-0.3, 1.3, (3, 2))
            t[int(rng.integers(0, 3))] *= 50.0
        elif kind == 6:    # an axis-aligned corner wedge, as a headset's mesh has them
            a, b = rng.uniform(0.2, 0.9, 2)
            cx, cy = rng.integers(0, 2, 2)
            t = np.array([(cx, cy), (cx + (a if cx == 0 else -a), cy), (cx, cy + (b if cy == 0 else -b))], float)
        else:
            t = rng.uniform(-0.3, 1.3, (3, 2))
        tris.append(np.asarray(t, np.float64))
    return np.asarray(tris, np.float32)


SHAPES = [(160, 128), (200, 147), (320, 267)]
TILES = [(32, 32), (32, 24)]


@pytest.mark.parametrize("tile", TILES, ids=["%dx%d" % t for t in TILES])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_rule_against_brute_force(shape, tile):
    """36 seeded meshes per (shape, tile size): 216 in all"""
    W, H = shape
    tw, th = tile
    hidden_some = 0
    for seed in range(36):
        rng = np.random.default_rng(1000 * W + 10 * th + seed)
        mesh = random_mesh(rng, W, H, tw, th)
        want = R.hidden_tiles(mesh, W, H, tw, th)
        got = K.hidden_tiles(mesh, W, H, tw, th)
        assert np.array_equal(got, want), (seed, mesh.tolist(), got.tolist(), want.tolist())
        hidden_some += int(want.any() and not want.all())
    assert hidden_some >= 10, hidden_some   # (the generator does produce meshes that hide some tiles and not others)


@pytest.mark.parametrize("shape", [(1, 1), (16384, 16)], ids=["1x1", "16384x16"])
def test_rule_extreme_shapes(shape):
    W, H = shape
    for seed in range(6):
        rng = np.random.default_rng(77 + seed)
        mesh = random_mesh(rng, W, H, 32, 32)
        for tw, th in TILES:
            assert np.array_equal(K.hidden_tiles(mesh, W, H, tw, th), R.hidden_tiles(mesh, W, H, tw, th)), (seed, tw, th)
    for mesh in (R.EVERYTHING, np.asarray([[(0.0, 0.0), (0.5, 0.0), (0.0, 1.0)]], np.float32)):
        assert np.array_equal(K.hidden_tiles(mesh, W, H), R.hidden_tiles(mesh, W, H))


def test_known_answers():
    assert not K.hidden_tiles(None, 160, 128).any()                            # an empty mesh hides nothing
    assert not K.hidden_tiles(np.zeros((0, 3, 2), np.float32), 200, 147, 32, 24).any()
    for W, H in SHAPES:
        for tw, th in TILES:                                                   # one triangle over the whole image hides every tile
            assert K.hidden_tiles([[(-1, -1), (3, -1), (-1, 3)]], W, H, tw, th).all()
            assert K.hidden_tiles([[(-1, -1), (-1, 3), (3, -1)]], W, H, tw, th).all()   # (the other winding)
    h = K.hidden_tiles([[(0, 0), (0.45, 0), (0, 0.6)]], 160, 128)
    assert h[0, 0] == 1 and h[1, 1] == 0
    assert h.tolist() == R.hidden_tiles([[(0, 0), (0.45, 0), (0, 0.6)]], 160, 128).tolist()
    # edges are inclusive: a triangle whose edge runs through the centres of a tile's last pixel column still hides the tile ...
    e = (31 + 0.5) / 160
    assert K.hidden_tiles(R.rect(0.0, 0.0, e, 1.0), 160, 128)[:, 0].all()
    # ... and one 1/256 pixel short of them does not
    short = (31 + 0.5 - 1 / 256) / 160
    assert not K.hidden_tiles(R.rect(0.0, 0.0, short, 1.0), 160, 128).any()
    # a degenerate triangle covers nothing, not even the pixel centres on its line
    assert not K.hidden_tiles([[(0, 0.5 / 128), (1, 0.5 / 128), (0.5, 0.5 / 128)]], 160, 128, 160, 1).any()


def test_the_test_meshes_hide_something_everywhere():
    for W, H in SHAPES:
        for eye in (0, 1):
            h = K.hidden_tiles(R.MESH[eye], W, H)
            assert h.any() and not h.all() and R.partly_covered(R.MESH[eye], W, H).any()
            assert np.array_equal(h, R.hidden_tiles(R.MESH[eye], W, H))


# ---- (b) the planner -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe():
    """the probe; every line it plans is compared with the recorded digest of the parent commit's plan (ids unique per call)"""
    build = R.build_probe()

    def run(lines):
        plans = build(lines)
        TP.assert_parent_digests("hidden_probe", plans)
        return plans

    yield run
    shutil.rmtree(build.tmp, ignore_errors=True)


def _no_mesh_lines():
    return [R.with_mesh(line) for _, line, _ in TP.FORM_TABLE]


def test_plan_without_a_mesh_is_unchanged(probe):
    """every row of test_pipeline_plan.FORM_TABLE: the six-argument call and the call with an empty mesh give the same plan, field by field
    (lists, records, spans, taps and form included), and the same refusal"""
    got = probe(_no_mesh_lines())
    for (name, _, want), g in zip(TP.FORM_TABLE, got):
        assert g["no_mesh_equal"] == 1, name
        assert g["status"] == want.get("status", 0), name
        if g["status"] == 0:
            assert g["hidden_area"] == 0 and g["skipped"] == [0, 0] and g["form"] == g["form_plain"], name
            assert g["tile_lists"] == want.get("tile_lists", g["tile_lists"]), name


M = dict(radius=0.5, proj_centre=(0.2, 0.3, 0.8, 0.7))
PLAN_SHAPES = [(80, 64, 160, 128), (150, 110, 200, 147), (240, 200, 320, 267)]
# name, format, one eye per texture, configuration, skips (does the form walk lists), two-kernel form (RCAS reads EASU's intermediate)
PLAN_FORMS = [
    ("two-pass unmasked", TP.RGBA8, 1, dict(radius=2.0), True, True),
    ("two-pass masked", TP.RGBA8, 1, dict(M, fused=0), True, True),
    ("two-pass 10-bit masked", TP.RGB10A2, 1, dict(M), True, True),
    ("mask-sorted", TP.RGBA8, 1, dict(M), True, True),
    ("mask-sorted shared", TP.RGBA8, 0, dict(M), True, True),
    ("exact masked", TP.RGBA8, 1, dict(M, precision=3), True, True),
    ("exact unmasked", TP.RGBA8, 1, dict(radius=2.0, precision=3), True, True),
    ("easu only", TP.RGBA8, 1, dict(radius=2.0, stage_mask=1), True, False),
    ("easu only masked", TP.RGBA8, 1, dict(M, stage_mask=1), True, False),
    ("fused", TP.RGBA8, 1, dict(radius=2.0, fused=1), True, False),
    ("fused masked", TP.RGBA8, 1, dict(M, fused=1), True, False),
    ("half masked", TP.RGBA16F, 1, dict(M), True, False),
    ("half unmasked", TP.RGBA16F, 1, dict(radius=2.0), True, True),
    ("nis", TP.RGBA8, 1, dict(radius=2.0, use_nis=1), True, False),
    ("nis masked shared", TP.RGBA16F, 0, dict(M, use_nis=1), True, False),
    ("strict", TP.RGBA8, 1, dict(M, precision=2), False, False),
]


def _plan_line(name, fmt, one_eye, shape, cfg, mesh="mesh"):
    """(the id names form, shape and mesh: unique over this file, as the digest record needs it)"""
    iw, ih, ow, oh = shape
    return TP._line("%s/%dx%d-%dx%d/%s" % ((name,) + tuple(shape) + (mesh,)), fmt, iw, ih, one_eye, -1, fsr_enabled=1, out_width=ow, out_height=oh,
                    sharpness=0.9, **cfg)


# the lines the tests below plan, each behind a name: test_digest_record_names_these_lines reads the same functions
def _mesh_lines(shape):
    return [R.with_mesh(_plan_line(n, f, one, shape, cfg), R.MESH[0], R.MESH[1]) for n, f, one, cfg, _, _ in PLAN_FORMS]


def _shared_or_not_lines():
    line, other = (_plan_line("shared-or-not", TP.RGBA8, 1, PLAN_SHAPES[0], dict(radius=2.0), mesh) for mesh in ("same", "different"))
    return [R.with_mesh(line, R.MESH[0], R.MESH[0]), R.with_mesh(other, R.MESH[0], R.MESH[1])]


def _everything_lines():
    return [R.with_mesh(_plan_line(n, f, one, PLAN_SHAPES[1], cfg, "everything"), R.EVERYTHING, R.EVERYTHING) for n, f, one, cfg, skips, _ in PLAN_FORMS if skips]


def _left_only_lines():
    return [R.with_mesh(_plan_line("left-only", TP.RGBA8, 1, PLAN_SHAPES[0], dict(M), "left"), R.MESH[0], None)]


@pytest.mark.parametrize("shape", PLAN_SHAPES, ids=["%dx%d-%dx%d" % s for s in PLAN_SHAPES])
def test_lists_under_a_mesh(probe, shape):
    lines = _mesh_lines(shape)
    ow, oh = shape[2:]
    for (name, _, one, cfg, skips, two_kernel), p in zip(PLAN_FORMS, probe(lines)):
        assert p["status"] == 0 and p["form"] == p["form_plain"], (name, p["form"], p["form_plain"])   # the mesh never changes the form
        if not skips:
            assert p["hidden_area"] == 0 and p["skipped"] == [0, 0], name
            continue
        assert p["hidden_area"] == 1 and p["tile_lists"] == 1, name
        tw, th = p["tile"]
        tx = (ow + tw - 1) // tw
        ty = p["tiles"] // tx
        for eye in (0, 1):
            # the probe's map is the rule's (and each pixel of a shared texture is tested against the mesh of its own half)
            want = R.hidden_tiles(R.MESH[eye], ow, oh, tw, th) if one else R.hidden_tiles_shared(R.MESH[0], R.MESH[1], ow, oh, tw, th)
            hidden = np.asarray(p["hidden"][eye], np.uint8).reshape(ty, tx)
            assert np.array_equal(hidden, want), (name, eye)
            hid = set(np.flatnonzero(hidden.reshape(-1)).tolist())
            inside, ring, outside, rcas = (p[k][eye] for k in ("inside", "ring", "outside", "rcas"))
            # inside + outside + skipped: every tile once
            assert p["skipped"][eye] == len(hid) > 0, name
            assert len(set(inside)) == len(inside) and len(set(outside)) == len(outside) and not set(inside) & set(outside), name
            assert sorted(set(inside) | set(outside) | hid) == list(range(p["tiles"])), name
            assert not (set(inside) | set(outside)) & hid, name            # no entry is hidden ...
            assert not set(rcas) & hid, name
            if not two_kernel:
                assert not set(ring) & hid, name                           # ... except ring entries, and those in the two-kernel forms only
                continue
            # what RCAS processes: the inside tiles; in the two-pass form every tile that is not hidden
            want_rcas = set(inside) | set(outside) if p["form"] == "two-pass" else set(inside)
            assert set(rcas) == want_rcas and len(rcas) == len(want_rcas), name
            # every RCAS tile's four edge neighbours are written by an EASU-stage launch (inside | ring; two-pass: the outside launch
            # writes the intermediate too) or lie off the image
            easu = set(inside) | set(ring) | (set(outside) if p["form"] == "two-pass" else set())
            for t in rcas:
                x, y = t % tx, t // tx
                for nx, ny in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
                    if 0 <= nx < tx and 0 <= ny < ty:
                        assert ny * tx + nx in easu, (name, eye, t, (nx, ny))
            # a hidden ring tile touches an RCAS tile
            for t in set(ring) & hid:
                x, y = t % tx, t // tx
                assert any(0 <= nx < tx and 0 <= ny < ty and ny * tx + nx in want_rcas for nx, ny in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1))), (name, t)
            assert set(ring) & hid, name   # (these meshes do put hidden tiles next to processed ones)
            # spans (cut for every plan of 32x32 tiles; RCAS walks them where it reads RGBA8): they cover exactly the RCAS tiles' pixels, once
            assert th == 32 and p["spans"][eye], name
            covered = np.zeros((ty, ow), np.int32)
            for x0, row, x_end in p["spans"][eye]:
                assert 0 < x_end - x0 <= 62 and x_end <= ow and row < ty, name
                covered[row, x0:x_end] += 1
            expect = np.zeros((ty, ow), np.int32)
            for t in rcas:
                expect[t // tx, (t % tx) * tw:(t % tx + 1) * tw] = 1
            assert np.array_equal(covered, expect), (name, eye)
        if not one:
            assert p["lists_shared"] == 1, name


def test_lists_shared_compares_the_final_lists(probe):
    """unmasked, one eye per texture: equal meshes give shared lists, different meshes do not"""
    same, different = probe(_shared_or_not_lines())
    assert same["lists_shared"] == 1 and different["lists_shared"] == 0


def test_everything_hidden_plans_no_launch(probe):
    for p in probe(_everything_lines()):
        assert p["status"] == 0 and p["form"] == p["form_plain"], p["id"]
        for eye in (0, 1):
            assert p["skipped"][eye] == p["tiles"], p["id"]
            assert p["inside"][eye] == p["ring"][eye] == p["outside"][eye] == p["rcas"][eye] == p["spans"][eye] == [], p["id"]


def test_one_eye_without_a_mesh(probe):
    """a mesh for the left eye only: the right eye's lists hold every tile"""
    p = probe(_left_only_lines())[0]
    assert p["hidden_area"] == 1 and p["skipped"][0] > 0 and p["skipped"][1] == 0
    assert len(p["inside"][1]) + len(p["outside"][1]) == p["tiles"]


def test_digest_record_names_these_lines():
    """the ids of the lines planned above are unique over the file, and the record holds no hidden_probe id that none of them has"""
    lines = _no_mesh_lines() + [line for shape in PLAN_SHAPES for line in _mesh_lines(shape)] + _shared_or_not_lines() + _everything_lines() + _left_only_lines()
    ids = [line.split(" ", 1)[0] for line in lines]
    assert len(set(ids)) == len(ids), sorted(i for i in set(ids) if ids.count(i) > 1)
    assert set(TP.parent_digests("hidden_probe")) <= set(ids)


# ---- (c) the C boundary ----------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported():
    lib = C.CDLL(A.library_path())
    for name in ("ovrfsr_set_hidden_area", "ovrfsr_hidden_area_stats", "ovrfsr_hidden_tiles"):
        assert hasattr(lib, name), name


def test_refusals_need_no_ctx():
    L = A.library()
    tri = np.asarray([0, 0, 1, 0, 0, 1], np.float32)
    total, skipped = C.c_uint32(7), C.c_uint32(7)
    assert L.ovrfsr_set_hidden_area(None, 0, tri.ctypes.data_as(f32p), 1) == 1             # NULL ctx
    assert L.ovrfsr_hidden_area_stats(None, 0, C.byref(total), C.byref(skipped)) == 1 and (total.value, skipped.value) == (7, 7)
    hidden = np.full(20, 9, np.uint8)
    hp = hidden.ctypes.data_as(u8p)
    assert L.ovrfsr_hidden_tiles(tri.ctypes.data_as(f32p), 1, 160, 128, 32, 32, hp, 20) == 0 and hidden.max() <= 1
    hidden[:] = 9
    assert L.ovrfsr_hidden_tiles(tri.ctypes.data_as(f32p), 1, 160, 128, 32, 32, hp, 19) == 1   # hidden_len too small
    for bad in (np.nan, np.inf, -np.inf):
        t = tri.copy()
        t[3] = bad
        assert L.ovrfsr_hidden_tiles(t.ctypes.data_as(f32p), 1, 160, 128, 32, 32, hp, 20) == 1  # a non-finite coordinate
    assert L.ovrfsr_hidden_tiles(None, 1, 160, 128, 32, 32, hp, 20) == 1                        # NULL with a count
    many = np.zeros(6 * 4097, np.float32)
    assert L.ovrfsr_hidden_tiles(many.ctypes.data_as(f32p), 4097, 160, 128, 32, 32, hp, 20) == 1  # more than 4096 triangles
    assert L.ovrfsr_hidden_tiles(many.ctypes.data_as(f32p), 4096, 160, 128, 32, 32, hp, 20) == 0
    hidden[:] = 9
    for w, h, tw, th in ((0, 128, 32, 32), (160, 0, 32, 32), (16385, 128, 32, 32), (160, 128, 0, 32), (160, 128, 32, 0)):
        assert L.ovrfsr_hidden_tiles(tri.ctypes.data_as(f32p), 1, w, h, tw, th, hp, 20) == 1
    assert L.ovrfsr_hidden_tiles(tri.ctypes.data_as(f32p), 1, 160, 128, 32, 32, None, 20) == 1
    assert (hidden == 9).all()   # nothing written by any refused call
