"""The mask feather on the GPU (header, "mask feather").  The contract is a composition, exact to the byte: every byte of a feathered apply
equals, for band pixels, store(o + (s - o) * t) evaluated in numpy float32 and, for every other pixel, the byte of the feather-off apply --
s: the same call with width 0 on the same ctx and build; o: the CPU oracle's outside-branch value (oracle.easu with the mask moved off the
image, tests/forms_model.py's store conversions for the intermediate and the destination, oracle.rcas's debug tint between them); w8: the
numpy restatement of the rule (tests/test_mask_feather.py).  Then the call shapes the pass has to follow: batches, pair_submit, a moving
gaze, a re-scale, capture and replay, a hidden-area mesh, the HDR domain; what ignores the setting; and the checked build."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import forms_model as FM
from tests import hdrmap
from tests import hidden_ref
from tests.test_mask_feather import band, feather_px, rule

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROJ = (0.2, 0.3, 0.8, 0.7)
RADIUS, WIDTH, SHARPNESS = 0.9, 0.3, 0.9
A_SHAPE, B_SHAPE, SHARED_SHAPE = (96, 80, 128, 107), (37, 29, 49, 39), (192, 80, 256, 107)
EDGE_GAZE = (1.05, 0.4)   # the disc's centre behind the right edge: a sliver of it on the image
# kind -> (shape, one eye per texture, gaze of eye 0 or None)
KINDS = {"A": (A_SHAPE, True, None), "B": (B_SHAPE, True, None), "shared": (SHARED_SHAPE, False, None), "edge": (A_SHAPE, True, EDGE_GAZE)}
SRCS = ("rgba8", "bgra8", "rgba16f", "rgba32f", "rgb10a2", "r11g11b10f", "ms4_rgba8")
DESTS = {"rgb10a2": ("rgb10a2", "rgba32f", "owned")}
DESTS_DEFAULT = ("rgba8", "rgba16f", "rgba32f", "owned")


def _R():
    return FM.record_forms()


# ---- the expectation ---------------------------------------------------------------------------------------------------------------------
def outside_value(x, pf, shape, sharpen, mid, dst, sharpness, debug):
    """o: float32 [oh, ow, 4], decoded from the destination format (x: the image the pipeline sees, tests/forms_model.decoded)"""
    iw, ih, ow, oh = shape
    nowhere, nothing = np.zeros(4, np.uint32), np.asarray([0, 0, ow, oh], np.uint32)   # every group centre is farther than 0 from (0, 0)
    o = O.easu(FM._to_float(x, pf), ow, oh, O.easu_con(iw, ih, ow, oh), nowhere, nothing)
    if sharpen:
        o = O.rcas(FM._requantise(o, mid), O.rcas_con(sharpness, debug), nowhere, nothing)
    return FM._requantise(o, dst)


def blended(s_arr, o, w8, inside, dst):
    """the feathered image from the feather-off image s_arr (the destination's own array), o and the rule"""
    s = FM._to_float(s_arr, dst)
    t = (w8.astype(np.float32) / np.float32(256))[..., None]
    v = o[..., :3] + (s[..., :3] - o[..., :3]) * t                      # float32 throughout: every operator rounded once
    v = np.concatenate([v, s[..., 3:4]], axis=2).astype(np.float32)
    enc = FM.encode(v, dst)
    b = band(w8, inside)
    if dst == "rgb10a2":   # packed words: alpha keeps its two stored bits
        enc = ((enc.view(np.uint32) & np.uint32(0x3FFFFFFF)) | (s_arr.view(np.uint32) & np.uint32(0xC0000000))).view(np.int32)
        return np.where(b, enc, s_arr), b
    enc[..., 3] = s_arr[..., 3]
    return np.where(b[..., None], enc, s_arr), b


def mask_of(A, shape, one_eye, eye, proj, radius, width):
    _, _, ow, oh = shape
    centre, rad = A.mask_constants(ow, oh, proj, radius, one_eye, eye)
    return centre, int(rad[0]), feather_px(width, oh)


def expected(A, s_arr, src, seed, content, shape, one_eye, eye, proj, cfg, dst, width=WIDTH):
    plan = FM.Plan(dict(cfg=dict(cfg, out_width=shape[2], out_height=shape[3]), src=src, kind="apply" if one_eye else "shared", shape=shape, dst=dst))
    assert plan.upscale and not plan.nis
    x = FM.decoded(src, shape[0], shape[1], seed, content)
    o = outside_value(x, plan.pf, shape, plan.sharpen, plan.mid, plan.dst, plan.sharpness, cfg.get("debug_mode", 0))
    centre, R, F = mask_of(A, shape, one_eye, eye, proj, cfg["radius"], width)
    w8, inside = rule(centre, R, F, shape[2], shape[3])
    return blended(s_arr, o, w8, inside, plan.dst) + (o, w8)


# ---- running --------------------------------------------------------------------------------------------------------------------------
def _host(torch, t):
    torch.cuda.synchronize()
    return t.contiguous().cpu().numpy().copy()


def _apply(torch, pp, src, seed, content, shape, one_eye, eye, dst, out=None):
    """one image through apply (or apply_batch_shared) -> the destination as numpy"""
    R = _R()
    iw, ih, ow, oh = shape
    tex, fmt = R._source(src, iw, ih, seed, content)
    if out is None and dst != "owned":
        out = R._dest(dst, ow, oh)[0]
    if one_eye:
        return _host(torch, pp.apply(eye, tex, out=out, in_format=fmt))
    assert out is not None
    pp.apply_batch(tex[None], out[None], in_format=fmt, shared=True)
    return _host(torch, out)


def _ctx(A, shape, **cfg):
    kw = dict(fsr_enabled=1, out_width=shape[2], out_height=shape[3], sharpness=SHARPNESS, radius=RADIUS, proj_centre=PROJ)
    kw.update(cfg)
    return A.PostProcessor(**kw), kw


# ---- 1. the matrix ---------------------------------------------------------------------------------------------------------------------
def configs():
    ci = 0
    for fused in (-1, 0, 1):
        for stage_mask in (0, 1):
            for q in (0, 1):
                for rf in (0, 1):
                    yield ci, dict(fused=fused, stage_mask=stage_mask, quantize_intermediate=q, reference_formats=rf)
                    ci += 1


def matrix(torch, A, si, kinds=tuple(KINDS)):
    """source SRCS[si] through every configuration, the shape, destination, precision and debug_mode rotated with the configuration and the
    source, so that every configuration meets every shape and every destination across the sources.  -> (cases, launched, failures)"""
    src = SRCS[si]
    dests = DESTS.get(src, DESTS_DEFAULT)
    ran, launched, bad = 0, 0, []
    for ci, cfg in configs():
        kind = kinds[(ci + si) % len(kinds)]
        shape, one_eye, gaze = KINDS[kind]
        dst = dests[(ci // 4 + ci + si) % len(dests)]
        if not one_eye and dst == "owned":
            dst = dests[0]
        cfg = dict(cfg, precision=(0, 2, 3)[(ci + 2 * si) % 3], debug_mode=((ci + si) // 2) % 2)
        eye = 0 if gaze or not one_eye else (ci + si) % 2
        seed, content = 3 + (ci + si) % 5, ("structured", "random")[(ci + si) % 2]
        pp, kw = _ctx(A, shape, **cfg)
        ran += 1
        try:
            if gaze:
                pp.set_gaze(0, *gaze)
            try:
                s_arr = _apply(torch, pp, src, seed, content, shape, one_eye, eye, dst)
            except A.OvrFsrError:
                continue   # a combination the library refuses with or without a feather (counted below)
            assert pp.mask_feather_stats() == 0
            pp.set_mask_feather(WIDTH)
            got = _apply(torch, pp, src, seed, content, shape, one_eye, eye, dst)
            launches = pp.mask_feather_stats()
        finally:
            pp.close()
        launched += 1
        proj = (gaze + PROJ[2:]) if gaze else PROJ
        want, b, _, _ = expected(A, s_arr, src, seed, content, shape, one_eye, eye, proj, kw, dst)
        differ = int((got != want).reshape(got.shape[0], got.shape[1], -1).any(axis=2).sum())
        if differ or launches != 1 or not b.any():
            bad.append((src, kind, dst, cfg, "pixels differing: %d of %d band pixels, launches %d" % (differ, int(b.sum()), launches)))
    return ran, launched, bad


@pytest.mark.parametrize("si", range(len(SRCS)), ids=SRCS)
def test_every_byte_is_the_composition(gpu, si):
    import openvr_fsr_amd as A
    ran, launched, bad = matrix(gpu, A, si)
    print("mask feather, %s: %d cases, %d launched, %d differ" % (SRCS[si], ran, launched, len(bad)))
    assert launched * 3 > ran, (ran, launched)   # not a list of refusals (RGB10A2 has no fused form, exact stores only RGBA8 destinations)
    assert not bad, bad[:4]


# ---- 2. not trivial ---------------------------------------------------------------------------------------------------------------------
def test_the_band_is_where_the_rule_says_and_the_blend_is_a_blend(gpu):
    import openvr_fsr_amd as A
    torch = gpu
    pp, kw = _ctx(A, A_SHAPE)
    try:
        s_arr = _apply(torch, pp, "rgba8", 11, "random", A_SHAPE, True, 0, "rgba8")
        pp.set_mask_feather(WIDTH)
        got = _apply(torch, pp, "rgba8", 11, "random", A_SHAPE, True, 0, "rgba8")
    finally:
        pp.close()
    want, b, o, w8 = expected(A, s_arr, "rgba8", 11, "random", A_SHAPE, True, 0, PROJ, kw, "rgba8")
    assert np.array_equal(got, want)
    assert int(b.sum()) == 4119
    changed = (got != s_arr).any(axis=2)
    assert not (changed & ~b).any()
    o8 = FM.encode(o, "rgba8")
    ramp = b & (w8 > 0)
    off_both = (got[..., :3] != s_arr[..., :3]).any(axis=2) & (got[..., :3] != o8[..., :3]).any(axis=2)
    print("band pixels changed: %.3f; ramp pixels off both ends: %.3f" % (changed[b].mean(), off_both[ramp].mean()))
    assert changed[b].mean() >= 0.90
    assert off_both[ramp].mean() >= 0.80
    assert np.array_equal(got[b & (w8 == 0)][:, :3], o8[b & (w8 == 0)][:, :3])   # along the staircase: exactly o


# ---- 3. call shapes ---------------------------------------------------------------------------------------------------------------------
def test_a_batch_of_five_alternating_eyes_with_a_row_gap(gpu):
    import openvr_fsr_amd as A
    torch = gpu
    R = _R()
    iw, ih, ow, oh = A_SHAPE
    texs = torch.stack([R._source("rgba8", iw, ih, 20 + i, "structured")[0] for i in range(5)])
    big = torch.full((5, oh + 3, ow, 4), 0xA5, dtype=torch.uint8, device="cuda")
    outs = big[:, :oh]
    pp, kw = _ctx(A, A_SHAPE)
    try:
        pp.apply_batch(texs, outs, first_eye=1)
        s_all = _host(torch, outs)
        pp.set_mask_feather(WIDTH)
        pp.apply_batch(texs, outs, first_eye=1)
        got = _host(torch, outs)
        assert pp.mask_feather_stats() == 2          # two eye passes (the eyes' centres differ)
    finally:
        pp.close()
    assert (_host(torch, big)[:, oh:] == 0xA5).all()
    for i in range(5):
        want, b, _, _ = expected(A, s_all[i], "rgba8", 20 + i, "structured", A_SHAPE, True, 1 ^ (i & 1), PROJ, kw, "rgba8")
        assert b.any() and np.array_equal(got[i], want), i


def test_pair_submit_launches_with_the_width_at_its_second_call(gpu):
    import openvr_fsr_amd as A
    torch = gpu
    R = _R()
    iw, ih, ow, oh = A_SHAPE
    texs = [R._source("rgba16f", iw, ih, 30 + e, "structured")[0] for e in (0, 1)]
    pp, kw = _ctx(A, A_SHAPE, pair_submit=1)
    try:
        outs = [torch.zeros((oh, ow, 4), dtype=torch.float16, device="cuda") for _ in (0, 1)]
        for e in (0, 1):
            pp.apply(e, texs[e], out=outs[e])
        s_all = [_host(torch, o) for o in outs]
        pp.apply(0, texs[0], out=outs[0])
        assert pp.pair_pending()
        pp.set_mask_feather(WIDTH)                   # between the two calls of the pair: no recorded eye dropped, both eyes feathered
        assert pp.pair_pending()
        pp.apply(1, texs[1], out=outs[1])
        assert not pp.pair_pending() and pp.mask_feather_stats() == 2
        got = [_host(torch, o) for o in outs]
    finally:
        pp.close()
    for e in (0, 1):
        want, b, _, _ = expected(A, s_all[e], "rgba16f", 30 + e, "structured", A_SHAPE, True, e, PROJ, kw, "rgba16f")
        assert b.any() and np.array_equal(got[e].view(np.uint16), want.view(np.uint16)), e


def test_the_band_follows_a_gaze(gpu):
    import openvr_fsr_amd as A
    torch = gpu
    gazes = ((0.3, 0.4), (0.6, 0.55), (0.62, 0.5))
    stats, images = [], []
    for width in (0.0, WIDTH):
        pp, kw = _ctx(A, A_SHAPE)
        try:
            pp.set_mask_feather(width)
            frames = []
            for g in gazes:
                pp.set_gaze(0, *g)
                frames.append(_apply(torch, pp, "rgba8", 5, "structured", A_SHAPE, True, 0, "rgba8"))
            stats.append(pp.gaze_stats())
            images.append(frames)
            assert pp.mask_feather_stats() == (len(gazes) if width else 0)
        finally:
            pp.close()
    assert stats[0] == stats[1] and stats[0][0] >= 1          # the feather changes nothing about re-aims and rebuilds
    bands = []
    for g, s_arr, got in zip(gazes, images[0], images[1]):
        want, b, _, _ = expected(A, s_arr, "rgba8", 5, "structured", A_SHAPE, True, 0, g + PROJ[2:], kw, "rgba8")
        assert np.array_equal(got, want), g
        bands.append(b)
    assert (bands[0] != bands[1]).any()


def test_a_rescale_in_place(gpu):
    import openvr_fsr_amd as A
    torch = gpu
    # (the first steps of the ladder tests/test_dynamic_resolution.py shows to be re-scales in place, under its mask)
    sizes, out_size = ((80, 64), (120, 96), (107, 86)), (160, 128)
    images = []
    for width in (0.0, WIDTH):
        pp, kw = _ctx(A, sizes[0] + out_size, radius=0.5)
        try:
            pp.set_max_input_size(152, 120)
            pp.set_mask_feather(width)
            images.append([_apply(torch, pp, "rgba8", 6, "structured", size + out_size, True, 0, "rgba8") for size in sizes])
            assert pp.rescale_stats() == (2, 0)
        finally:
            pp.close()
    for size, s_arr, got in zip(sizes, images[0], images[1]):
        want, b, _, _ = expected(A, s_arr, "rgba8", 6, "structured", size + out_size, True, 0, PROJ, kw, "rgba8")
        assert b.any() and np.array_equal(got, want), size


def test_capture_and_replay(gpu):
    import openvr_fsr_amd as A
    torch = gpu
    R = _R()
    iw, ih, ow, oh = A_SHAPE
    tex, _ = R._source("rgba8", iw, ih, 7, "structured")
    out = torch.zeros((oh, ow, 4), dtype=torch.uint8, device="cuda")
    pp, kw = _ctx(A, A_SHAPE)
    try:
        s_arr = _host(torch, pp.apply(0, tex, out=out))
        stream = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                pp.set_mask_feather(WIDTH)           # the setter and the apply behind it are accepted under capture: the pass builds nothing
                pp.apply(0, tex, out=out)
        torch.cuda.synchronize()
        pp.set_mask_feather(0.0)                     # the graph replays the width it was captured with
        out.zero_()
        graph.replay()
        got = _host(torch, out)
    finally:
        pp.close()
    want, b, _, _ = expected(A, s_arr, "rgba8", 7, "structured", A_SHAPE, True, 0, PROJ, kw, "rgba8")
    assert b.any() and np.array_equal(got, want)


def test_skipped_tiles_of_a_hidden_area_mesh_keep_their_bytes(gpu):
    import openvr_fsr_amd as A
    torch = gpu
    shape = (150, 110, 200, 147)
    iw, ih, ow, oh = shape
    R = _R()
    tex, _ = R._source("rgba8", iw, ih, 8, "structured")
    images = []
    for gaze in (None, (0.45, 0.5)):                 # (with a gaze: the maps the planner leaves; without: rasterised for the bitmap)
        pp, kw = _ctx(A, shape, radius=0.7, proj_centre=(0.4, 0.45, 0.6, 0.55))
        try:
            pp.set_hidden_area(0, hidden_ref.MESH[0])
            if gaze:
                pp.set_gaze(0, *gaze)
            pair = []
            for width in (0.0, WIDTH):
                pp.set_mask_feather(width)
                out = torch.full((oh, ow, 4), 0xA5, dtype=torch.uint8, device="cuda")
                pair.append(_host(torch, pp.apply(0, tex, out=out)))
            skipped = pp.hidden_area_stats(0)[1]
            assert skipped > 0 and pp.mask_feather_stats() == 1
        finally:
            pp.close()
        tiles = hidden_ref.hidden_tiles(hidden_ref.MESH[0], ow, oh, 32, 32)
        skip = np.kron(tiles, np.ones((32, 32), np.uint8))[:oh, :ow].astype(bool)
        assert int(tiles.sum()) == skipped
        proj = (gaze + kw["proj_centre"][2:]) if gaze else kw["proj_centre"]
        want, b, _, _ = expected(A, pair[0], "rgba8", 8, "structured", shape, True, 0, proj, kw, "rgba8")
        want[skip] = 0xA5
        assert (b & skip).any(), "no band pixel in a skipped tile: the mesh does not test the bitmap"
        assert (b & ~skip).any() and np.array_equal(pair[1], want)
        assert (pair[1][skip] == 0xA5).all()
        images.append(pair[1])


def test_under_the_hdr_domain_the_pass_runs_in_the_mapped_domain(gpu):
    """OVRFSR_HDR_DOMAIN_SRTM against its manual composition: forward map on the host, the RGBA32F pipeline WITH the feather on a ctx without
    the setting, back map and the destination's store conversion on the host (tests/hdrmap.py)"""
    import openvr_fsr_amd as A
    from openvr_fsr_amd import _capi as K
    from tests.test_gpu_hdr_domain import content
    torch = gpu
    iw, ih, ow, oh = A_SHAPE
    x = content(iw, ih, 9)
    for dst_np, dt in ((np.float16, torch.float16), (np.uint8, torch.uint8)):
        pp, kw = _ctx(A, A_SHAPE)
        try:
            pp.set_hdr_domain(K.HDR_DOMAIN_SRTM)
            pp.set_mask_feather(WIDTH)
            got = _host(torch, pp.apply(0, torch.from_numpy(x.astype(np.float16)).cuda(), out_dtype=dt))
            assert pp.mask_feather_stats() == 1
        finally:
            pp.close()
        ref, _ = _ctx(A, A_SHAPE)
        try:
            ref.set_mask_feather(WIDTH)
            mid = _host(torch, ref.apply(0, torch.from_numpy(hdrmap.forward(x)).cuda(), out_dtype=torch.float32))
            ref.set_mask_feather(0.0)
            plain = _host(torch, ref.apply(0, torch.from_numpy(hdrmap.forward(x)).cuda(), out_dtype=torch.float32))
        finally:
            ref.close()
        assert (mid != plain).any()
        want = hdrmap.to_dest(hdrmap.back(mid), dst_np, O.float_to_unorm8)
        assert got.tobytes() == np.ascontiguousarray(want).tobytes(), dst_np.__name__


# ---- 4. what ignores the setting ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape,cfg", [("nvscaler", A_SHAPE, dict(use_nis=1)), ("nvsharpen", (128, 107, 128, 107), dict(use_nis=1)),
                                            ("rcas-only", (128, 107, 128, 107), {}), ("unmasked", A_SHAPE, dict(radius=2.0, proj_centre=(0.5, 0.5, 0.5, 0.5))),
                                            ("width-0", A_SHAPE, {})])
def test_no_launch_and_no_byte_moves(gpu, name, shape, cfg):
    import openvr_fsr_amd as A
    torch = gpu
    pp, _ = _ctx(A, shape, **cfg)
    try:
        before = _apply(torch, pp, "rgba8", 4, "structured", shape, True, 0, "rgba8")
        pp.set_mask_feather(0.0 if name == "width-0" else WIDTH)
        after = _apply(torch, pp, "rgba8", 4, "structured", shape, True, 0, "rgba8")
        assert pp.mask_feather_stats() == 0
    finally:
        pp.close()
    assert np.array_equal(before, after)


def test_setter_and_getter(gpu):
    import openvr_fsr_amd as A
    pp, _ = _ctx(A, A_SHAPE)
    try:
        assert pp.mask_feather() == 0.0 and pp.mask_feather_stats() == 0
        pp.set_mask_feather(0.25)
        for bad in (float("nan"), float("inf"), -float("inf"), -0.01, 2.001):
            with pytest.raises(A.OvrFsrError) as e:
                pp.set_mask_feather(bad)
            assert e.value.status == 1
        assert pp.mask_feather() == 0.25                       # the stored value stayed
        pp.reset()
        assert pp.mask_feather() == 0.25
        pp.set_config(A.Config.default(fsr_enabled=1, out_width=64, out_height=48, radius=0.4))
        assert pp.mask_feather() == 0.25
        pp.set_mask_feather(2.0)
        assert pp.mask_feather() == 2.0
        pp.set_mask_feather(0.0)
        assert pp.mask_feather() == 0.0
    finally:
        pp.close()


# ---- 5. checked build --------------------------------------------------------------------------------------------------------------------
_CHILD_BOUNDS = r"""
import ctypes, sys
sys.path.insert(0, %r)
import torch
import openvr_fsr_amd as A
from tests import test_gpu_mask_feather as T
lib = A.library()
n = lib.ovrfsr_debug_bounds_slots()
buf = (ctypes.c_ulonglong * n)()
lib.ovrfsr_debug_bounds.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.c_int]
assert lib.ovrfsr_debug_bounds(buf, n, 1) == 0
ran = launched = 0
bad = []
for si in range(len(T.SRCS)):
    r, l, b = T.matrix(torch, A, si, kinds=("B",))
    ran += r; launched += l; bad += b
torch.cuda.synchronize()
assert lib.ovrfsr_debug_bounds(buf, n, 0) == 0
nk = (n - 5) // 3
v = list(buf)
print("feather checked: launched %%d, mismatches %%d, checked %%d, out of bounds %%d" %% (launched, len(bad), sum(v[2 * nk:3 * nk]), sum(v[:nk])))
"""


def test_checked_build(gpu):
    """the matrix on its smallest shape against the -DOVRFSR_BOUNDS build, in a fresh child process: every image and table access of the pass
    through the checked accessors, 0 violations, and the same bytes"""
    from tests.variants import variant
    lib = variant("bounds", "-DOVRFSR_BOUNDS")
    env = dict(os.environ, OVRFSR_LIB=lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", _CHILD_BOUNDS % ROOT], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    m = re.search(r"feather checked: launched (\d+), mismatches (\d+), checked (\d+), out of bounds (\d+)", r.stdout)
    assert r.returncode == 0 and m, (r.stdout[-1500:], r.stderr[-1500:])
    print(m.group(0))
    assert int(m.group(1)) > 60 and int(m.group(2)) == 0 and int(m.group(3)) > 1e5 and int(m.group(4)) == 0, m.group(0)
