"""Dynamic resolution on the GPU (include/openvr_fsr_amd.h, "dynamic resolution").  The contract is one sentence -- with a maximum input size
set, every call behaves as the same call on a fresh ctx (the TWIN: same cfg, meshes, gazes, HDR domain and maximum) that never saw another
input size -- so every test compares bytes with a twin: one ctx per form walking a ladder of input sizes (tests/test_dynamic_resolution.py
shows on the CPU that every step of these ladders is a re-scale in place), ovrfsr_rescale_stats counting the steps and the ctx-owned output
staying where it is; the strict build against the oracle; batches, shared textures and pair_submit across a size change; a refusal; the two
routes that refill the tap tables; re-scales that create nothing (fault injection in the checked build); unsynchronised frames; capture; and a
ctx without a maximum, which rebuilds as it always has."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from openvr_fsr_amd import _capi as K
from tests import hidden_ref as R
from tests import synth
from tests.test_gpu_hidden_area import _outputs, _source

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK, UNMASKED = dict(radius=0.5, proj_centre=(0.2, 0.3, 0.8, 0.7)), dict(radius=2.0)
# shape: output, maximum input size, the ladder of input sizes (the first builds the ctx)
SHAPE_A = ((160, 128), (160, 120), [(80, 64), (120, 96), (107, 86), (152, 120), (64, 52), (100, 64), (160, 100), (80, 64)])
SHAPE_A_NIS = (SHAPE_A[0], SHAPE_A[1], [s for s in SHAPE_A[2] if s != (64, 52)])   # NVScaler scales 1x..2x only
SHAPE_B = ((200, 147), (150, 110), [(150, 110), (100, 74), (134, 98)])
# W: the 200 x 160 input's footprint is wider than 40 cells -- an R11G11B10F submission is decoded in staging, then unpacked by the pass, then
# decoded in staging again (unmasked: the masked half pipeline changes its form there, which is a rebuild)
SHAPE_W = ((160, 128), (208, 168), [(80, 64), (200, 160), (80, 64)])
G = [(0.5, 0.5), (0.2, 0.3), (0.8, 0.7), (0.0, 0.0), (1.0, 1.0), (0.37, 0.61)]

# id, source, configuration, shape, extra ("mesh+gaze": hidden-area meshes, and a gaze that moves in the same apply as the size; "srtm"),
# destination (torch dtype name, bytes per pixel; None: the source's own)
WALKS = [
    ("two-pass-unmasked", "rgba8", UNMASKED, SHAPE_A, None, None),
    ("mask-sorted-A", "rgba8", MASK, SHAPE_A, None, None),
    ("mask-sorted-B", "rgba8", MASK, SHAPE_B, None, None),
    ("half-fused-outside", "rgba16f", MASK, SHAPE_A, None, None),
    ("easu-only-into-float", "rgba8", dict(MASK, stage_mask=1), SHAPE_B, None, ("float32", 16)),
    ("nis-masked", "rgba8", dict(MASK, use_nis=1), SHAPE_A_NIS, None, None),
    ("rgb10a2", "rgb10a2", UNMASKED, SHAPE_A, None, None),
    ("bgra8", "bgra8", MASK, SHAPE_A, None, None),
    ("ms4", "ms4", MASK, SHAPE_A, None, None),
    ("r11g11b10f-flip", "r11", UNMASKED, SHAPE_W, None, None),
    ("half-srtm", "rgba16f", MASK, SHAPE_A, "srtm", None),
    ("exact", "rgba8", dict(MASK, precision=3), SHAPE_A, None, None),
    ("hidden-area-and-gaze", "rgba8", MASK, SHAPE_A, "mesh+gaze", None),
]


def _make(A, out, maximum, cfg, extra=None, gaze=None):
    pp = A.PostProcessor(fsr_enabled=1, out_width=out[0], out_height=out[1], sharpness=0.9, **cfg)
    if extra == "mesh+gaze":
        for eye in (0, 1):
            pp.set_hidden_area(eye, R.MESH[eye])
    if extra == "srtm":
        pp.set_hdr_domain(K.HDR_DOMAIN_SRTM)
    if gaze is not None:
        pp.set_gaze(0, *gaze)
    if maximum is not None:
        pp.set_max_input_size(*maximum)
    return pp


_SOURCES = {}


def _tex(torch, src, size, i):
    """-> (device tensor, in_format, output dtype, output bytes per pixel); made once per (source, size, image)"""
    key = (src, size, i)
    if key not in _SOURCES:
        iw, ih = size
        if src == "rgb10a2":
            words = np.random.default_rng(synth.seed_for(31, i) + iw * 131 + ih).integers(0, 2 ** 32, (ih, iw), dtype=np.uint64).astype(np.uint32)
            _SOURCES[key] = (torch.from_numpy(words.view(np.int32)).cuda(), None, torch.int32, 4)
        else:
            _SOURCES[key] = _source(torch, src, iw, ih, synth.seed_for(31, i) + iw * 131 + ih)
    return _SOURCES[key]


def _dest(torch, n, out, dtype, bpp):
    ow, oh = out
    if dtype == torch.int32:   # packed R10G10B10A2: [n, oh, ow] dwords
        raw = torch.full((n, oh, ow * 4), 0xA5, dtype=torch.uint8, device="cuda")
        return raw.view(torch.int32).reshape(n, oh, ow), raw
    return _outputs(torch, n, oh, ow, dtype, bpp)


def _frame(torch, pp, src, size, out, dest, owned=True):
    """both eyes of one frame at `size` into fresh destinations, then the left eye once more into the ctx-owned image
    -> (bytes written, the ctx-owned result or None)"""
    texs = [_tex(torch, src, size, i) for i in (0, 1)]
    in_format, dtype, bpp = texs[0][1:]
    if dest is not None:
        dtype, bpp = getattr(torch, dest[0]), dest[1]
    outs, raw = _dest(torch, 2, out, dtype, bpp)
    for eye in (0, 1):
        pp.apply(eye, texs[eye][0], out=outs[eye], in_format=in_format)
    mine = pp.apply(0, texs[0][0], in_format=in_format) if owned else None
    torch.cuda.synchronize()
    return raw.cpu().numpy(), mine


# ---- 1. every step of a walk equals its twin -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,cfg,shape,extra,dest", [pytest.param(*w[1:], id=w[0]) for w in WALKS])
def test_every_step_of_the_walk_equals_its_twin(gpu, src, cfg, shape, extra, dest):
    torch = gpu
    import openvr_fsr_amd as A
    out, maximum, sizes = shape
    owned = src != "rgb10a2"   # (the Python wrapper hands back no packed 10-bit tensor)
    pp = _make(A, out, maximum, cfg, extra, G[0] if extra == "mesh+gaze" else None)
    try:
        where, steps = None, 0
        for i, size in enumerate(sizes):
            gaze = G[i % 6] if extra == "mesh+gaze" else None
            if gaze is not None:
                pp.set_gaze(0, *gaze)   # (moves in the same apply as the size)
            got, mine = _frame(torch, pp, src, size, out, dest, owned)
            twin = _make(A, out, maximum, cfg, extra, gaze)
            try:
                want, theirs = _frame(torch, twin, src, size, out, dest, owned)
                assert [pp.hidden_area_stats(e) for e in (0, 1)] == [twin.hidden_area_stats(e) for e in (0, 1)], i
                assert (want != 0xA5).any() and np.array_equal(got, want), "step %d %s: the bytes differ from the twin's" % (i, size)
                if owned:
                    assert mine.shape == theirs.shape and mine.dtype == theirs.dtype and mine.stride() == theirs.stride(), i
                    assert torch.equal(mine.view(torch.uint8), theirs.view(torch.uint8)), "step %d %s: the ctx-owned image" % (i, size)
                    assert where in (None, mine.data_ptr()), "step %d: the ctx-owned output moved" % i
                    where = mine.data_ptr()
            finally:
                twin.close()
            steps += 1 if i and size != sizes[i - 1] else 0
            assert pp.rescale_stats() == (steps, 0), (i, size, pp.rescale_stats())
        assert steps == len(sizes) - 1 and pp.max_input_size() == maximum
    finally:
        pp.close()


def test_the_strict_build_walks_to_the_oracles_bytes(gpu):
    """O.easu then O.rcas with O.easu_con of each size (oracle.fsr_pipeline_u8 chains them as ApplyPostProcess does), bit for bit: the walk
    against the reference's arithmetic, not only against the library"""
    torch = gpu
    import openvr_fsr_amd as A
    from oracle import oracle as O
    out, maximum, sizes = SHAPE_A
    pp = _make(A, out, maximum, dict(MASK, precision=2))
    try:
        for n, size in enumerate([sizes[0], sizes[2], sizes[5]]):   # 2x, (107, 86), anisotropic
            got, _ = _frame(torch, pp, "rgba8", size, out, None, owned=False)
            for eye in (0, 1):
                img8 = _tex(torch, "rgba8", size, eye)[0].cpu().numpy()
                want = O.fsr_pipeline_u8(img8, out[0], out[1], sharpness=0.9, radius=MASK["radius"], proj=MASK["proj_centre"], eye=eye)
                assert np.array_equal(got[eye].reshape(out[1], out[0], 4), want), (size, eye)
            assert pp.rescale_stats() == (n, 0)
    finally:
        pp.close()


# ---- 2. call shapes --------------------------------------------------------------------------------------------------------------------
def _batch(torch, pp, texs, out, shared):
    outs, raw = _outputs(torch, len(texs), out[1], out[0], torch.uint8, 4)
    pp.apply_batch(torch.stack(texs), outs, first_eye=0, alternate_eyes=True, shared=shared)
    torch.cuda.synchronize()
    return raw.cpu().numpy()


@pytest.mark.parametrize("shared", [False, True], ids=["batch-of-4", "shared-pair"])
def test_batches_across_a_size_change(gpu, shared):
    torch = gpu
    import openvr_fsr_amd as A
    out = (320, 128) if shared else (160, 128)
    sizes = [(160, 64), (240, 96)] if shared else [(80, 64), (120, 96)]
    maximum, n = sizes[1], 2 if shared else 4
    pp = _make(A, out, maximum, MASK)
    try:
        for i, size in enumerate(sizes):
            texs = [_tex(torch, "rgba8", size, k)[0] for k in range(n)]
            got = _batch(torch, pp, texs, out, shared)
            twin = _make(A, out, maximum, MASK)
            try:
                want = _batch(torch, twin, texs, out, shared)
            finally:
                twin.close()
            assert (want != 0xA5).any() and np.array_equal(got, want), size
            assert pp.rescale_stats() == (i, 0)
    finally:
        pp.close()


def _pair(torch, pp, texs, out):
    outs, raw = _outputs(torch, 2, out[1], out[0], torch.uint8, 4)
    pp.apply(0, texs[0], out=outs[0])
    assert pp.pair_pending()
    pp.apply(1, texs[1], out=outs[1])
    assert not pp.pair_pending()
    torch.cuda.synchronize()
    return raw.cpu().numpy()


def test_pair_submit_across_a_size_change_and_between_the_eyes(gpu):
    """between frames: each frame's pair equals a fresh ctx's pair.  Between the eyes of a frame: the recorded eye is launched first, on its
    own and at its own size -- what single applies on fresh ctxs write"""
    torch = gpu
    import openvr_fsr_amd as A
    out, maximum, sizes = SHAPE_A
    cfg = dict(MASK, pair_submit=1)
    pp = _make(A, out, maximum, cfg)
    try:
        for i, size in enumerate(sizes[:2]):
            texs = [_tex(torch, "rgba8", size, k)[0] for k in (0, 1)]
            got = _pair(torch, pp, texs, out)
            twin = _make(A, out, maximum, cfg)
            try:
                want = _pair(torch, twin, texs, out)
            finally:
                twin.close()
            assert (want != 0xA5).any() and np.array_equal(got, want), size
            assert pp.rescale_stats() == (i, 0)
        # a frame whose eyes differ in size: left at sizes[2] is recorded, right at sizes[3] flushes it and is recorded itself
        left, right = _tex(torch, "rgba8", sizes[2], 0)[0], _tex(torch, "rgba8", sizes[3], 1)[0]
        outs, raw = _outputs(torch, 2, out[1], out[0], torch.uint8, 4)
        pp.apply(0, left, out=outs[0])
        assert pp.pair_pending() and pp.rescale_stats() == (2, 0)
        pp.apply(1, right, out=outs[1])
        assert pp.rescale_stats() == (3, 0)
        if pp.pair_pending():   # (recorded in its turn: the other eye follows, and the pair launches)
            pp.apply(0, _tex(torch, "rgba8", sizes[3], 0)[0], out=torch.empty_like(outs[0]))
        torch.cuda.synchronize()
        got = raw.cpu().numpy()
        for eye, tex, size in ((0, left, sizes[2]), (1, right, sizes[3])):
            twin = _make(A, out, maximum, MASK)
            try:
                touts, traw = _outputs(torch, 1, out[1], out[0], torch.uint8, 4)
                twin.apply(eye, tex, out=touts[0])
                torch.cuda.synchronize()
                assert np.array_equal(got[eye], traw.cpu().numpy()[0]), (eye, size)
            finally:
                twin.close()
    finally:
        pp.close()


# ---- 3. refusal, arguments -------------------------------------------------------------------------------------------------------------
def test_a_refused_size_fails_as_on_a_fresh_ctx_and_reset_recovers(gpu):
    torch = gpu
    import openvr_fsr_amd as A
    out, maximum, sizes = SHAPE_A
    cfg = dict(MASK, use_nis=1)
    pp, twin = _make(A, out, maximum, cfg), _make(A, out, maximum, cfg)
    try:
        _frame(torch, pp, "rgba8", sizes[0], out, None)
        _frame(torch, pp, "rgba8", sizes[1], out, None)
        assert pp.rescale_stats() == (1, 0)
        small = _tex(torch, "rgba8", (64, 52), 0)[0]
        errors = []
        for ctx in (pp, twin):
            with pytest.raises(A.OvrFsrError) as e:
                ctx.apply(0, small)
            errors.append((e.value.status, str(e.value)))
        assert errors[0] == errors[1] and errors[0][0] == 2, errors
        with pytest.raises(A.OvrFsrError) as e:
            pp.apply(0, _tex(torch, "rgba8", sizes[0], 0)[0])
        assert e.value.status == 5                      # disabled until reset
        pp.reset()
        got, _ = _frame(torch, pp, "rgba8", sizes[0], out, None)
        again, _ = _frame(torch, pp, "rgba8", sizes[2], out, None)
        assert pp.rescale_stats() == (2, 0) and pp.max_input_size() == maximum
        fresh = _make(A, out, maximum, cfg)
        try:
            want, _ = _frame(torch, fresh, "rgba8", sizes[2], out, None)
        finally:
            fresh.close()
        assert np.array_equal(again, want)
    finally:
        pp.close()
        twin.close()


def test_arguments_and_what_outlives_a_reset(gpu):
    import openvr_fsr_amd as A
    pp = _make(A, (160, 128), (160, 120), MASK)
    try:
        for bad in ((0, 5), (5, 0), (16385, 10), (10, 16385)):
            with pytest.raises(A.OvrFsrError) as e:
                pp.set_max_input_size(*bad)
            assert e.value.status == 1
        assert pp.max_input_size() == (160, 120)        # the stored value stayed
        pp.reset()
        pp.set_config(pp.cfg)
        assert pp.max_input_size() == (160, 120) and pp.rescale_stats() == (0, 0)
        pp.set_max_input_size(16384, 1)
        assert pp.max_input_size() == (16384, 1)
        pp.set_max_input_size(0, 0)
        assert pp.max_input_size() == (0, 0)
    finally:
        pp.close()


def test_above_the_maximum_and_an_output_that_follows_are_rebuilds(gpu):
    torch = gpu
    import openvr_fsr_amd as A
    out, maximum, sizes = SHAPE_B
    pp = _make(A, out, (120, 100), MASK)
    scaled = A.PostProcessor(fsr_enabled=1, render_scale=0.75, sharpness=0.9, **MASK)   # out_width = 0: the output follows the input
    try:
        scaled.set_max_input_size(160, 120)
        _frame(torch, pp, "rgba8", sizes[1], out, None)
        got, _ = _frame(torch, pp, "rgba8", sizes[2], out, None)      # (134, 98): wider than the maximum
        assert pp.rescale_stats() == (0, 1)
        twin = _make(A, out, (120, 100), MASK)
        try:
            want, _ = _frame(torch, twin, "rgba8", sizes[2], out, None)
        finally:
            twin.close()
        assert np.array_equal(got, want)
        for i, size in enumerate([(80, 64), (120, 96)]):
            scaled.apply(0, _tex(torch, "rgba8", size, 0)[0])
            assert scaled.rescale_stats() == (0, i)
        torch.cuda.synchronize()
    finally:
        pp.close()
        scaled.close()


# ---- 4. the checked build: both tap routes, creations, bounds --------------------------------------------------------------------------
_CHILD = r"""
import ctypes, sys
sys.path.insert(0, %r)
import numpy as np
import torch
import openvr_fsr_amd as A
from tests import test_gpu_dynamic_resolution as T
lib = A.library()
n = lib.ovrfsr_debug_bounds_slots()
buf = (ctypes.c_ulonglong * n)()
lib.ovrfsr_debug_bounds.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.c_int]
lib.ovrfsr_debug_read_taps.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
assert lib.ovrfsr_debug_bounds(buf, n, 1) == 0
out, maximum, sizes = T.SHAPE_A

def taps_of(pp):
    t = np.zeros(((out[0] + 31) // 32 * 32 + out[1] + 64, 2), np.uint32)
    assert lib.ovrfsr_debug_read_taps(pp._ctx, t.ctypes.data, t.nbytes) == 0
    return t

# (a) the two routes leave the same table, which is the host header's (what a fresh ctx uploads at build time)
same_taps = 1
for size in (sizes[1], sizes[2], sizes[6]):
    tables = []
    for upload in (0, 1):
        lib.ovrfsr_debug_tap_route(upload)
        pp = T._make(A, out, maximum, T.MASK)
        pp.apply(0, T._tex(torch, "rgba8", sizes[0], 0)[0])
        pp.apply(0, T._tex(torch, "rgba8", size, 0)[0])
        assert pp.rescale_stats() == (1, 0)
        tables.append(taps_of(pp))
        pp.close()
    fresh = T._make(A, out, maximum, T.MASK)
    fresh.apply(0, T._tex(torch, "rgba8", size, 0)[0])
    tables.append(taps_of(fresh))
    fresh.close()
    same_taps &= int(np.array_equal(tables[0], tables[1]) and np.array_equal(tables[0], tables[2]) and bool(tables[2].any()))
lib.ovrfsr_debug_tap_route(0)

# (b) the walk, a batch and a pair against the checked accessors, by both routes; twenty re-scales with a creation armed to fail
same = 1
for upload, src, cfg in ((0, "rgba8", T.MASK), (1, "rgba8", T.MASK), (0, "rgba16f", T.MASK), (0, "rgba8", T.UNMASKED), (0, "r11", T.UNMASKED)):
    lib.ovrfsr_debug_tap_route(upload)
    o, mx, ladder = T.SHAPE_W if src == "r11" else T.SHAPE_A
    pp = T._make(A, o, mx, cfg)
    T._frame(torch, pp, src, ladder[0], o, None)
    lib.ovrfsr_debug_fail_resource(1)            # the next creation fails: a re-scale creates nothing
    for k in range(20 if src == "rgba8" and not upload and cfg is T.MASK else len(ladder) - 1):
        size = ladder[1 + k %% (len(ladder) - 1)]
        got, _ = T._frame(torch, pp, src, size, o, None)
    lib.ovrfsr_debug_fail_resource(0)
    twin = T._make(A, o, mx, cfg)
    want, _ = T._frame(torch, twin, src, size, o, None)
    twin.close()
    same &= int(np.array_equal(got, want))
    rebuilds = pp.rescale_stats()[1]
    same &= int(rebuilds == 0)
    pp.close()
lib.ovrfsr_debug_tap_route(0)
for shared in (False, True):
    o = (320, 128) if shared else (160, 128)
    ladder = [(160, 64), (240, 96)] if shared else [(80, 64), (120, 96)]
    pp = T._make(A, o, ladder[1], T.MASK)
    for size in ladder:
        T._batch(torch, pp, [T._tex(torch, "rgba8", size, k)[0] for k in range(2 if shared else 4)], o, shared)
    same &= int(pp.rescale_stats() == (1, 0))
    pp.close()
pp = T._make(A, out, maximum, dict(T.MASK, pair_submit=1))
for size in sizes[:3]:
    T._pair(torch, pp, [T._tex(torch, "rgba8", size, k)[0] for k in (0, 1)], out)
same &= int(pp.rescale_stats() == (2, 0))
pp.close()
torch.cuda.synchronize()
assert lib.ovrfsr_debug_bounds(buf, n, 0) == 0
nk = (n - 5) // 3
oob = sum(list(buf)[:nk])

# (c) the positive control: a size above the maximum rebuilds, and a rebuild does create
pp = T._make(A, out, maximum, T.MASK)
pp.apply(0, T._tex(torch, "rgba8", sizes[0], 0)[0])
lib.ovrfsr_debug_fail_resource(1)
try:
    pp.apply(0, T._tex(torch, "rgba8", (200, 160), 0)[0])
    status = 0
except A.OvrFsrError as e:
    status = e.status
lib.ovrfsr_debug_fail_resource(0)
pp.close()

# (d) no maximum means what it always did: a size change is a rebuild, which creates
pp = T._make(A, out, None, T.MASK)
pp.apply(0, T._tex(torch, "rgba8", sizes[0], 0)[0])
lib.ovrfsr_debug_fail_resource(1)
try:
    pp.apply(0, T._tex(torch, "rgba8", sizes[1], 0)[0])
    plain_status = 0
except A.OvrFsrError as e:
    plain_status = e.status
lib.ovrfsr_debug_fail_resource(0)
print("dynamic resolution, checked build: same taps %%d, same bytes %%d, out of bounds %%d, rebuild status %%d, without a maximum %%d" %% (same_taps, same, oob, status, plain_status))
"""


def test_the_checked_build_tap_routes_creations_and_bounds(gpu):
    """-DOVRFSR_BOUNDS: (a) bilinDev_ read back after a re-scale by tap_tables_kernel and after one by upload -- byte-equal, and equal to the
    table the host header builds for a fresh ctx; (b) walks (twenty re-scales with the next creation armed to fail: none of it is consumed),
    batches and pairs with 0 out-of-bounds accesses, the shrunk and grown footprints against the real image extents included; (c) a size
    above the maximum with the same arming fails: a rebuild does create; (d) and so does every size change of a ctx without a maximum"""
    from tests.variants import variant
    lib = variant("bounds", "-DOVRFSR_BOUNDS")
    env = dict(os.environ, OVRFSR_LIB=lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    m = re.search(r"checked build: same taps (\d+), same bytes (\d+), out of bounds (\d+), rebuild status (\d+), without a maximum (\d+)", r.stdout)
    assert r.returncode == 0 and m, (r.stdout[-1500:], r.stderr[-1500:])
    assert [int(x) for x in m.groups()][:3] == [1, 1, 0] and int(m.group(4)) != 0 and int(m.group(5)) != 0, m.group(0)


# ---- 5. unsynchronised frames, capture -------------------------------------------------------------------------------------------------
def test_eight_frames_without_a_synchronise(gpu):
    """a device-side delay in front, then eight applies, each at the next size of the ladder, into eight outputs and no synchronisation: more
    frames than the staging ring has slots.  Tables refilled out of stream order would put a later frame's taps under an earlier launch."""
    torch = gpu
    import openvr_fsr_amd as A
    out, maximum, sizes = SHAPE_A
    ladder = sizes[1:] + sizes[1:2]
    texs = [_tex(torch, "rgba8", s, 0)[0] for s in ladder]
    pp = _make(A, out, maximum, MASK)
    try:
        warm, _ = _outputs(torch, 1, out[1], out[0], torch.uint8, 4)
        pp.apply(0, _tex(torch, "rgba8", sizes[0], 0)[0], out=warm[0])
        torch.cuda.synchronize()
        outs, raw = _outputs(torch, len(ladder), out[1], out[0], torch.uint8, 4)
        torch.cuda._sleep(int(0.04 * 2.0e9))
        for i, tex in enumerate(texs):
            pp.apply(0, tex, out=outs[i])
        assert pp.rescale_stats() == (len(ladder), 0)
        torch.cuda.synchronize()
        got = raw.cpu().numpy()
    finally:
        pp.close()
    for i, (size, tex) in enumerate(zip(ladder, texs)):
        twin = _make(A, out, maximum, MASK)
        try:
            touts, traw = _outputs(torch, 1, out[1], out[0], torch.uint8, 4)
            twin.apply(0, tex, out=touts[0])
            torch.cuda.synchronize()
            assert np.array_equal(got[i], traw.cpu().numpy()[0]), "frame %d %s" % (i, size)
        finally:
            twin.close()


@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_capture(gpu):
    """an apply that would re-scale is refused under capture and the capture stays valid; after the same call outside the capture a capture at
    that size replays to the twin's bytes"""
    torch = gpu
    import openvr_fsr_amd as A
    out, maximum, sizes = SHAPE_A
    first, second = _tex(torch, "rgba8", sizes[0], 0)[0], _tex(torch, "rgba8", sizes[1], 0)[0]
    pp, twin = _make(A, out, maximum, MASK), _make(A, out, maximum, MASK)
    dst = torch.zeros((out[1], out[0], 4), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()

    def capture():
        g = torch.cuda.CUDAGraph()
        side.wait_stream(torch.cuda.current_stream())
        err = None
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):          # (leaving the block ends the capture: it must still be valid)
                try:
                    pp.apply(0, second, out=dst)
                except A.OvrFsrError as e:
                    err = e
        torch.cuda.synchronize()
        return g, err

    try:
        pp.apply(0, first, out=dst)
        torch.cuda.synchronize()
        g, err = capture()
        assert err is not None and err.status == 1 and pp.rescale_stats() == (0, 0), err
        pp.apply(0, second, out=dst)                         # once outside the capture: the re-scale
        torch.cuda.synchronize()
        assert pp.rescale_stats() == (1, 0)
        g, err = capture()
        assert err is None
        dst.zero_()
        g.replay()
        torch.cuda.synchronize()
        want = torch.zeros_like(dst)
        twin.apply(0, second, out=want)
        torch.cuda.synchronize()
        assert torch.equal(dst, want) and bool((want != 0).any())
    finally:
        pp.close()
        twin.close()


# ---- 6. no maximum means what it always did --------------------------------------------------------------------------------------------
def test_without_a_maximum_every_size_change_rebuilds(gpu):
    """the same ladder on a ctx without a maximum: the same bytes and no re-scale counted -- every size change is the reset and rebuild it
    always was (that it creates resources is shown by fault injection: test_the_checked_build_tap_routes_creations_and_bounds, (d))"""
    torch = gpu
    import openvr_fsr_amd as A
    out, maximum, sizes = SHAPE_A
    plain, pp = _make(A, out, None, MASK), _make(A, out, maximum, MASK)
    try:
        for size in sizes[:4]:
            got, mine = _frame(torch, plain, "rgba8", size, out, None)
            want, theirs = _frame(torch, pp, "rgba8", size, out, None)
            assert np.array_equal(got, want) and torch.equal(mine, theirs), size
        assert plain.rescale_stats() == (0, 0) and plain.max_input_size() == (0, 0) and pp.rescale_stats() == (3, 0)
    finally:
        plain.close()
        pp.close()
