"""Eye-tracked foveation on the GPU (include/openvr_fsr_amd.h, "Eye-tracked foveation").  The pixel contract is one sentence -- with a gaze set
for eye e, every call behaves as the same call on a fresh ctx (the TWIN) whose cfg.proj_centre holds the gaze in eye e's slots -- so every
test compares bytes with a twin: one ctx per form walking a sequence of gazes (re-aims in place, a sub-tile move, a no-op, a rebuild, clear),
with ovrfsr_gaze_stats advancing as the planner probe (tests/debug/gaze_probe.cpp, `sequence`) predicts; eight unsynchronised frames behind a
device-side delay (more than the staging ring holds); re-aims that allocate nothing (the ctx-owned image stays put; fault injection in the
checked build); stream capture; and a ctx whose gaze was cleared."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from openvr_fsr_amd import _capi as K
from tests import hidden_ref as R
from tests import synth
from tests import test_gaze as TG
from tests import test_pipeline_plan as TP
from tests.test_gpu_hidden_area import PLAN_FORMAT, _launch, _outputs, _source

pytestmark = pytest.mark.gpu

ROOT = TG.ROOT
S1, S2, S3 = TG.SHAPES["S1"], TG.SHAPES["S2"], TG.SHAPES["S3"]
G, OUT = TG.NAMED, (2.0, 2.0)
BASE = dict(radius=0.5, proj_centre=(0.2, 0.3, 0.8, 0.7))
# id, source, call, configuration, extra ("mesh": the meshes of tests/hidden_ref.py on both ctxs; "srtm": OVRFSR_HDR_DOMAIN_SRTM)
FORMS = [
    ("mask-sorted", "rgba8", "apply", {}, None),
    ("easu-only", "rgba8", "apply", dict(stage_mask=1), None),
    ("fused", "rgba8", "apply", dict(fused=1), None),
    ("half-fused-outside", "rgba16f", "apply", {}, None),
    ("nis-masked", "rgba8", "apply", dict(use_nis=1), None),
    ("exact", "rgba8", "apply", dict(precision=3), None),
    ("strict", "rgba8", "apply", dict(precision=2), None),
    ("bgra8", "bgra8", "apply", {}, None),
    ("ms4", "ms4", "apply", {}, None),
    ("r11g11b10f", "r11", "apply", {}, None),
    ("half-srtm", "rgba16f", "apply", {}, "srtm"),
    ("hidden-area", "rgba8", "apply", {}, "mesh"),
    ("batch", "rgba8", "batch", {}, None),
    ("shared", "rgba8", "shared", {}, None),
    ("pair", "rgba8", "pair", dict(pair_submit=1), None),
]
CASES = [pytest.param(src, call, cfg, extra, shape, id="%s-%dx%d" % (name, shape[2], shape[3]))
         for name, src, call, cfg, extra in FORMS for shape in (S1, S2, S3)]

# the walk: (left, right) gazes, None = cleared
WALK = [(G[i], G[(i + 1) % 6]) for i in range(6)] + [     # 1. G in order, different gazes on the two eyes
    (G[0], OUT),                                          # 2. one eye at OUT
    (G[0], G[0]), ((0.51, 0.5), G[0]),                    # 3. a sub-tile move: the same lists, a new centre
    ((0.5101, 0.5), G[0]),                                # 4. the same centre: nothing to do
    (OUT, OUT),                                           # 5. both eyes at OUT: no mask, a rebuild
    (None, None),                                         # 6. clear
]


@pytest.fixture(scope="module")
def probe():
    run, tmp = TG.build_gaze_probe()
    yield run
    shutil.rmtree(tmp, ignore_errors=True)


def _make(A, cfg, extra, shape, **more):
    iw, ih, ow, oh = shape
    pp = A.PostProcessor(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, **dict(BASE, **dict(cfg, **more)))
    if extra == "mesh":
        for eye in (0, 1):
            pp.set_hidden_area(eye, R.MESH[eye])
    if extra == "srtm":
        pp.set_hdr_domain(K.HDR_DOMAIN_SRTM)
    return pp


def _f32(xy):
    """what ovrfsr_get_gaze hands back for these values: floats"""
    return tuple(float(np.float32(v)) for v in xy)


def _centres(step):
    """the twin's proj_centre for a step of the walk"""
    pc = list(BASE["proj_centre"])
    for eye in (0, 1):
        if step[eye] is not None:
            pc[2 * eye], pc[2 * eye + 1] = step[eye]
    return tuple(pc)


def _aim(pp, step):
    for eye in (0, 1):
        if step[eye] is None:
            pp.clear_gaze(eye)
        else:
            pp.set_gaze(eye, *step[eye])


def _predicted(probe, src, call, cfg, shape, walk):
    iw, ih, ow, oh = shape
    line = TP._line("walk", PLAN_FORMAT[src], iw, ih, call != "shared", -1, fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, **dict(BASE, **cfg))
    steps = []
    for left, right in walk:
        for g in (left, right):
            steps += ["0 0.0 0.0"] if g is None else ["1 %r %r" % (float(g[0]), float(g[1]))]
    (got,) = probe("sequence", [line + " %d " % len(walk) + " ".join(steps)])
    return got["steps"]


# ---- 1. twin equality ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,call,cfg,extra,shape", CASES)
def test_every_step_of_the_walk_equals_its_twin(gpu, probe, src, call, cfg, extra, shape):
    torch = gpu
    import openvr_fsr_amd as A
    iw, ih, ow, oh = shape
    want_steps = _predicted(probe, src, call, cfg, shape, WALK)
    # (the strict build tests the mask per group, without lists: no mask at all is one more re-aim to it, and so is the way back)
    to_no_mask = "reaim" if cfg.get("precision") == 2 else "rebuild"
    # (a shared texture's eye image is half as wide: at 160 columns 0.5 and 0.51 are the same pixel of it, and the sub-tile move is a no-op)
    eye_w = ow // 2 if call == "shared" else ow
    sub_tile = "reaim" if int(np.float32(eye_w) * np.float32(0.51)) != eye_w // 2 else "nothing"
    assert want_steps == ["first"] + ["reaim"] * 7 + [sub_tile, "nothing", to_no_mask, to_no_mask], want_steps
    n = {"apply": 2, "pair": 2, "batch": 4, "shared": 2}[call]
    built = [_source(torch, src, iw, ih, synth.seed_for(21, i)) for i in range(n)]
    texs, (in_format, dtype, bpp) = [b[0] for b in built], built[0][1:]
    pp = _make(A, cfg, extra, shape)
    try:
        stats = (0, 0)
        for i, step in enumerate(WALK):
            _aim(pp, step)
            outs, raw = _outputs(torch, n, oh, ow, dtype, bpp)
            _launch(torch, pp, call, texs, in_format, outs)
            twin = _make(A, cfg, extra, shape, proj_centre=_centres(step))
            try:
                touts, traw = _outputs(torch, n, oh, ow, dtype, bpp)
                _launch(torch, twin, call, texs, in_format, touts)
                assert [pp.hidden_area_stats(e) for e in (0, 1)] == [twin.hidden_area_stats(e) for e in (0, 1)], i
            finally:
                twin.close()
            got, want = raw.cpu().numpy(), traw.cpu().numpy()
            assert (want != 0xA5).any() and np.array_equal(got, want), "step %d (%s): the bytes differ from the twin's" % (i, want_steps[i])
            now = pp.gaze_stats()
            delta = (now[0] - stats[0], now[1] - stats[1])
            assert delta == {"reaim": (1, 0), "rebuild": (0, 1)}.get(want_steps[i], (0, 0)), (i, want_steps[i], delta)
            stats = now
        assert pp.gaze(0) == (_f32(BASE["proj_centre"][:2]), False)
    finally:
        pp.close()


def test_a_gaze_set_between_the_eyes_of_a_pair_keeps_the_recorded_eye(gpu):
    """unlike the other setters: the recorded eye stays, and the pair launches with the gazes in effect at its second call"""
    torch = gpu
    import openvr_fsr_amd as A
    iw, ih, ow, oh = S2
    texs = [_source(torch, "rgba8", iw, ih, synth.seed_for(22, i))[0] for i in range(2)]
    pp = _make(A, dict(pair_submit=1), None, S2)
    twin = _make(A, dict(pair_submit=1), None, S2, proj_centre=G[5] + G[2])
    try:
        pp.set_gaze(0, *G[1])
        pp.set_gaze(1, *G[2])
        outs, raw = _outputs(torch, 2, oh, ow, torch.uint8, 4)
        pp.apply(0, texs[0], out=outs[0])
        assert pp.pair_pending()
        pp.set_gaze(0, *G[5])
        assert pp.pair_pending()
        pp.apply(1, texs[1], out=outs[1])
        assert not pp.pair_pending()
        touts, traw = _outputs(torch, 2, oh, ow, torch.uint8, 4)
        _launch(torch, twin, "pair", texs, None, touts)
        torch.cuda.synchronize()
        assert np.array_equal(raw.cpu().numpy(), traw.cpu().numpy())
    finally:
        pp.close()
        twin.close()


def test_arguments(gpu):
    import openvr_fsr_amd as A
    pp = _make(A, {}, None, S1)
    try:
        pp.set_gaze(1, 0.25, 0.75)
        for bad in ((2, 0.5, 0.5), (0, float("nan"), 0.5), (0, 0.5, float("inf")), (1, 2.5, 0.5), (1, 0.5, -1.5)):
            with pytest.raises(A.OvrFsrError) as e:
                pp.set_gaze(*bad)
            assert e.value.status == 1
        assert pp.gaze(1) == ((0.25, 0.75), True) and pp.gaze(0) == (_f32(BASE["proj_centre"][:2]), False)   # the stored values stayed
        pp.reset()
        pp.set_config(pp.cfg)
        assert pp.gaze(1) == ((0.25, 0.75), True)                                                       # reset and set_config keep the gaze
        pp.clear_gaze(1)
        assert pp.gaze(1) == (_f32(BASE["proj_centre"][2:]), False) and pp.gaze_stats() == (0, 0)
    finally:
        pp.close()


# ---- 2. unsynchronised frames ----------------------------------------------------------------------------------------------------------------
def test_eight_frames_without_a_synchronise(gpu):
    """a device-side delay in front, then eight set_gaze + apply pairs into eight outputs and no synchronisation: twice what the staging ring
    holds.  A single staging buffer, or a slot reused without its event, uploads a later frame's lists under an earlier frame's launch."""
    torch = gpu
    import openvr_fsr_amd as A
    iw, ih, ow, oh = S3
    tex = _source(torch, "rgba8", iw, ih, synth.seed_for(23, 0))[0]
    gazes = G + [(0.3, 0.7), (0.7, 0.3)]
    pp = _make(A, {}, None, S3)
    try:
        pp.set_gaze(0, 0.9, 0.1)
        warm, _ = _outputs(torch, 1, oh, ow, torch.uint8, 4)
        pp.apply(0, tex, out=warm[0])                       # the build: everything after it is a re-aim
        torch.cuda.synchronize()
        outs, raw = _outputs(torch, len(gazes), oh, ow, torch.uint8, 4)
        torch.cuda._sleep(int(0.04 * 2.0e9))               # tens of ms of device time in front of everything below
        for i, g in enumerate(gazes):
            pp.set_gaze(0, *g)
            pp.apply(0, tex, out=outs[i])
        assert pp.gaze_stats() == (len(gazes), 0)
        torch.cuda.synchronize()
        got = raw.cpu().numpy()
    finally:
        pp.close()
    seen = set()
    for i, g in enumerate(gazes):
        twin = _make(A, {}, None, S3, proj_centre=tuple(g) + BASE["proj_centre"][2:])
        try:
            touts, traw = _outputs(torch, 1, oh, ow, torch.uint8, 4)
            twin.apply(0, tex, out=touts[0])
            torch.cuda.synchronize()
            want = traw.cpu().numpy()[0]
        finally:
            twin.close()
        assert np.array_equal(got[i], want), "frame %d" % i
        seen.add(want.tobytes())
    assert len(seen) == len(gazes)                          # (the frames differ: an upload gone astray cannot hide)


# ---- 3. in place means in place ----------------------------------------------------------------------------------------------------------------
def test_fifty_reaims_leave_the_ctx_owned_image_where_it_is(gpu):
    torch = gpu
    import openvr_fsr_amd as A
    iw, ih, ow, oh = S2
    tex = _source(torch, "rgba8", iw, ih, synth.seed_for(24, 0))[0]
    pp = _make(A, {}, None, S2)
    twin = _make(A, {}, None, S2, proj_centre=G[49 % 6] + BASE["proj_centre"][2:])
    try:
        pp.set_gaze(0, 0.9, 0.1)
        where = pp.apply(0, tex).data_ptr()
        for i in range(50):
            pp.set_gaze(0, *G[i % 6])
            out = pp.apply(0, tex)
            assert out.data_ptr() == where, i
        torch.cuda.synchronize()
        assert pp.gaze_stats() == (50, 0)
        assert torch.equal(out, twin.apply(0, tex))
    finally:
        pp.close()
        twin.close()


_CHILD = r"""
import ctypes, sys
sys.path.insert(0, %r)
import numpy as np
import torch
import openvr_fsr_amd as A
from tests import test_gpu_gaze as T
lib = A.library()
n = lib.ovrfsr_debug_bounds_slots()
buf = (ctypes.c_ulonglong * n)()
lib.ovrfsr_debug_bounds.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.c_int]
assert lib.ovrfsr_debug_bounds(buf, n, 1) == 0
iw, ih, ow, oh = T.S2
tex = T._source(torch, "rgba8", iw, ih, 7)[0]
pp = T._make(A, {}, None, T.S2)
pp.set_gaze(0, *T.G[1]); pp.set_gaze(1, *T.G[2])
pp.apply(0, tex)
pp.set_gaze(0, *T.G[5])
lib.ovrfsr_debug_fail_resource(1)            # the next creation fails: a re-aim creates nothing
got = pp.apply(0, tex).clone()
lib.ovrfsr_debug_fail_resource(0)
twin = T._make(A, {}, None, T.S2, proj_centre=T.G[5] + T.G[2])
same = bool(torch.equal(got, twin.apply(0, tex)))
torch.cuda.synchronize()
assert lib.ovrfsr_debug_bounds(buf, n, 0) == 0
nk = (n - 5) // 3
oob = sum(list(buf)[:nk])
pp.set_gaze(0, *T.OUT); pp.set_gaze(1, *T.OUT)
lib.ovrfsr_debug_fail_resource(1)            # the positive control: a rebuild does create
try:
    pp.apply(0, tex)
    status = 0
except A.OvrFsrError as e:
    status = e.status
lib.ovrfsr_debug_fail_resource(0)
print("gaze fault injection: reaims %%d rebuilds %%d, same %%d, out of bounds %%d, rebuild status %%d" %% (pp.gaze_stats() + (same, oob, status)))
"""


def test_a_reaim_creates_nothing_and_a_rebuild_does(gpu):
    """the checked build's fault injection: with the next creation armed to fail, a re-aiming apply succeeds (and equals its twin, with no
    out-of-bounds access of tile_records_kernel or anything else); the same arming in front of the both-eyes-OUT rebuild fails with
    OVRFSR_ERR_OUT_OF_MEMORY"""
    from tests.variants import variant
    lib = variant("bounds", "-DOVRFSR_BOUNDS")
    env = dict(os.environ, OVRFSR_LIB=lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    m = re.search(r"gaze fault injection: reaims (\d+) rebuilds (\d+), same (\d+), out of bounds (\d+), rebuild status (\d+)", r.stdout)
    assert r.returncode == 0 and m, (r.stdout[-1500:], r.stderr[-1500:])
    assert [int(x) for x in m.groups()] == [1, 0, 1, 0, 6], m.group(0)


# ---- 4. capture ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_capture(gpu):
    """an apply with a pending re-aim is refused under capture and the capture stays valid; after one plain call with that gaze the same call
    captures, and the replay equals the twin"""
    torch = gpu
    import openvr_fsr_amd as A
    iw, ih, ow, oh = S1
    tex = _source(torch, "rgba8", iw, ih, synth.seed_for(25, 0))[0]
    pp = _make(A, {}, None, S1)
    twin = _make(A, {}, None, S1, proj_centre=G[2] + BASE["proj_centre"][2:])
    out = torch.zeros((oh, ow, 4), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()

    def capture(before=None):
        g = torch.cuda.CUDAGraph()
        side.wait_stream(torch.cuda.current_stream())
        err = None
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):          # (leaving the block ends the capture: it must still be valid)
                try:
                    if before:
                        before()
                    pp.apply(0, tex, out=out)
                except A.OvrFsrError as e:
                    err = e
        torch.cuda.synchronize()
        return g, err

    try:
        pp.set_gaze(0, *G[1])
        pp.apply(0, tex, out=out)
        torch.cuda.synchronize()
        g, err = capture(lambda: pp.set_gaze(0, *G[2]))     # the setter is accepted, the re-aim it asks for is not
        assert err is not None and err.status == 1 and pp.gaze_stats() == (0, 0), err
        pp.apply(0, tex, out=out)                            # once outside the capture: the re-aim
        torch.cuda.synchronize()
        assert pp.gaze_stats() == (1, 0)
        g, err = capture()
        assert err is None
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        want = torch.zeros_like(out)
        twin.apply(0, tex, out=want)
        torch.cuda.synchronize()
        assert torch.equal(out, want) and bool((want != 0).any())
    finally:
        pp.close()
        twin.close()


# ---- 5. default untouched ----------------------------------------------------------------------------------------------------------------------
def test_set_then_cleared_equals_a_plain_ctx(gpu):
    torch = gpu
    import openvr_fsr_amd as A
    iw, ih, ow, oh = S2
    texs = [_source(torch, "rgba8", iw, ih, synth.seed_for(26, i))[0] for i in range(2)]
    pp, plain = _make(A, {}, None, S2), _make(A, {}, None, S2)
    try:
        pp.set_gaze(0, *G[0])
        pp.clear_gaze(0)
        outs, raw = _outputs(torch, 2, oh, ow, torch.uint8, 4)
        _launch(torch, pp, "apply", texs, None, outs)
        pouts, praw = _outputs(torch, 2, oh, ow, torch.uint8, 4)
        _launch(torch, plain, "apply", texs, None, pouts)
        assert np.array_equal(raw.cpu().numpy(), praw.cpu().numpy()) and pp.gaze_stats() == (0, 0)
    finally:
        pp.close()
        plain.close()
