"""Multisampled input images (OVRFSR_FORMAT_MS) on the GPU: every output is, byte for byte, the output of the same call on the single-sample
image that tests/msaa.py's numpy resolve makes of the samples -- on every path, in both builds -- and the refusals / rebuilds the header
promises.  (A library without the feature refuses every multisampled descriptor with OVRFSR_ERR_UNSUPPORTED.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import msaa

pytestmark = pytest.mark.gpu
STRICT, FP32 = 2, 0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a shape whose interior EASU tiles take the quad staging sweep, and an odd one that is nearly all edge tiles (flat sweep)
SHAPES = ((96, 80, 128, 107), (37, 29, 50, 41))
CONTENTS = ("structured", "random", "natural")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _out_dtype(fmt):
    import torch
    return {"rgba8": torch.uint8, "bgra8": torch.uint8, "rgba16f": torch.float16, "rgba32f": torch.float32, "rgb10a2": torch.int32}[fmt]


def _in_format(fmt):
    from openvr_fsr_amd import _capi as K
    return K.FORMAT_BGRA8 if fmt == "bgra8" else None


def _apply(fmt, img, ow, oh, eye=0, **cfg):
    """one ovrfsr_apply on a fresh ctx -> numpy output"""
    import torch
    import openvr_fsr_amd as A
    kw = dict(fsr_enabled=1, out_width=ow, out_height=oh, radius=2.0, sharpness=0.9)
    kw.update(cfg)
    pp = A.PostProcessor(**kw)
    out = pp.apply(eye, _dev(img), out_dtype=_out_dtype(fmt), in_format=_in_format(fmt))
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    pp.close()
    return res


def _single(fmt, ms):
    """the numpy-resolved single-sample image and the format it is submitted in (a resolved BGRA8 image is RGBA8)"""
    return msaa.resolve(ms, fmt), ("rgba8" if fmt == "bgra8" else fmt)


def _twin(fmt, ms, ow, oh, **cfg):
    got = _apply(fmt, ms, ow, oh, **cfg)
    ss, sfmt = _single(fmt, ms)
    want = _apply(sfmt, ss, ow, oh, **cfg)
    return got, want


def matrix():
    """(1) of the issue: every base format x S x build x shape x content.  Returns the list of failing cases."""
    bad = []
    seed = 0
    for fmt in msaa.FORMATS:
        for s in msaa.SAMPLES:
            for prec in (FP32, STRICT):
                for (iw, ih, ow, oh) in SHAPES:
                    for content in CONTENTS:
                        seed += 1
                        ms = msaa.make_ms(iw, ih, s, fmt, content, seed)
                        got, want = _twin(fmt, ms, ow, oh, precision=prec)
                        if got.tobytes() != want.tobytes():
                            bad.append((fmt, s, prec, iw, ih, content))
    return bad


def test_output_bytes_equal_resolved_single_sample_apply(gpu):
    assert matrix() == []


def _ms(fmt="rgba8", s=4, w=96, h=80, content="structured", seed=7):
    return msaa.make_ms(w, h, s, fmt, content, seed)


@pytest.mark.parametrize("name,cfg,shape", [
    ("easu_only", dict(stage_mask=1), (96, 80, 128, 107)),
    ("rcas_only", dict(out_width=0, out_height=0, render_scale=1.0), (96, 80, 96, 80)),
    ("nvscaler", dict(use_nis=1), (96, 80, 128, 107)),
    ("nvsharpen", dict(use_nis=1, out_width=0, out_height=0, render_scale=1.0), (96, 80, 96, 80)),
    ("mask_sorted_r05", dict(radius=0.5, fused=-1), (192, 160, 256, 214)),
    ("nvscaler_r05", dict(use_nis=1, radius=0.5), (192, 160, 256, 214)),
    ("fused", dict(fused=1), (96, 80, 128, 107)),
    ("fused_masked", dict(fused=1, radius=0.5), (192, 160, 256, 214)),
    ("debug_tint", dict(debug_mode=1, radius=0.5), (96, 80, 128, 107)),
    ("strict_r05", dict(radius=0.5, precision=STRICT), (96, 80, 128, 107)),
])
def test_paths_equal_single_sample(gpu, name, cfg, shape):
    iw, ih, ow, oh = shape
    ms = _ms(w=iw, h=ih)
    kw = dict(cfg)
    if kw.get("out_width", 1) == 0:
        ow, oh = iw, ih
    got, want = _twin("rgba8", ms, ow, oh, **kw)
    assert got.tobytes() == want.tobytes(), name


def test_fused_half_input(gpu):
    ms = _ms(fmt="rgba16f")
    got, want = _twin("rgba16f", ms, 128, 107, fused=1)
    assert got.tobytes() == want.tobytes()


def _pp(**cfg):
    import openvr_fsr_amd as A
    kw = dict(fsr_enabled=1, out_width=128, out_height=107, radius=0.5, sharpness=0.9)
    kw.update(cfg)
    return A.PostProcessor(**kw)


def test_batch_of_alternating_eyes(gpu):
    import torch
    n = 6
    ms = np.stack([_ms(seed=30 + i) for i in range(n)])
    ss = np.stack([msaa.resolve_unorm8(m) for m in ms])
    outs = []
    for src in (ms, ss):
        pp = _pp()
        o = torch.zeros((n, 107, 128, 4), dtype=torch.uint8, device="cuda")
        pp.apply_batch(_dev(src), o)
        torch.cuda.synchronize()
        outs.append(o.cpu().numpy())
        pp.close()
    assert outs[0].tobytes() == outs[1].tobytes()
    # and each image equals its own single apply (eye i & 1)
    for i in range(n):
        assert outs[0][i].tobytes() == _apply("rgba8", ss[i], 128, 107, eye=i & 1, radius=0.5).tobytes(), i


def test_batch_shared(gpu):
    import torch
    n = 3
    ms = np.stack([_ms(w=192, h=80, seed=50 + i) for i in range(n)])
    ss = np.stack([msaa.resolve_unorm8(m) for m in ms])
    outs = []
    for src in (ms, ss):
        pp = _pp(out_width=256, out_height=107)
        o = torch.zeros((n, 107, 256, 4), dtype=torch.uint8, device="cuda")
        pp.apply_batch(_dev(src), o, shared=True)
        torch.cuda.synchronize()
        outs.append(o.cpu().numpy())
        pp.close()
    assert outs[0].tobytes() == outs[1].tobytes()


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_pair_submit(gpu, order):
    import torch
    frames = [(_ms(seed=70 + 2 * f), _ms(seed=71 + 2 * f)) for f in range(3)]
    res = []
    for single in (False, True):
        pp = _pp(pair_submit=1)
        got = []
        for f, (a, b) in enumerate(frames):
            imgs = {0: a, 1: b}
            outs = {}
            for eye in order:
                src = msaa.resolve_unorm8(imgs[eye]) if single else imgs[eye]
                o = torch.zeros((107, 128, 4), dtype=torch.uint8, device="cuda")
                t = _dev(src)
                pp.apply(eye, t, out=o)
                outs[eye] = (o, t)
            torch.cuda.synchronize()
            got.append([outs[e][0].cpu().numpy() for e in (0, 1)])
        pp.close()
        res.append(got)
    for f in range(len(frames)):
        for e in (0, 1):
            assert res[0][f][e].tobytes() == res[1][f][e].tobytes(), (f, e)


def test_ctx_owned_output(gpu):
    import torch
    ms = _ms()
    pp = _pp()
    got = pp.apply(0, _dev(ms))
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (107, 128, 4)
    g = got.cpu().numpy()
    pp.close()
    assert g.tobytes() == _apply("rgba8", msaa.resolve_unorm8(ms), 128, 107, radius=0.5).tobytes()
    # BGRA8 multisampled -> RGBA8 ctx-owned output
    from openvr_fsr_amd import _capi as K
    pp = _pp()
    got = pp.apply(0, _dev(ms), in_format=K.FORMAT_BGRA8)
    torch.cuda.synchronize()
    g = got.cpu().numpy()
    pp.close()
    assert g.tobytes() == _apply("rgba8", msaa.resolve_bgra8(ms), 128, 107, radius=0.5).tobytes()


def test_full_c2_size(gpu):
    from oracle import oracle as O
    iw, ih, ow, oh = 1683, 1869, 2244, 2492
    ms = msaa.make_ms(iw, ih, 4, "rgba8", "structured", 3)
    ss = msaa.resolve_unorm8(ms)
    strict = _apply("rgba8", ms, ow, oh, precision=STRICT)
    want = O.fsr_pipeline_u8(ss, ow, oh, sharpness=0.9, radius=2.0)
    assert strict.tobytes() == want.tobytes()
    prod = _apply("rgba8", ms, ow, oh)
    assert prod.tobytes() == _apply("rgba8", ss, ow, oh).tobytes()


# ---- refusals and rebuilds -------------------------------------------------------------------------------------------------


def _img(t, fmt, width=None, pitch=None):
    from openvr_fsr_amd import _capi as K
    return K.Image(t.data_ptr(), width if width is not None else t.shape[1], t.shape[0],
                   pitch if pitch is not None else t.stride(0) * t.element_size(), fmt)


def test_refusals_leave_the_ctx_enabled(gpu):
    import ctypes as C
    import torch
    from openvr_fsr_amd import _capi as K
    pp = _pp()
    lib = pp._lib
    ms = _dev(_ms())
    out = torch.zeros((107, 128, 4), dtype=torch.uint8, device="cuda")
    ok_out = _img(out, K.FORMAT_RGBA8)

    def call(img, o=None):
        o = o if o is not None else ok_out
        return lib.ovrfsr_apply(pp._ctx, 0, C.byref(img), None, C.byref(o), pp._stream())

    good = _img(ms.view(80, 96 * 4, 4), K.format_ms(K.FORMAT_RGBA8, 4), width=96)
    # a multisampled output
    out_ms = torch.zeros((107, 128, 4, 4), dtype=torch.uint8, device="cuda")
    assert call(good, _img(out_ms.view(107, 128 * 4, 4), K.format_ms(K.FORMAT_RGBA8, 4), width=128)) == 2
    # ... of any base format, BGRA8 (itself input-only) included, and whatever its pitch: the caller's likely mistake is a single-sample
    # pitch, and the refusal must be the header's OVRFSR_ERR_UNSUPPORTED in front of the size and pitch tests, not "bad pitch"
    for base in (K.FORMAT_BGRA8, K.FORMAT_RGBA8, K.FORMAT_R11G11B10F):
        for o in (_img(out, K.format_ms(base, 4)), _img(out_ms.view(107, 128 * 4, 4), K.format_ms(base, 4), width=128)):
            assert call(good, o) == 2, (base, o.pitch_bytes)
            want_text = b"out: R11G11B10F is an input-only format" if base == K.FORMAT_R11G11B10F else b"out: multisampled images are input-only"
            assert lib.ovrfsr_last_error(pp._ctx) == want_text, (base, lib.ovrfsr_last_error(pp._ctx))
    # sample counts 3 and 16, an unknown bit
    for bad_fmt in (K.format_ms(K.FORMAT_RGBA8, 3), K.format_ms(K.FORMAT_RGBA8, 16), K.FORMAT_RGBA8 | 1 << 20, K.format_ms(5, 4)):
        assert call(_img(ms.view(80, 96 * 4, 4), bad_fmt, width=96)) == 2, hex(bad_fmt)
    # a pitch that does not hold width x S texels; a misaligned base
    assert call(_img(ms.view(80, 96 * 4, 4), K.format_ms(K.FORMAT_RGBA8, 4), width=96, pitch=96 * 4 * 4 - 4)) == 1
    mis = K.Image(ms.data_ptr() + 2, 95, 80, 96 * 16, K.format_ms(K.FORMAT_RGBA8, 4))
    assert call(mis) == 1
    # still enabled: the good call works and matches
    assert call(good) == 0
    torch.cuda.synchronize()
    want = _apply("rgba8", msaa.resolve_unorm8(ms.cpu().numpy()), 128, 107, radius=0.5)
    assert out.cpu().numpy().tobytes() == want.tobytes()
    pp.close()


def test_save_refuses_multisampled(gpu, tmp_path):
    import ctypes as C
    from openvr_fsr_amd import _capi as K
    lib = K.library()
    ms = _dev(_ms())
    for fmt in (K.format_ms(K.FORMAT_RGBA8, 4), K.format_ms(K.FORMAT_RGBA8, 3), K.FORMAT_RGBA8 | 1 << 20):
        img = _img(ms.view(80, 96 * 4, 4), fmt, width=96)
        assert lib.ovrfsr_save_ppm(C.byref(img), str(tmp_path / "a.ppm").encode(), None) == 2, hex(fmt)
        assert lib.ovrfsr_save_dds(C.byref(img), str(tmp_path / "a.dds").encode(), None) == 2, hex(fmt)
    # samples = 1 is the single-sample image: saved exactly as the base format
    ss = _dev(msaa.resolve_unorm8(_ms()))
    for fmt, name in ((K.FORMAT_RGBA8, "b"), (K.format_ms(K.FORMAT_RGBA8, 1), "c")):
        img = _img(ss, fmt)
        assert lib.ovrfsr_save_ppm(C.byref(img), str(tmp_path / (name + ".ppm")).encode(), None) == 0
        assert lib.ovrfsr_save_dds(C.byref(img), str(tmp_path / (name + ".dds")).encode(), None) == 0
    assert (tmp_path / "b.ppm").read_bytes() == (tmp_path / "c.ppm").read_bytes()
    assert (tmp_path / "b.dds").read_bytes() == (tmp_path / "c.dds").read_bytes()


@pytest.mark.parametrize("fmt", ["rgba16f", "rgba32f"])
@pytest.mark.parametrize("stage_mask", [0, 1])
def test_float_sum_order_on_the_device(gpu, fmt, stage_mask):
    """The fp32 sample-order rule pinned on the device: texels [1024, 2^-14, 2^-14, -1024] resolve to 0 and their reverse to 2^-15
    (pairwise summation would give 2^-16 for both).  Laid out in blocks so that whole EASU footprints see one answer."""
    dt = np.float16 if fmt == "rgba16f" else np.float32
    e = 2.0 ** -14
    fwd, rev = np.array([1024, e, e, -1024], dt), np.array([-1024, e, e, 1024], dt)
    h, w = 80, 96
    ms = np.empty((h, w, 4, 4), dt)
    blk = ((np.arange(h)[:, None] // 8 + np.arange(w)[None, :] // 8) % 2).astype(bool)
    ms[blk] = np.repeat(fwd[:, None], 4, axis=1)
    ms[~blk] = np.repeat(rev[:, None], 4, axis=1)
    ms[..., 3] = 1.0  # alpha: plain ones
    ss = msaa.resolve_float(ms)
    assert set(np.unique(ss[..., :3]).tolist()) == {0.0, 2.0 ** -15}
    got, want = _twin(fmt, ms, 128, 107, stage_mask=stage_mask)
    assert got.tobytes() == want.tobytes()
    # and the outputs do tell the two answers apart (a resolve to 2^-16 everywhere would not give these bytes)
    flat = _apply(fmt, np.full_like(ss, 2.0 ** -16), 128, 107, stage_mask=stage_mask)
    assert got.tobytes() != flat.tobytes()


def test_sample_count_changes_rebuild(gpu):
    import torch
    pp = _pp()
    base = _ms(s=8, seed=90)
    for s in (4, 2, 1, 4):
        src = base[:, :, :s] if s > 1 else base[:, :, 0]
        out = torch.zeros((107, 128, 4), dtype=torch.uint8, device="cuda")
        pp.apply(0, _dev(src), out=out)
        torch.cuda.synchronize()
        ss = msaa.resolve_unorm8(src) if s > 1 else src
        assert out.cpu().numpy().tobytes() == _apply("rgba8", ss, 128, 107, radius=0.5).tobytes(), s
    pp.close()


def test_fsr_disabled_forwards_the_descriptor(gpu):
    import torch
    import openvr_fsr_amd as A
    pp = A.PostProcessor(fsr_enabled=0)
    t = _dev(_ms())
    got = pp.apply(0, t)
    assert got.data_ptr() == t.data_ptr()
    pp.close()


@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_capture(gpu):
    """A first multisampled call under capture must build (the resolve scratch, the pipeline): refused, capture intact, ctx enabled.  After
    one eager call a captured call replays to the same bytes."""
    import torch
    import openvr_fsr_amd as A
    ms = _dev(np.stack([_ms(seed=95), _ms(seed=96)]))
    pp = _pp()
    out = torch.zeros((2, 107, 128, 4), dtype=torch.uint8, device="cuda")
    ref = torch.zeros_like(out)
    side = torch.cuda.Stream()

    def capture():
        g = torch.cuda.CUDAGraph()
        side.wait_stream(torch.cuda.current_stream())
        err = None
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                try:
                    pp.apply_batch(ms, out)
                except A.OvrFsrError as e:
                    err = e
        torch.cuda.synchronize()
        return g, err

    g, err = capture()
    assert err is not None and err.status == 1, err
    pp.apply_batch(ms, ref)
    torch.cuda.synchronize()
    g, err = capture()
    assert err is None
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    pp.close()


# ---- checked builds ---------------------------------------------------------------------------------------------------------

_CHILD = r"""
import ctypes, sys
sys.path.insert(0, %r)
import openvr_fsr_amd as A
from tests import test_gpu_msaa as T
lib = A.library()
n = lib.ovrfsr_debug_bounds_slots()
buf = (ctypes.c_ulonglong * n)()
lib.ovrfsr_debug_bounds.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.c_int]
assert lib.ovrfsr_debug_bounds(buf, n, 1) == 0
bad = T.matrix()
import torch; torch.cuda.synchronize()
assert lib.ovrfsr_debug_bounds(buf, n, 0) == 0
nk = (n - 5) // 3
v = list(buf)
print("MSAA checked: mismatches %%d, checked %%d, out of bounds %%d" %% (len(bad), sum(v[2 * nk:3 * nk]), sum(v[:nk])))
"""

_AUDIT = r"""
import ctypes, sys
sys.path.insert(0, %r)
import numpy as np
import openvr_fsr_amd as A
from tests import msaa
from tests import test_gpu_msaa as T
lib = A.library()
c = (ctypes.c_ulonglong * 6)()
assert lib.ovrfsr_debug_tie_audit(c, 1) == 0
ms = msaa.make_ms(1683, 1869, 4, "rgba8", "natural", 11)
T._apply("rgba8", ms, 2244, 2492)
assert lib.ovrfsr_debug_tie_audit(c, 0) == 0
print("MSAA audit: audited %%d, flips %%d" %% (c[0], c[2]))
"""


def test_checked_build_matrix(gpu):
    from tests.variants import variant
    lib = variant("bounds", "-DOVRFSR_BOUNDS")
    env = dict(os.environ, OVRFSR_LIB=lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    import re
    m = re.search(r"MSAA checked: mismatches (\d+), checked (\d+), out of bounds (\d+)", r.stdout)
    assert r.returncode == 0 and m, (r.stdout[-1500:], r.stderr[-1500:])
    assert int(m.group(1)) == 0 and int(m.group(2)) > 1e6 and int(m.group(3)) == 0, m.group(0)


def test_audit_build_msaa_c2(gpu):
    from tests.variants import variant
    lib = variant("audit", "-DOVRFSR_TIE_AUDIT")
    env = dict(os.environ, OVRFSR_LIB=lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", _AUDIT % ROOT], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    import re
    m = re.search(r"MSAA audit: audited (\d+), flips (\d+)", r.stdout)
    assert r.returncode == 0 and m, (r.stdout[-1500:], r.stderr[-1500:])
    assert int(m.group(1)) > 1e6 and int(m.group(2)) == 0, m.group(0)
