"""OVRFSR_PRECISION_FP32_EXACT on the GPU: the product build's kernels everywhere, and every UNORM8 byte an RGBA8-intermediate FSR pipeline
stores equal to the strict build's (precision 2), which equals the oracle.  The exactness is RCAS's near-tie guard (rcas_exact_bytes,
fsr_kernels.inc); the tie-rich fixture of tests/rcas_ties.py puts most of a small image's pixels where that guard has to act.

Shapes are the smallest that reach every kernel form: rcas_dpp_exact_kernel's cells are 62 columns x 32 or 16 rows; launch_rcas takes the
16-row form for tiny launches and the 32-row form when the 32-row grid holds 1025..2048 workgroups; a masked pipeline takes the span form;
rcas_direct_exact_kernel serves a masked RCAS-only launch (no tile lists without an upscale).  A mask-sorted pipeline with tiles inside the
radius always has span records (PrepareTileLists cuts one per run of inside tiles), so that kernel has no mask-sorted case."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import natural, rcas_ties, synth

pytestmark = pytest.mark.gpu
FP32, STRICT, EXACT = 0, 2, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pp(prec, **cfg):
    import openvr_fsr_amd as A
    kw = dict(fsr_enabled=1, radius=2.0, sharpness=0.9, precision=prec)
    kw.update(cfg)
    return A.PostProcessor(**kw)


def _apply(img, prec, eye=0, in_format=None, out_dt=np.uint8, **cfg):
    """one ovrfsr_apply on a fresh ctx into a caller-owned image -> numpy"""
    import torch
    pp = _pp(prec, **cfg)
    try:
        tdt = {np.uint8: torch.uint8, np.float16: torch.float16, np.int32: torch.int32}[out_dt]
        out = pp.apply(eye, _dev(img), out_dtype=tdt, in_format=in_format)
        torch.cuda.synchronize()
        return out.cpu().numpy()
    finally:
        pp.close()


def _batch(imgs, prec, ow, oh, shared=False, in_format=None, **cfg):
    import torch
    pp = _pp(prec, **cfg)
    try:
        texs = _dev(imgs)
        outs = torch.zeros((texs.shape[0], oh, ow, 4), dtype=torch.uint8, device=texs.device)
        pp.apply_batch(texs, outs, shared=shared, in_format=in_format)
        torch.cuda.synchronize()
        return outs.cpu().numpy()
    finally:
        pp.close()


def _ndiff(a, b):
    return int((a != b).sum())


def _rcas_oracle(img8, sharp=rcas_ties.SHARP):
    return O.float_to_unorm8(rcas_ties.rcas_f32(img8, sharp))


def dpp_rows(ow, oh, n):
    """rows per workgroup of the unmasked DPP form for a launch of n images: the arithmetic of rcas_dpp_small (fsr_sizes.h)"""
    wgs = ((ow + 61) // 62) * ((oh + 31) // 32) * n
    full, half = (wgs + 2047) // 2048, (2 * wgs + 2047) // 2048
    return 16 if wgs < 16 * 2048 and 103 * half < 200 * full else 32


# ---- 1, 2: RCAS alone on the tie-rich fixture ---------------------------------------------------------------------------------


def test_rcas_only_tie_rich_16_row_form(gpu):
    img, harvested, n15, n13 = rcas_ties.fixture(7)
    S = rcas_ties.SIZE
    assert dpp_rows(S, S, 1) == 16
    want = _rcas_oracle(img)
    strict = _apply(img, STRICT, stage_mask=2)
    exact = _apply(img, EXACT, stage_mask=2)
    product = _apply(img, FP32, stage_mask=2)
    print("tie-rich fixture (%d pixels within 2^-15 byte): precision 0 differs from strict in %d bytes, precision 3 in %d"
          % (n15, _ndiff(product, strict), _ndiff(exact, strict)))
    assert np.array_equal(strict, want)
    assert np.array_equal(exact, strict), _ndiff(exact, strict)


def test_rcas_only_tie_rich_32_row_form(gpu):
    """192 images, 2 x 3 cells each: 1152 workgroups, the 32-row form.  Image i is the fixture rolled by 3 * (i % 32) texels along both axes
    (the stride-3 grid of neighbourhoods keeps its alignment; only those cut by the wrap-around are lost)."""
    img = rcas_ties.fixture(7)[0]
    S, N = rcas_ties.SIZE, 192
    assert dpp_rows(S, S, N) == 32 and ((S + 61) // 62) * ((S + 31) // 32) * N == 1152
    imgs = np.stack([np.roll(img, (3 * (i % 32), 3 * (i % 32)), axis=(0, 1)) for i in range(N)])
    strict = _batch(imgs, STRICT, S, S, stage_mask=2)
    exact = _batch(imgs, EXACT, S, S, stage_mask=2)
    product = _batch(imgs, FP32, S, S, stage_mask=2)
    print("192 tie-rich images: precision 0 differs from strict in %d bytes, precision 3 in %d" % (_ndiff(product, strict), _ndiff(exact, strict)))
    for i in (0, 1, 95, 191):
        assert np.array_equal(strict[i], _rcas_oracle(imgs[i])), i
    for i in range(N):
        assert np.array_equal(exact[i], strict[i]), (i, _ndiff(exact[i], strict[i]))


# ---- 3, 4: pipelines ----------------------------------------------------------------------------------------------------------


def _contents(w, h):
    rng = np.random.default_rng(11)
    rnd = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    rnd[..., 3] = 255
    return (("uniform-random", rnd), ("natural", np.ascontiguousarray(natural.load("cube")[:h, :w])))


@pytest.mark.parametrize("sharp", [0.9, 0.0])
def test_pipeline_unmasked(gpu, sharp):
    iw, ih, ow, oh = 97, 71, 129, 94
    for name, img in _contents(iw, ih):
        want = O.fsr_pipeline_u8(img, ow, oh, sharpness=sharp)
        strict = _apply(img, STRICT, render_scale=0.75, sharpness=sharp)
        exact = _apply(img, EXACT, render_scale=0.75, sharpness=sharp)
        assert strict.shape == (oh, ow, 4)
        assert np.array_equal(strict, want), name
        assert np.array_equal(exact, strict), (name, _ndiff(exact, strict))


@pytest.mark.parametrize("radius", [0.7, 0.5])
@pytest.mark.parametrize("debug", [0, 1])
def test_pipeline_masked(gpu, radius, debug):
    """the span form, ring tiles, tiles outside the radius and the tint"""
    iw, ih, ow, oh = 144, 120, 192, 160
    for name, img in _contents(iw, ih):
        for eye in (0, 1):
            want = O.fsr_pipeline_u8(img, ow, oh, sharpness=0.9, radius=radius, eye=eye, debug=debug)
            cfg = dict(out_width=ow, out_height=oh, radius=radius, debug_mode=debug)
            strict = _apply(img, STRICT, eye=eye, **cfg)
            exact = _apply(img, EXACT, eye=eye, **cfg)
            assert np.array_equal(strict, want), (name, eye)
            assert np.array_equal(exact, strict), (name, eye, _ndiff(exact, strict))


@pytest.mark.parametrize("debug", [0, 1])
def test_rcas_only_masked_takes_the_per_lane_kernel(gpu, debug):
    """RCAS alone under a radius mask: no tile lists, rcas_direct_exact_kernel with the mask test per 16 x 16 group; the tie-rich fixture tiled
    2 x 2 (192 x 192) so that groups inside and outside the radius both hold near-tie pixels."""
    img = np.tile(rcas_ties.fixture(7)[0], (2, 2, 1))
    centre, rad = O.mask_constants(192, 192, 0.5)
    want = O.float_to_unorm8(O.rcas(O.unorm8_to_float(img), O.rcas_con(0.9, debug), centre, rad))
    strict = _apply(img, STRICT, stage_mask=2, radius=0.5, debug_mode=debug)
    exact = _apply(img, EXACT, stage_mask=2, radius=0.5, debug_mode=debug)
    product = _apply(img, FP32, stage_mask=2, radius=0.5, debug_mode=debug)
    print("masked RCAS-only, tie-rich x4: precision 0 differs from strict in %d bytes" % _ndiff(product, strict))
    assert np.array_equal(strict, want)
    assert np.array_equal(exact, strict), _ndiff(exact, strict)


# ---- 5: other submissions through the same RCAS -------------------------------------------------------------------------------


def test_bgra8_submission(gpu):
    import openvr_fsr_amd as A
    img = _contents(97, 71)[0][1]
    cfg = dict(render_scale=0.75, in_format=A.FORMAT_BGRA8)
    assert np.array_equal(_apply(img, EXACT, **cfg), _apply(img, STRICT, **cfg))
    cfg = dict(stage_mask=2, in_format=A.FORMAT_BGRA8)
    fix = rcas_ties.fixture(7)[0]
    assert np.array_equal(_apply(fix, EXACT, **cfg), _apply(fix, STRICT, **cfg))


def test_multisampled_rgba8_submission_staging_fused(gpu):
    """4 x RGBA8, unmasked: the resolve runs inside EASU's staging sweep under precision 3 as under precision 0"""
    rng = np.random.default_rng(5)
    ms = rng.integers(0, 256, (71, 97, 4, 4), dtype=np.uint8)
    ms[..., 3] = 255
    exact, strict = _apply(ms, EXACT, render_scale=0.75), _apply(ms, STRICT, render_scale=0.75)
    assert exact.shape == (94, 129, 4)
    assert np.array_equal(exact, strict), _ndiff(exact, strict)
    assert np.array_equal(_apply(ms, EXACT, render_scale=0.75, radius=0.6), _apply(ms, STRICT, render_scale=0.75, radius=0.6))


def test_rgba16f_submission_under_reference_formats(gpu):
    """a float submission whose intermediate is RGBA8 (cfg.reference_formats = 1), content reaching 2.0"""
    img = (synth.structured_u8(97, 71, 5).astype(np.float32) * np.float32(2.0 / 255.0)).astype(np.float16)
    img[..., 3] = np.float16(1.0)
    assert float(img[..., :3].max()) > 1.5
    for radius in (2.0, 0.6):
        cfg = dict(render_scale=0.75, reference_formats=1, radius=radius)
        exact, strict = _apply(img, EXACT, **cfg), _apply(img, STRICT, **cfg)
        assert np.array_equal(exact, strict), (radius, _ndiff(exact, strict))


def test_shared_side_by_side_textures(gpu):
    rng = np.random.default_rng(6)
    imgs = rng.integers(0, 256, (2, 72, 192, 4), dtype=np.uint8)
    imgs[..., 3] = 255
    cfg = dict(out_width=256, out_height=96, radius=0.6, shared=True)
    exact, strict = _batch(imgs, EXACT, 256, 96, **cfg), _batch(imgs, STRICT, 256, 96, **cfg)
    assert np.array_equal(exact, strict), _ndiff(exact, strict)


def test_batch_of_four_equals_four_applies(gpu):
    rng = np.random.default_rng(8)
    imgs = rng.integers(0, 256, (4, 71, 97, 4), dtype=np.uint8)
    imgs[..., 3] = 255
    for radius in (2.0, 0.6):
        exact = _batch(imgs, EXACT, 129, 94, render_scale=0.75, radius=radius)
        assert np.array_equal(exact, _batch(imgs, STRICT, 129, 94, render_scale=0.75, radius=radius)), radius
        for i in range(4):
            assert np.array_equal(exact[i], _apply(imgs[i], EXACT, eye=i & 1, render_scale=0.75, radius=radius)), (radius, i)


def test_pair_submit(gpu):
    import torch
    rng = np.random.default_rng(9)
    imgs = rng.integers(0, 256, (2, 71, 97, 4), dtype=np.uint8)
    imgs[..., 3] = 255

    def frame(prec):
        pp = _pp(prec, render_scale=0.75, radius=0.6, pair_submit=1)
        try:
            l, r = _dev(imgs[0]), _dev(imgs[1])
            ol = pp.apply(0, l, out_dtype=torch.uint8)
            assert pp.pair_pending()
            orr = pp.apply(1, r, out_dtype=torch.uint8)
            assert not pp.pair_pending()
            torch.cuda.synchronize()
            return ol.cpu().numpy(), orr.cpu().numpy()
        finally:
            pp.close()

    (el, er), (sl, sr) = frame(EXACT), frame(STRICT)
    assert np.array_equal(el, sl) and np.array_equal(er, sr)
    assert np.array_equal(el, _apply(imgs[0], EXACT, eye=0, render_scale=0.75, radius=0.6))


# ---- 6, 7: refusals and rebuilds ----------------------------------------------------------------------------------------------


def _half(img8):
    h = (img8.astype(np.float32) / np.float32(255.0)).astype(np.float16)
    h[..., 3] = np.float16(1.0)
    return h


def _ten_bit(img8):
    v = img8.astype(np.uint32) * 4
    return (v[..., 0] | (v[..., 1] << 10) | (v[..., 2] << 20) | (np.uint32(3) << 30)).astype(np.uint32).view(np.int32)


REFUSALS = {
    "use_nis": (dict(use_nis=1), lambda u8: u8, np.uint8, "NIS"),
    "fused": (dict(fused=1), lambda u8: u8, np.uint8, "fused"),
    "float intermediate": (dict(quantize_intermediate=0), lambda u8: u8, np.uint8, "quantize_intermediate"),
    "rgba16f out": (dict(), lambda u8: u8, np.float16, "write RGBA8"),
    "rgba16f submission": (dict(), _half, np.uint8, "read RGBA8"),
    "rgb10a2": (dict(), _ten_bit, np.int32, "read RGBA8"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals(gpu, case):
    """UNSUPPORTED with a message that names the reason, the caller's image untouched, the ctx disabled until reset; the same ctx then
    serves the configuration with precision 0."""
    import torch
    import openvr_fsr_amd as A
    extra, make, out_dt, word = REFUSALS[case]
    base = dict(fsr_enabled=1, render_scale=0.75, radius=2.0, sharpness=0.9)
    base.update(extra)
    src = make(synth.structured_u8(97, 71, 3))
    t = _dev(src)
    tdt = {np.uint8: torch.uint8, np.float16: torch.float16, np.int32: torch.int32}[out_dt]
    out = torch.full((94, 129) if out_dt is np.int32 else (94, 129, 4), 77, dtype=tdt, device=t.device)
    pp = A.PostProcessor(precision=EXACT, **base)
    try:
        with pytest.raises(A.OvrFsrError) as ei:
            pp.apply(0, t, out=out)
        assert ei.value.status == 2 and "FP32_EXACT" in str(ei.value) and word in str(ei.value), str(ei.value)
        with pytest.raises(A.OvrFsrError) as ei:
            pp.apply(0, t, out=out)
        assert ei.value.status == 5   # OVRFSR_ERR_DISABLED
        torch.cuda.synchronize()
        assert bool((out == 77).all())
        pp.reset()
        with pytest.raises(A.OvrFsrError) as ei:   # reset enables the ctx; the configuration is still refused
            pp.apply(0, t, out=out)
        assert ei.value.status == 2
        pp.reset()
        pp.set_config(A.Config.default(precision=FP32, **base))
        got = pp.apply(0, t, out=out)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), _apply(src, FP32, out_dt=out_dt, **{k: v for k, v in base.items() if k != "fsr_enabled"}))
    finally:
        pp.close()


def test_set_config_0_3_0(gpu):
    import torch
    import openvr_fsr_amd as A
    img = rcas_ties.fixture(7)[0]
    base = dict(fsr_enabled=1, stage_mask=2, radius=2.0, sharpness=0.9)
    t = _dev(img)
    pp = A.PostProcessor(precision=FP32, **base)
    try:
        def once():
            o = pp.apply(0, t, out_dtype=torch.uint8)
            torch.cuda.synchronize()
            return o.cpu().numpy()
        first = once()
        pp.set_config(A.Config.default(precision=EXACT, **base))
        exact = once()
        pp.set_config(A.Config.default(precision=FP32, **base))
        again = once()
    finally:
        pp.close()
    assert np.array_equal(first, again)
    assert np.array_equal(exact, _rcas_oracle(img))
    assert np.array_equal(first, _apply(img, FP32, stage_mask=2))


# ---- 8, 9: audit and checked builds -------------------------------------------------------------------------------------------


def test_audit_build_finds_no_flip_in_rcas(gpu):
    """tools/debug/tie_audit.py --rcas at a reduced scale against a fresh audit build: every pixel the guarded RCAS instances store is
    evaluated in reference order too.  FLIPS 0 over >= 2e7 pixels with pixels listed; the largest product-versus-reference distance stays
    inside the band (profiles/exact_stores.txt holds the full-scale campaign the band comes from)."""
    from tests.variants import variant
    lib = variant("audit", "-DOVRFSR_TIE_AUDIT")
    env = dict(os.environ, OVRFSR_LIB=lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "debug", "tie_audit.py"), "--rcas", "0.1"], capture_output=True, text=True,
                       timeout=600, env=env, cwd=ROOT)
    print(r.stdout[-8000:])
    m = re.search(r"TOTAL audited (\d+) pixels, listed (\d+) \([\d.]+ %\), FLIPS (\d+), max \|product - reference-order\| ([\d.eE+-]+) byte = ([\d.]+) of the band", r.stdout)
    assert m, (r.stdout[-1500:], r.stderr[-1500:])
    audited, listed, flips, frac = int(m.group(1)), int(m.group(2)), int(m.group(3)), float(m.group(5))
    print("audit: %d pixels, %d listed, %d flips, largest distance %s byte = %.3f of the band" % (audited, listed, flips, m.group(4), frac))
    assert r.returncode == 0 and flips == 0, m.group(0)
    assert audited >= 2e7 and listed > 0, m.group(0)
    assert frac < 1.0, m.group(0)


_CHILD = r"""
import ctypes, sys
sys.path.insert(0, %r)
import numpy as np
import openvr_fsr_amd as A
from tests import rcas_ties, test_gpu_exact_stores as T
lib = A.library()
n = lib.ovrfsr_debug_bounds_slots()
buf = (ctypes.c_ulonglong * n)()
lib.ovrfsr_debug_bounds.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.c_int]
assert lib.ovrfsr_debug_bounds(buf, n, 1) == 0
fix = rcas_ties.fixture(7)[0]
img = T._contents(144, 120)[0][1]
ran = 0
for radius in (2.0, 0.5):
    T._apply(img, T.EXACT, out_width=192, out_height=160, radius=radius); ran += 1
    T._apply(img[:71, :97], T.EXACT, render_scale=0.75, radius=radius); ran += 1
    T._apply(fix, T.EXACT, stage_mask=2, radius=radius); ran += 1
T._batch(np.stack([fix] * 192), T.EXACT, 96, 96, stage_mask=2); ran += 1
import torch; torch.cuda.synchronize()
assert lib.ovrfsr_debug_bounds(buf, n, 0) == 0
nk = (n - 5) // 3
v = list(buf)
print("exact stores checked: launched %%d, checked %%d, out of bounds %%d" %% (ran, sum(v[2 * nk:3 * nk]), sum(v[:nk])))
"""


def test_checked_build(gpu):
    """pipelines (unmasked, span form) and RCAS alone (16-row, 32-row, per-lane kernel) under the -DOVRFSR_BOUNDS build: 0 violations"""
    from tests.variants import variant
    lib = variant("bounds", "-DOVRFSR_BOUNDS")
    env = dict(os.environ, OVRFSR_LIB=lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    m = re.search(r"exact stores checked: launched (\d+), checked (\d+), out of bounds (\d+)", r.stdout)
    assert r.returncode == 0 and m, (r.stdout[-1500:], r.stderr[-1500:])
    print(m.group(0))
    assert int(m.group(1)) == 7 and int(m.group(2)) > 1e5 and int(m.group(3)) == 0, m.group(0)
