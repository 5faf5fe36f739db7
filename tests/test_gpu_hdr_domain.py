"""OVRFSR_HDR_DOMAIN_SRTM on the GPU (include/openvr_fsr_amd.h, "HDR domain").  The contract is a composition, so the main test has no tolerance:
the bytes of an apply with the setting equal -- decode the submission to fp32 in numpy, map it with tests/hdrmap.py, apply it on a second ctx
WITHOUT the setting as an RGBA32F image into an RGBA32F `out`, un-map in numpy, convert to the destination's format.  Then: the strict build
against the oracle, off means off, call shapes (batch, shared, pair_submit, a hidden-area mesh), stream capture, and the checked build.
Content: tests/synth.py's structure scaled to span 0 ... 4000, a dark field with isolated highlights, one texel at 65504, exact zeros."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from openvr_fsr_amd import _capi as K
from oracle import oracle as O
from tests import hdrmap, msaa, packedf, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the issue's shapes: inside, ring and outside tiles per eye; partial last tiles; sharpen-only.  ODD adds what a copy kernel that moves
# 2 or 4 texels per thread can get wrong and those even widths cannot show: a last group of 1, and (with rows padded by 2 texels) bases
# and pitches that are not 16-byte aligned
S1, S2, S3, ODD = (80, 64, 160, 128), (150, 110, 200, 147), (96, 80, 96, 80), (61, 47, 81, 63)
M, U = dict(radius=0.5, proj_centre=(0.2, 0.3, 0.8, 0.7)), dict(radius=2.0)
NP_OF = {"owned": None, "rgba16f": np.float16, "rgba32f": np.float32, "rgba8": np.uint8}


def content(w, h, seed):
    """float32 [h, w, 4], alpha 1, every value exactly representable in half"""
    rng = np.random.default_rng(seed)
    img = synth.structured_u8(w, h, seed).astype(np.float32) / np.float32(255) * np.float32(4000)
    img[:, : w // 3, :3] *= np.float32(1e-4)                              # a dark field (0 ... 0.4) ...
    hot = rng.random((h, w)) < 0.01
    hot[:, w // 3:] = False
    img[hot, :3] = rng.uniform(500.0, 4000.0, (int(hot.sum()), 3)).astype(np.float32)   # ... with isolated highlights
    img[h // 2:h // 2 + 6, w // 2:w // 2 + 9, :3] = 0.0                   # exact zeros: a block, and scattered texels
    img[rng.random((h, w)) < 0.01, :3] = 0.0
    img[h // 4, w // 5, :3] = (65504.0, 3.0, 0.25)                        # one texel at the top of the half range
    img = img.astype(np.float16).astype(np.float32)
    img[..., 3] = 1.0
    return img


def submission(torch, kind, w, h, seed, pad=0):
    """-> (device tensor as submitted, in_format, the fp32 image its texels decode to)"""
    base = content(w, h, seed)
    rng = np.random.default_rng(seed + 77)

    def dev(a):   # rows `pad` texels wider than the image: base and pitch off 16-byte alignment where the texel allows it
        if not pad:
            return torch.from_numpy(np.ascontiguousarray(a)).cuda()
        big = torch.zeros((a.shape[0], a.shape[1] + pad) + a.shape[2:], dtype=torch.from_numpy(a[:1, :1]).dtype, device="cuda")
        big[:, :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return big[:, :a.shape[1]]
    if kind == "rgba16f":
        return dev(base.astype(np.float16)), None, base
    if kind == "rgba32f":
        x = base.copy()
        x[..., :3] *= (np.float32(1) + rng.uniform(0, 1e-4, (h, w, 3)).astype(np.float32))   # (uses the fp32 mantissa)
        return dev(x), None, x
    if kind == "r11":
        words = packedf.encode(base)
        return dev(words), K.FORMAT_R11G11B10F, packedf.unpack(words).astype(np.float32)
    if kind == "ms4":
        ms = base[:, :, None, :] * (np.float32(1) + rng.uniform(-0.05, 0.05, (h, w, 4, 1)).astype(np.float32))
        ms = np.minimum(ms, np.float32(65504)).astype(np.float16)          # (every sample finite: the texel at 65504 stays at or below it)
        ms[..., 3] = np.float16(1)
        return dev(ms), None, msaa.resolve_float(ms).astype(np.float32)
    raise ValueError(kind)


def destination(torch, dest, ow, oh, pad=0):
    if dest == "owned":
        return None
    dt = {"rgba16f": torch.float16, "rgba32f": torch.float32, "rgba8": torch.uint8}[dest]
    big = torch.full((oh, ow + pad, 4), 7, dtype=dt, device="cuda")
    return big[:, :ow]


def composed(torch, A, decoded, eye, ow, oh, np_dtype, cfg):
    """the contract's right-hand side for one image: numpy around a ctx without the setting"""
    ref = A.PostProcessor(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, **cfg)
    try:
        mid = ref.apply(eye, torch.from_numpy(hdrmap.forward(decoded)).cuda(), out_dtype=torch.float32)
        torch.cuda.synchronize()
        mid = mid.cpu().numpy()
    finally:
        ref.close()
    return hdrmap.to_dest(hdrmap.back(mid), np_dtype, O.float_to_unorm8)


def owned_dtype(kind, cfg):
    return np.uint8 if cfg.get("reference_formats") else (np.float32 if kind == "rgba32f" else np.float16)


# submission, form, reference_formats, destination, shape, eye, padded rows
CASES = [
    ("rgba16f", "two-pass", U, 0, "owned", S1, 0, 0),
    ("rgba16f", "masked", M, 0, "rgba16f", S2, 1, 0),
    ("rgba32f", "fused", dict(M, fused=1), 0, "rgba32f", S1, 0, 0),
    ("r11", "easu-only", dict(M, stage_mask=1), 0, "rgba8", S2, 1, 0),
    ("ms4", "sharpen-only", dict(M, stage_mask=2), 0, "owned", S3, 0, 0),
    ("rgba16f", "nvscaler-masked", dict(M, use_nis=1), 0, "rgba16f", S1, 1, 0),
    ("rgba32f", "two-pass", U, 1, "owned", S2, 0, 0),
    ("r11", "masked", M, 1, "owned", S1, 1, 0),
    ("ms4", "masked", M, 0, "rgba8", S1, 0, 0),
    ("rgba16f", "easu-only", dict(U, stage_mask=1), 1, "rgba32f", S1, 0, 0),
    ("r11", "two-pass", U, 0, "owned", S2, 1, 0),
    ("rgba32f", "sharpen-only", dict(U, stage_mask=2), 1, "rgba16f", S3, 1, 0),
    ("ms4", "fused", dict(U, fused=1), 0, "rgba32f", S2, 0, 0),
    # odd widths.  Rows padded by 2 texels: half and byte pitches off 16-byte alignment (texel-by-texel accesses); by 1 or 3: aligned
    # pitches, so 16-byte accesses with a last group of one texel
    ("rgba16f", "masked", M, 0, "rgba16f", ODD, 0, 2),
    ("rgba16f", "two-pass", U, 1, "rgba8", ODD, 1, 3),
    ("rgba32f", "masked", M, 0, "rgba8", ODD, 1, 2),
    ("r11", "easu-only", dict(U, stage_mask=1), 0, "rgba16f", ODD, 0, 1),
    ("ms4", "two-pass", U, 0, "rgba32f", ODD, 1, 1),
]
IDS = ["%s-%s-rf%d-%s-%dx%d%s" % (c[0], c[1], c[3], c[4], c[5][2], c[5][3], "-padded" if c[7] else "") for c in CASES]


def run_case(torch, case):
    """-> (bytes of the apply with the setting, bytes of the composition), both numpy"""
    import openvr_fsr_amd as A
    kind, _, form, rf, dest, (iw, ih, ow, oh), eye, pad = case
    cfg = dict(form, reference_formats=rf)
    tex, in_format, decoded = submission(torch, kind, iw, ih, synth.seed_for(11, eye), pad)
    np_dtype = NP_OF[dest] or owned_dtype(kind, cfg)
    pp = A.PostProcessor(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, **cfg)
    try:
        pp.set_hdr_domain(K.HDR_DOMAIN_SRTM)
        assert pp.hdr_domain() == K.HDR_DOMAIN_SRTM
        out = destination(torch, dest, ow, oh, pad)
        got = pp.apply(eye, tex, out=out, in_format=in_format)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
    finally:
        pp.close()
    assert got.dtype == np_dtype, (got.dtype, np_dtype)     # (a ctx-owned output keeps the submission's own format rule)
    return got, composed(torch, A, decoded, eye, ow, oh, np_dtype, cfg)


def _same(got, want):
    return got.shape == want.shape and np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


# ---- 1. the composition contract, product build -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_composition_contract(gpu, case):
    got, want = run_case(gpu, case)
    differ = np.ascontiguousarray(got).view(np.uint8) != np.ascontiguousarray(want).view(np.uint8)
    print("%d of %d bytes differ" % (int(differ.sum()), differ.size))
    assert got.shape == want.shape and not differ.any()
    # (the image did go through, highlights and all.  Not every value need be finite in a half destination: where RCAS overshoots 2 in the
    # mapped domain the un-mapped value is past the half range -- header -- and the composition holds the same +Inf)
    rgb = got[..., :3].astype(np.float32)
    assert not np.isnan(rgb).any() and rgb[np.isfinite(rgb)].max() > (0.9 if got.dtype == np.uint8 else 100.0)


def test_the_matrix_covers_what_it_must():
    assert {c[0] for c in CASES} == {"rgba16f", "rgba32f", "r11", "ms4"}
    assert {c[1] for c in CASES} == {"two-pass", "masked", "fused", "easu-only", "sharpen-only", "nvscaler-masked"}
    assert {c[3] for c in CASES} == {0, 1} and {c[4] for c in CASES} == {"owned", "rgba16f", "rgba32f", "rgba8"}
    assert {c[5] for c in CASES} >= {S1, S2, S3}


# ---- 2. the strict build against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [U, M], ids=["unmasked", "masked"])
def test_strict_build_equals_the_oracle(gpu, mask):
    torch = gpu
    import openvr_fsr_amd as A
    iw, ih, ow, oh = S1
    eye = 1
    tex, _, decoded = submission(torch, "rgba16f", iw, ih, synth.seed_for(12, eye))
    centre, rad = O.mask_constants(ow, oh, mask["radius"], mask.get("proj_centre", (0.5,) * 4), True, eye)
    e = O.easu(hdrmap.forward(decoded), ow, oh, O.easu_con(iw, ih, ow, oh), centre, rad)      # the strict RGBA32F pipeline keeps an fp32 intermediate
    want = hdrmap.back(O.rcas(e, O.rcas_con(0.9, 0), centre, rad)).astype(np.float16)
    pp = A.PostProcessor(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, precision=A.PRECISION_FP32_STRICT, **mask)
    try:
        pp.set_hdr_domain(K.HDR_DOMAIN_SRTM)
        got = pp.apply(eye, tex, out_dtype=torch.float16)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
    finally:
        pp.close()
    differ = got[..., :3].view(np.uint16) != want[..., :3].view(np.uint16)
    print("%d of %d values differ" % (int(differ.sum()), differ.size))
    assert not differ.any() and (got[..., 3] == np.float16(1)).all()


# ---- 3. off means off ---------------------------------------------------------------------------------------------------------------------------
def test_off_means_off(gpu):
    torch = gpu
    import openvr_fsr_amd as A
    iw, ih, ow, oh = S1
    half = submission(torch, "rgba16f", iw, ih, synth.seed_for(13, 0))[0]
    byte = torch.from_numpy(synth.structured_u8(iw, ih, synth.seed_for(13, 1))).cuda()
    kw = dict(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, **M)
    toggled, never, on = A.PostProcessor(**kw), A.PostProcessor(**kw), A.PostProcessor(**kw)
    try:
        assert toggled.hdr_domain() == K.HDR_DOMAIN_LINEAR                          # the default
        toggled.set_hdr_domain(K.HDR_DOMAIN_SRTM)
        for bad in (-1, 2, 7):                                                       # refused, the stored value stays
            assert toggled._lib.ovrfsr_set_hdr_domain(toggled._ctx, bad) == 1 and toggled.hdr_domain() == K.HDR_DOMAIN_SRTM
        toggled.reset()
        assert toggled.hdr_domain() == K.HDR_DOMAIN_SRTM                            # ovrfsr_reset and ovrfsr_set_config keep it
        toggled.set_config(toggled.cfg)
        assert toggled.hdr_domain() == K.HDR_DOMAIN_SRTM
        mapped = toggled.apply(0, half, out_dtype=torch.float16).clone()
        toggled.set_hdr_domain(K.HDR_DOMAIN_LINEAR)
        a, b = toggled.apply(0, half, out_dtype=torch.float16), never.apply(0, half, out_dtype=torch.float16)
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and not torch.equal(mapped.view(torch.int16), b.view(torch.int16))
        on.set_hdr_domain(K.HDR_DOMAIN_SRTM)
        c, d = on.apply(1, byte, out_dtype=torch.uint8), never.apply(1, byte, out_dtype=torch.uint8)
        torch.cuda.synchronize()
        assert torch.equal(c, d)
    finally:
        for p in (toggled, never, on):
            p.close()


# ---- 4. call shapes ---------------------------------------------------------------------------------------------------------------------------
CORNERS = [[(0, 0), (0.5, 0), (0, 0.6)], [(1, 0), (0.5, 0), (1, 0.6)], [(0, 1), (0.5, 1), (0, 0.4)], [(1, 1), (0.5, 1), (1, 0.4)]]   # four corner wedges


def run_call_shapes(torch):
    """-> [(name, equal)]: a batch of 4 (L, R, L, R) and a pair_submit pair against single applies, a shared side-by-side image against the
    composition, a hidden-area mesh against no mesh"""
    import openvr_fsr_amd as A
    iw, ih, ow, oh = S1
    kw = dict(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, **M)
    built = [submission(torch, "rgba16f", iw, ih, synth.seed_for(14, i)) for i in range(4)]
    texs = torch.stack([b[0] for b in built])
    res = []
    pp, pair = A.PostProcessor(**kw), A.PostProcessor(pair_submit=1, **kw)
    try:
        for p in (pp, pair):
            p.set_hdr_domain(K.HDR_DOMAIN_SRTM)
        single = torch.zeros((4, oh, ow, 4), dtype=torch.float16, device="cuda")
        for i in range(4):
            pp.apply(i & 1, texs[i], out=single[i])
        batch = torch.zeros_like(single)
        pp.apply_batch(texs, batch, first_eye=0, alternate_eyes=True)
        torch.cuda.synchronize()
        res.append(("batch of 4", torch.equal(batch.view(torch.int16), single.view(torch.int16)) and bool((single != 0).any())))
        # pair_submit: the first eye is recorded, the second launches both; R, L order with the outputs in reverse order in memory
        outs = torch.zeros((2, oh, ow, 4), dtype=torch.float16, device="cuda")
        pair.apply(1, texs[1], out=outs[0])
        pending = pair.pair_pending()
        pair.apply(0, texs[0], out=outs[1])
        torch.cuda.synchronize()
        res.append(("pair_submit", pending and not pair.pair_pending() and torch.equal(outs[0].view(torch.int16), single[1].view(torch.int16)) and
                    torch.equal(outs[1].view(torch.int16), single[0].view(torch.int16))))
        # shared side-by-side images, two of them: against the composition through the same call on a ctx without the setting
        shared = torch.zeros((2, oh, ow, 4), dtype=torch.float16, device="cuda")
        pp.apply_batch(texs[:2], shared, shared=True)
        ref = A.PostProcessor(**kw)
        try:
            mid = torch.zeros((2, oh, ow, 4), dtype=torch.float32, device="cuda")
            ref.apply_batch(torch.from_numpy(np.stack([hdrmap.forward(b[2]) for b in built[:2]])).cuda(), mid, shared=True)
            torch.cuda.synchronize()
        finally:
            ref.close()
        want = hdrmap.back(mid.cpu().numpy()).astype(np.float16)
        res.append(("shared", _same(shared.cpu().numpy(), want)))
        # a hidden-area mesh is ignored: same bytes, 0 tiles skipped
        for eye in (0, 1):
            pp.set_hidden_area(eye, CORNERS)
        meshed = torch.zeros((2, oh, ow, 4), dtype=torch.float16, device="cuda")
        for eye in (0, 1):
            pp.apply(eye, texs[eye], out=meshed[eye])
        torch.cuda.synchronize()
        stats = [pp.hidden_area_stats(eye) for eye in (0, 1)]
        hides = K.hidden_tiles(CORNERS, ow, oh)
        res.append(("mesh", bool(hides.any()) and all(s == (hides.size, 0) for s in stats) and torch.equal(meshed.view(torch.int16), single[:2].view(torch.int16))))
    finally:
        pp.close()
        pair.close()
    return res


def test_call_shapes(gpu):
    res = run_call_shapes(gpu)
    assert [n for n, _ in res] == ["batch of 4", "pair_submit", "shared", "mesh"] and all(ok for _, ok in res), res


# ---- 5. steady state --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_capture(gpu):
    """the second apply of a size can be captured and replays to the same bytes; ovrfsr_set_hdr_domain under capture is accepted, the apply
    that must then rebuild is refused with INVALID_ARGUMENT, and the capture stays valid (header, `stream`)"""
    torch = gpu
    import openvr_fsr_amd as A
    iw, ih, ow, oh = S1
    src = torch.stack([submission(torch, "rgba16f", iw, ih, synth.seed_for(15, i))[0] for i in range(2)])
    pp = A.PostProcessor(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, **M)
    pp.set_hdr_domain(K.HDR_DOMAIN_SRTM)
    out = torch.zeros((2, oh, ow, 4), dtype=torch.float16, device="cuda")
    ref = torch.zeros_like(out)
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
                    pp.apply_batch(src, out)
                except A.OvrFsrError as e:
                    err = e
        torch.cuda.synchronize()
        return g, err

    try:
        g, err = capture()
        assert err is not None and err.status == 1, err        # the first call for a size builds: refused, nothing touched
        pp.apply_batch(src, ref)
        torch.cuda.synchronize()
        g, err = capture()
        assert err is None
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), ref.view(torch.int16)) and bool((ref != 0).any())
        g, err = capture(lambda: pp.set_hdr_domain(K.HDR_DOMAIN_LINEAR))   # the setter is accepted, the rebuild it asks for is not
        assert err is not None and err.status == 1 and pp.hdr_domain() == K.HDR_DOMAIN_LINEAR, err
        pp.set_hdr_domain(K.HDR_DOMAIN_SRTM)
        pp.apply_batch(src, out)                                             # the ctx stayed enabled
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    finally:
        pp.close()


def test_debug_timer_brackets_the_passes(gpu):
    """the debug-mode timer gives a reading for an apply with the setting (it starts in front of the forward pass and ends behind the back pass)"""
    torch = gpu
    import openvr_fsr_amd as A
    iw, ih, ow, oh = S1
    tex = submission(torch, "rgba16f", iw, ih, synth.seed_for(16, 0))[0]
    pp = A.PostProcessor(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, debug_mode=1, **U)
    try:
        pp.set_hdr_domain(K.HDR_DOMAIN_SRTM)
        pp.apply(0, tex, out_dtype=torch.float16)
        assert pp.last_gpu_time_ms() > 0.0
    finally:
        pp.close()


# ---- 6. the checked build ---------------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import ctypes, sys
sys.path.insert(0, %r)
import numpy as np
import torch
import openvr_fsr_amd as A
from tests import test_gpu_hdr_domain as T
lib = A.library()
n = lib.ovrfsr_debug_bounds_slots()
buf = (ctypes.c_ulonglong * n)()
lib.ovrfsr_debug_bounds.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.c_int]
assert lib.ovrfsr_debug_bounds(buf, n, 1) == 0
bad = []
for case, name in zip(T.CASES, T.IDS):
    got, want = T.run_case(torch, case)
    if not T._same(got, want):
        bad.append(name)
bad += [name for name, ok in T.run_call_shapes(torch) if not ok]
torch.cuda.synchronize()
assert lib.ovrfsr_debug_bounds(buf, n, 0) == 0
nk = (n - 5) // 3
v = list(buf)
print("HDR domain checked: cases %%d, mismatches %%d %%s, checked %%d, out of bounds %%d" %% (len(T.CASES) + 4, len(bad), bad, sum(v[2 * nk:3 * nk]), sum(v[:nk])))
"""


def test_checked_build(gpu):
    """cases 1 and 4 against the -DOVRFSR_BOUNDS build: every access of the two passes (and of everything between them) through the checked
    accessors, 0 violations, and the bytes still equal (a wrongly redirected access would corrupt them)"""
    from tests.variants import variant
    lib = variant("bounds", "-DOVRFSR_BOUNDS")
    env = dict(os.environ, OVRFSR_LIB=lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    m = re.search(r"HDR domain checked: cases (\d+), mismatches (\d+) .*, checked (\d+), out of bounds (\d+)", r.stdout)
    assert r.returncode == 0 and m, (r.stdout[-1500:], r.stderr[-1500:])
    assert int(m.group(1)) == len(CASES) + 4 and int(m.group(2)) == 0 and int(m.group(3)) > 1e6 and int(m.group(4)) == 0, m.group(0)
