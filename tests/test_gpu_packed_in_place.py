"""R11G11B10F eye images decoded inside kernel staging, on the GPU: wherever the product build's fixed-pitch kernels read the packed words
themselves (easu_fast_kernel, fused_kernel, easu_outside_kernel: every form with an upscale stage), every output byte is the byte of the
same call on the RGBA16F image holding the decoded values (tests/packedf.py) -- on the three LDS pitches, on rows that are only 4-byte
aligned, on clamped columns, across eye passes and batch strides; no ctx-owned RGBA16F copy of the submission exists any more; the checked
build finds no access out of bounds; and on HDR content the near-tie guards list exactly the pixels they list for the RGBA16F image."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import packedf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF_CENTRE = (0.2, 0.3, 0.8, 0.7)

# (input w, h, words of row padding, output w, h).  LDS pitch of the EASU-only kernel: 28 (scale 3/4: interior tiles take the quad sweep), 32,
# 40; 37 + 3 / + 2 pad words: rows 4- but not 16- / 8-byte aligned, nearly every tile on the border (flat clamped sweep); 1x5: every column
# clamped (the unpaired loads of the outside-tile bilinear); 200x160 -> 128x102: refused for RGBA16F too (one tile's footprint exceeds the
# LDS); 160x128 -> 128x102: a 44-cell footprint, beyond the fixed pitches -- the resolve pass and the generic kernel, still equal.
SHAPES = ((96, 80, 0, 128, 107), (110, 92, 0, 128, 107), (116, 97, 0, 128, 107), (37, 29, 3, 49, 39), (37, 29, 2, 49, 39), (1, 5, 0, 2, 7),
          (200, 160, 0, 128, 102), (160, 128, 0, 128, 102))
SMALLEST = (SHAPES[5], SHAPES[3], SHAPES[4])
SCALES = (1.0, 6.0, 40.0)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _torch_dtype(dt):
    import torch
    return {np.uint8: torch.uint8, np.float16: torch.float16, np.float32: torch.float32}[dt]


def _padded(packed, pad):
    """the packed image [H, W] as a device view whose rows are `pad` NaN words longer than the image"""
    import torch
    t = _dev(packed)
    if not pad:
        return t
    big = torch.full((t.shape[0], t.shape[1] + pad), 0x7FFFFFFF, dtype=torch.int32, device="cuda")   # NaN codes: must never be read
    big[:, :t.shape[1]] = t
    return big[:, :t.shape[1]]


def _apply(img, ow, oh, out_dt, pad=0, **cfg):
    """one ovrfsr_apply on a fresh ctx -> numpy output; out_dt None: the ctx-owned image.  int32 images are R11G11B10F, float16 ones RGBA16F."""
    import torch
    import openvr_fsr_amd as A
    kw = dict(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9)
    kw.update(cfg)
    pp = A.PostProcessor(**kw)
    try:
        dt = _torch_dtype(out_dt) if out_dt is not None else None
        if img.dtype == np.int32:
            out = pp.apply(0, _padded(img, pad), out_dtype=dt, in_format=A.FORMAT_R11G11B10F)
        else:
            out = pp.apply(0, _dev(img), out_dtype=dt)
        torch.cuda.synchronize()
        return out.cpu().numpy()
    finally:
        pp.close()


def _twin(packed, ow, oh, out_dt, pad=0, **cfg):
    """(status, or dtype + bytes, of the packed apply; the same of the RGBA16F apply of the decoded image), each on a fresh ctx"""
    import openvr_fsr_amd as A
    res = []
    for img in (packed, packedf.unpack(packed)):
        try:
            o = _apply(img, ow, oh, out_dt, pad=pad if img is packed else 0, **cfg)
            res.append((str(o.dtype), o.shape, o.tobytes()))
        except A.OvrFsrError as e:
            res.append(e.status)
    return res


DESTS = (np.uint8, np.float16, np.float32, None)   # None: the ctx-owned image


def configs():
    """(configuration index, destination index, configuration, destination): precision 0 on everything, precision 3 only where it is
    promised (reference_formats, RGBA8 destination)"""
    ci = 0
    for radius in (2.0, 0.5):
        for fused in (-1, 0, 1):
            for stage_mask in (0, 1):
                for ref in (0, 1):
                    cfg = dict(precision=0, radius=radius, fused=fused, stage_mask=stage_mask, reference_formats=ref)
                    if radius == 0.5:
                        cfg["proj_centre"] = OFF_CENTRE
                    for di, out_dt in enumerate(DESTS):
                        yield ci, di, cfg, out_dt
                    if ref and fused != 1:
                        yield ci, len(DESTS), dict(cfg, precision=3), np.uint8
                    ci += 1


def matrix(shapes=SHAPES):
    """Every (configuration, destination) on two of the shapes, rotated so that every configuration meets every shape (8 shapes = 4
    destinations x 2) and every shape every destination.  -> (cases, cases that launched, failing cases)"""
    bad, ran, launched = [], 0, 0
    n = len(shapes)
    for ci, di, cfg, out_dt in configs():
        for s in sorted({(2 * di + ci) % n, (2 * di + 1 + ci) % n}):
            w, h, pad, ow, oh = shapes[s]
            seed = 40 * ci + 8 * di + s
            packed = packedf.make(w, h, ("structured", "random", "natural")[seed % 3], seed, SCALES[(seed // 3) % 3])
            got, want = _twin(packed, ow, oh, out_dt, pad=pad, **cfg)
            ran += 1
            launched += not isinstance(want, int)
            if got != want:
                bad.append((cfg, getattr(out_dt, "__name__", "owned"), shapes[s], got if isinstance(got, int) else "bytes",
                            want if isinstance(want, int) else "bytes"))
    return ran, launched, bad


# ---- 1. equality with the RGBA16F twin ------------------------------------------------------------------------------------------------


def test_output_bytes_equal_the_rgba16f_twin(gpu):
    ran, launched, bad = matrix()
    print("R11G11B10F in place: %d cases, %d launched, %d differ" % (ran, launched, len(bad)))
    assert launched * 3 > 2 * ran, (ran, launched)   # not a list of refusals (a refusal must be the twin's: compared as a status above)
    assert not bad, bad[:5]


# ---- 2. eye parity and in_stride --------------------------------------------------------------------------------------------------


def _batch(src, out_shape, out_dt, in_format=None, row_gap=0, **call):
    """apply_batch on a fresh ctx; row_gap: rows of NaN words between the images (in_stride exceeds the image)"""
    import torch
    import openvr_fsr_amd as A
    pp = A.PostProcessor(fsr_enabled=1, out_width=out_shape[2], out_height=out_shape[1], radius=0.5, proj_centre=OFF_CENTRE, sharpness=0.9)
    try:
        t = _dev(src)
        if row_gap:
            big = torch.full((t.shape[0], t.shape[1] + row_gap) + tuple(t.shape[2:]), 0x7FFFFFFF, dtype=t.dtype, device="cuda")
            big[:, :t.shape[1]] = t
            t = big[:, :t.shape[1]]
        o = torch.zeros(out_shape + (4,), dtype=_torch_dtype(out_dt), device="cuda")
        pp.apply_batch(t, o, in_format=in_format, **call)
        torch.cuda.synchronize()
        return o.cpu().numpy()
    finally:
        pp.close()


def test_batches_equal_their_twins(gpu):
    import openvr_fsr_amd as A
    # 5 alternating eyes, masked with unequal eye centres (two eye passes over stride-2 sub-batches), 7 rows of NaN words between the images
    packed = np.stack([packedf.make(96, 80, "structured", 30 + i, SCALES[i % 3]) for i in range(5)])
    dec = np.stack([packedf.unpack(p) for p in packed])
    got = _batch(packed, (5, 107, 128), np.float16, in_format=A.FORMAT_R11G11B10F, row_gap=7, first_eye=1)
    want = _batch(dec, (5, 107, 128), np.float16, first_eye=1)
    assert got.tobytes() == want.tobytes()
    assert got[0].tobytes() != got[2].tobytes()   # (the images differ: a wrong stride would show)
    # side-by-side textures holding both eyes
    packed = np.stack([packedf.make(192, 80, "natural", 50 + i, SCALES[i % 3]) for i in range(3)])
    dec = np.stack([packedf.unpack(p) for p in packed])
    got = _batch(packed, (3, 107, 256), np.uint8, in_format=A.FORMAT_R11G11B10F, shared=True)
    want = _batch(dec, (3, 107, 256), np.uint8, shared=True)
    assert got.tobytes() == want.tobytes()


# ---- 3. no copy is built ------------------------------------------------------------------------------------------------------------


def test_no_copy_of_the_submission_is_built(gpu):
    """Device memory a ctx takes for a masked 1024x768 -> 1365x1024 apply into a caller-owned RGBA16F image: the packed ctx may exceed the
    RGBA16F twin's by less than half of the 1024 x 768 x 8-byte copy the resolve pass used to write (it exceeded it by the whole copy)."""
    import torch
    import openvr_fsr_amd as A
    iw, ih, ow, oh = 1024, 768, 1365, 1024
    packed = packedf.make(iw, ih, "structured", 5, 6.0)
    srcs = (_dev(packed), _dev(packedf.unpack(packed)))
    outs = [torch.zeros((oh, ow, 4), dtype=torch.float16, device="cuda") for _ in srcs]
    # (the kernels' code object is loaded at a process's first launch: both routes once on a small image before anything is measured)
    small = packedf.make(96, 80, "structured", 4)
    for img in (small, packedf.unpack(small)):
        _apply(img, 128, 107, np.float16, radius=0.5, proj_centre=OFF_CENTRE)
    torch.cuda.synchronize()
    taken = []
    for src, out, fmt in zip(srcs, outs, (A.FORMAT_R11G11B10F, None)):
        free0 = torch.cuda.mem_get_info()[0]
        pp = A.PostProcessor(fsr_enabled=1, out_width=ow, out_height=oh, radius=0.5, proj_centre=OFF_CENTRE, sharpness=0.9)
        pp.apply(0, src, out=out, in_format=fmt)
        torch.cuda.synchronize()
        taken.append(free0 - torch.cuda.mem_get_info()[0])
        pp.close()
    print("device memory taken: packed ctx %d bytes, RGBA16F ctx %d bytes" % tuple(taken))
    assert outs[0].cpu().numpy().tobytes() == outs[1].cpu().numpy().tobytes()
    assert taken[0] - taken[1] <= iw * ih * 8 // 2, taken


def test_masked_forms_are_equal_where_a_last_bit_would_show(gpu):
    """Equality again at 1024x768 -> 1365x1024, masked, random HDR content: the bilinear fallback of the tiles outside the radius rounds a
    contracted blend to half in some forms, and a kernel that fused that rounding for other pixels than its RGBA16F twin would differ in
    about one value of 10^4 -- invisible on the small shapes above, some hundred values here.  (Forms whose outside-tile kernel was not
    shown equal this way run behind the resolve pass: pipeline_plan.cpp, packed_in_staging.)"""
    iw, ih, ow, oh = 1024, 768, 1365, 1024
    packed = packedf.make(iw, ih, "random", 5, 6.0)
    bad = []
    for cfg in (dict(), dict(quantize_intermediate=0), dict(reference_formats=1), dict(stage_mask=1), dict(fused=0)):
        for out_dt in (np.uint8, np.float16, np.float32):
            got, want = _twin(packed, ow, oh, out_dt, radius=0.5, proj_centre=OFF_CENTRE, **cfg)
            assert not isinstance(want, int), (cfg, want)
            if got != want:
                bad.append((cfg, out_dt.__name__))
    assert not bad, bad


# ---- 4. checked build ---------------------------------------------------------------------------------------------------------------

_CHILD_BOUNDS = r"""
import ctypes, sys
sys.path.insert(0, %r)
import openvr_fsr_amd as A
from tests import test_gpu_packed_in_place as T
lib = A.library()
n = lib.ovrfsr_debug_bounds_slots()
buf = (ctypes.c_ulonglong * n)()
lib.ovrfsr_debug_bounds.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.c_int]
assert lib.ovrfsr_debug_bounds(buf, n, 1) == 0
ran, launched, bad = T.matrix(T.SMALLEST)
import torch; torch.cuda.synchronize()
assert lib.ovrfsr_debug_bounds(buf, n, 0) == 0
nk = (n - 5) // 3
v = list(buf)
print("in place checked: launched %%d, mismatches %%d, checked %%d, out of bounds %%d" %% (launched, len(bad), sum(v[2 * nk:3 * nk]), sum(v[:nk])))
"""


def test_checked_build_matrix(gpu):
    """The matrix on its three smallest shapes against the -DOVRFSR_BOUNDS build: every image, LDS and table access of the new instances
    through the checked accessors, 0 violations."""
    from tests.variants import variant
    lib = variant("bounds", "-DOVRFSR_BOUNDS")
    env = dict(os.environ, OVRFSR_LIB=lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", _CHILD_BOUNDS % ROOT], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    m = re.search(r"in place checked: launched (\d+), mismatches (\d+), checked (\d+), out of bounds (\d+)", r.stdout)
    assert r.returncode == 0 and m, (r.stdout[-1500:], r.stderr[-1500:])
    print(m.group(0))
    assert int(m.group(1)) > 100 and int(m.group(2)) == 0 and int(m.group(3)) > 1e6 and int(m.group(4)) == 0, m.group(0)


# ---- 5. guard parity on HDR -----------------------------------------------------------------------------------------------------------

_CHILD_AUDIT = r"""
import ctypes, sys
sys.path.insert(0, %r)
import numpy as np
import openvr_fsr_amd as A
from tests import packedf
from tests import test_gpu_packed_in_place as T
lib = A.library()
c = (ctypes.c_ulonglong * 6)()
packed = packedf.make(110, 92, "natural", 21, 40.0)
assert float(packedf.unpack(packed).astype(np.float32)[..., :3].max()) > 8.0
for name, out_dt, cfg in (("masked half pipeline", np.float16, dict(radius=0.5, proj_centre=T.OFF_CENTRE)),
                          ("reference_formats unmasked", np.uint8, dict(radius=2.0, reference_formats=1))):
    counts = []
    for img in (packed, packedf.unpack(packed)):
        assert lib.ovrfsr_debug_tie_audit(c, 1) == 0
        T._apply(img, 128, 107, out_dt, **cfg)
        assert lib.ovrfsr_debug_tie_audit(c, 0) == 0
        counts.append((int(c[0]), int(c[1]), int(c[2])))
    print("in place audit, %%s: packed %%d %%d %%d twin %%d %%d %%d" %% ((name,) + counts[0] + counts[1]))
"""


def test_guards_list_the_same_pixels_on_hdr_content(gpu):
    """-DOVRFSR_TIE_AUDIT, content at scale 40 (the guards' HDR bands, scaled by the staged footprint's largest channel): the audited and listed
    counts of the packed run equal the RGBA16F twin's, and no unlisted pixel flips in either -- a staging sweep that forgot the footprint
    maximum would list fewer pixels."""
    from tests.variants import variant
    lib = variant("audit", "-DOVRFSR_TIE_AUDIT")
    env = dict(os.environ, OVRFSR_LIB=lib, PYTHONPATH=ROOT)
    env.pop("OVRFSR_TIE_HALF_MIN", None)
    r = subprocess.run([sys.executable, "-c", _CHILD_AUDIT % ROOT], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    found = re.findall(r"in place audit, ([^:]+): packed (\d+) (\d+) (\d+) twin (\d+) (\d+) (\d+)", r.stdout)
    assert r.returncode == 0 and len(found) == 2, (r.stdout[-1500:], r.stderr[-1500:])
    for name, *v in found:
        pa, pl, pf, ta, tl, tf = map(int, v)
        print("%s: audited %d / %d, listed %d / %d, unlisted flips %d / %d" % (name, pa, ta, pl, tl, pf, tf))
        assert pa == ta and pa > 1000, (name, v)
        assert pl == tl and pl > 0, (name, v)
        assert pf == 0 and tf == 0, (name, v)
