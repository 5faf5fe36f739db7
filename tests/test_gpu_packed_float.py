"""R11G11B10F input images (OVRFSR_FORMAT_R11G11B10F) on the GPU: every output is, byte for byte, the output of the same call on the
RGBA16F image that tests/packedf.py's numpy decode (and, for multisampled images, numpy resolve) makes of the packed words -- on every
path, in both builds -- plus the oracle behind the decode, and the refusals / rebuilds the header promises.  (A library without the
format refuses it with OVRFSR_ERR_UNSUPPORTED.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import packedf

pytestmark = pytest.mark.gpu
STRICT, FP32 = 2, 0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (width, height, words of row padding behind the image).  Odd widths: the last thread of a row has one texel.  37 + 3 words = 160-byte
# rows: the vector path with a scalar last group; 37 + 2 = 156-byte rows: not 8-byte aligned, the scalar path throughout; width 1: below
# one thread's two texels; 96: even, interior EASU tiles take the quad staging sweep; 66 + 1 = 268 bytes: 8- but not 16-byte aligned rows
# (vector path at S = 1 only).
SOURCES = ((37, 29, 3), (37, 29, 2), (1, 5, 0), (96, 80, 0), (66, 40, 1))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _torch_dtype(dt):
    import torch
    return {np.uint8: torch.uint8, np.float16: torch.float16, np.float32: torch.float32}[dt]


def _padded(packed, pad):
    """the packed image ([H, W] or [H, W, S]) as a device view whose rows are `pad` words longer than the image"""
    import torch
    t = _dev(packed)
    if not pad:
        return t
    if t.dim() == 2:
        big = torch.full((t.shape[0], t.shape[1] + pad), 0x7FFFFFFF, dtype=torch.int32, device="cuda")  # NaN words: must never be read
        big[:, :t.shape[1]] = t
        return big[:, :t.shape[1]]
    s = t.shape[2]
    flat = torch.full((t.shape[0], t.shape[1] * s + pad), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    flat[:, :t.shape[1] * s] = t.reshape(t.shape[0], -1)
    return flat.as_strided(tuple(t.shape), (flat.stride(0), s, 1))


def _apply(img, ow, oh, out_dt, eye=0, pad=0, **cfg):
    """one ovrfsr_apply on a fresh ctx -> numpy output.  int32 images are R11G11B10F ([H, W] or [H, W, S]), float16 ones RGBA16F."""
    import torch
    import openvr_fsr_amd as A
    kw = dict(fsr_enabled=1, out_width=ow, out_height=oh, radius=2.0, sharpness=0.9)
    kw.update(cfg)
    pp = A.PostProcessor(**kw)
    try:
        if img.dtype == np.int32:
            out = pp.apply(eye, _padded(img, pad), out_dtype=_torch_dtype(out_dt), in_format=A.FORMAT_R11G11B10F)
        else:
            out = pp.apply(eye, _dev(img), out_dtype=_torch_dtype(out_dt))
        torch.cuda.synchronize()
        return out.cpu().numpy()
    finally:
        pp.close()


def _decoded(packed):
    """the RGBA16F image holding the same values: the decode, behind the numpy resolve for a multisampled image"""
    return packedf.unpack(packed) if packed.ndim == 2 else packedf.resolve(packed)


def _twin(packed, ow, oh, out_dt, pad=0, **cfg):
    """(status or bytes of the packed apply, status or bytes of the RGBA16F apply of the decoded image)"""
    import openvr_fsr_amd as A
    res = []
    for img in (packed, _decoded(packed)):
        try:
            res.append(_apply(img, ow, oh, out_dt, pad=pad if img is packed else 0, **cfg).tobytes())
        except A.OvrFsrError as e:
            res.append(e.status)
    return res


def configs():
    """builds x FSR / NIS x radius x cfg.fused x stage masks: what the issue's equality matrix names"""
    for prec in (FP32, STRICT):
        for nis in (0, 1):
            for radius in (2.0, 0.5):
                for fused in (-1, 0, 1):
                    for stage_mask in (0, 1, 2):
                        yield dict(precision=prec, use_nis=nis, radius=radius, fused=fused, stage_mask=stage_mask)


def matrix(samples, sources=SOURCES):
    """Every configuration x output format x source shape, for one sample count.  A configuration the RGBA16F route refuses must be
    refused with the same status.  Returns (cases run, cases that launched, list of failing cases)."""
    bad, ran, launched = [], 0, 0
    seed = 0
    for cfg in configs():
        for out_dt in (np.uint8, np.float16, np.float32):
            for i, (w, h, pad) in enumerate(sources):
                # the whole matrix on the first two sources (vector and scalar path), the others on a third of it
                if i >= 2 and (seed + i) % 3:
                    continue
                seed += 1
                ow, oh = (w, h) if cfg["stage_mask"] == 2 else ((w * 4 + 2) // 3, (h * 4 + 2) // 3)
                content = ("structured", "random", "natural")[seed % 3]
                scale = (1.0, 6.0)[seed % 2]
                packed = packedf.make(w, h, content, seed, scale) if samples == 1 else packedf.make_ms(w, h, samples, content, seed, scale)
                got, want = _twin(packed, ow, oh, out_dt, pad=pad, **cfg)
                ran += 1
                launched += isinstance(want, bytes)
                if got != want:
                    bad.append((samples, cfg, out_dt.__name__, (w, h, pad), got if isinstance(got, int) else "bytes",
                                want if isinstance(want, int) else "bytes"))
    return ran, launched, bad


# ---- equality with the RGBA16F apply of the decoded image ---------------------------------------------------------------------


def test_output_bytes_equal_the_rgba16f_apply(gpu):
    ran, launched, bad = matrix(1)
    print("R11G11B10F equality: %d cases, %d launched, %d differ" % (ran, launched, len(bad)))
    assert launched * 2 > ran, (ran, launched)   # the matrix is not a list of refusals
    assert not bad, bad[:5]


@pytest.mark.parametrize("samples", [2, 4, 8])
def test_multisampled_output_bytes_equal_the_rgba16f_apply_of_the_resolved_image(gpu, samples):
    ran, launched, bad = matrix(samples)
    print("R11G11B10F x%d equality: %d cases, %d launched, %d differ" % (samples, ran, launched, len(bad)))
    assert launched * 2 > ran, (ran, launched)
    assert not bad, bad[:5]


@pytest.mark.parametrize("stage_mask", [0, 1])
def test_sum_order_on_the_device(gpu, stage_mask):
    """The fp32 sample-order rule pinned on the device.  No negative values exist in this format, so the order shows only where the sum
    lands next to a half rounding tie: the sample set below (tests/test_packed_float.py) resolves to 4544 in sample order and to 4548
    reversed.  Laid out in blocks so that whole EASU footprints see one answer."""
    c = np.array((1854, 342, 1617, 1567), np.uint32)
    fwd = packedf.pack(c, c, c >> 1)
    h, w = 80, 96
    blk = ((np.arange(h)[:, None] // 8 + np.arange(w)[None, :] // 8) % 2).astype(bool)
    ms = np.empty((h, w, 4), np.int32)
    ms[blk] = fwd
    ms[~blk] = fwd[::-1]
    ss = packedf.resolve(ms)
    assert set(np.unique(ss[..., 0]).tolist()) == {4544.0, 4548.0}
    got, want = _twin(ms, 128, 107, np.float16, stage_mask=stage_mask)
    assert isinstance(got, bytes) and got == want
    # and the outputs do tell the two answers apart
    flat = ss.copy()
    flat[..., :2] = np.float16(4544.0)
    assert got != _apply(flat, 128, 107, np.float16, stage_mask=stage_mask).tobytes()


# ---- the oracle behind the decode ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("samples", [1, 4])
@pytest.mark.parametrize("scale", [1.0, 40.0, 65024.0])
def test_against_the_oracle(gpu, samples, scale):
    """The CPU oracle on the decoded floats, held to what tests/test_gpu_formats.py::test_half_pipeline_hdr_values holds an RGBA16F
    input of this configuration to (EASU -> half intermediate -> RCAS, radius 0.6): the strict build bit-exact at every magnitude, the
    product build within 1e-3 relative to the image's magnitude on every form of the pipeline, the same pixels finite.  65024 is the
    format's largest finite value (R, G; blue reaches 64512)."""
    from oracle import oracle as O
    iw, ih, ow, oh = 237, 180, 316, 240
    from tests import msaa
    u8 = msaa._base_u8(iw, ih, 91, "structured") if samples == 1 else msaa.make_ms(iw, ih, samples, "rgba8", "structured", 91)
    unit = u8[..., :3].astype(np.float32) / u8[..., :3].reshape(-1, 3).max(axis=0).astype(np.float32)   # every channel reaches 1.0
    packed = packedf.encode(unit * np.float32(scale))
    imgh = _decoded(packed)
    if scale == 65024.0:
        top = packedf.unpack(packed).astype(np.float32).reshape(-1, 4).max(axis=0)
        assert top.tolist() == [packedf.MAX_RG, packedf.MAX_RG, packedf.MAX_B, 1.0]
    centre, rad = O.mask_constants(ow, oh, 0.6)
    e = O.easu(imgh.astype(np.float32), ow, oh, O.easu_con(iw, ih, ow, oh), centre, rad)
    with np.errstate(over="ignore", invalid="ignore"):
        want = O.rcas(e.astype(np.float16).astype(np.float32), O.rcas_con(0.9), centre, rad).astype(np.float16)
    kw = dict(sharpness=0.9, radius=0.6)
    got = _apply(packed, ow, oh, np.float16, precision=STRICT, **kw)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), scale
    for fused in (-1, 0, 1):
        got = _apply(packed, ow, oh, np.float16, precision=FP32, fused=fused, **kw).astype(np.float32)
        w32 = want.astype(np.float32)
        ok = np.isfinite(w32)
        err = np.abs(got[ok] - w32[ok])
        print("scale %g, S %d, fused %d: max abs error %g (bound %g)" % (scale, samples, fused, float(err.max()), 1e-3 * max(1.0, scale)))
        assert err.max() <= 1e-3 * max(1.0, scale), (scale, fused, float(err.max()))
        assert np.array_equal(np.isfinite(got), ok)


def test_c5_size(gpu):
    """The full C5 shape (2370^2 -> 3160^2, radius 0.5, RGBA16F output) against the oracle on the decoded image, with the thresholds of
    tests/test_gpu_parity.py's C5 case: the strict build bit-exact, the product build within 1e-3; and both builds equal to the RGBA16F
    apply byte for byte."""
    from oracle import oracle as O
    iw, ih, ow, oh = 2370, 2370, 3160, 3160
    packed = packedf.make(iw, ih, "structured", 77)
    imgh = packedf.unpack(packed)
    centre, rad = O.mask_constants(ow, oh, 0.5)
    e = O.easu(imgh.astype(np.float32), ow, oh, O.easu_con(iw, ih, ow, oh), centre, rad)
    want = O.rcas(e.astype(np.float16).astype(np.float32), O.rcas_con(0.9), centre, rad).astype(np.float16)
    got = _apply(packed, ow, oh, np.float16, precision=STRICT, radius=0.5)
    assert np.array_equal(got, want)
    assert got.tobytes() == _apply(imgh, ow, oh, np.float16, precision=STRICT, radius=0.5).tobytes()
    prod = _apply(packed, ow, oh, np.float16, precision=FP32, radius=0.5)
    assert prod.tobytes() == _apply(imgh, ow, oh, np.float16, precision=FP32, radius=0.5).tobytes()
    err = np.abs(prod.astype(np.float32) - want.astype(np.float32))
    print("C5 product build: max abs error %g" % float(err.max()))
    assert err.max() <= 1e-3, (float(err.max()), int((err > 1e-3).sum()))


def test_inf_and_nan_codes_stay_local(gpu):
    """Inf / NaN codes are outside the parity contract and inside the memory-safety one: pixels whose taps do not reach such a texel equal
    the RGBA16F run (which holds the same Inf / NaN halves).  The checked pixels lie more than 8 output pixels (EASU's 12 taps reach 2
    texels, RCAS one more pixel, the tiles' near-tie bands none further) from every such texel's footprint."""
    iw, ih, ow, oh = 96, 80, 128, 107
    packed = packedf.make(iw, ih, "structured", 12, 3.0).copy()
    u = packed.view(np.uint32)
    spots = ((10, 12, 0x7C0, 0, 0), (40, 70, 0, 0x7FF, 0), (60, 30, 0, 0, 0x3E0), (70, 85, 0x7C1, 0x7C0, 0x3FF))
    far = np.ones((oh, ow), bool)
    yy, xx = np.mgrid[0:oh, 0:ow]
    for (y, x, r, g, b) in spots:
        u[y, x] = r | (g << 11) | (b << 22)
        cy, cx = (y + 0.5) * oh / ih, (x + 0.5) * ow / iw
        far &= (np.abs(yy - cy) > 12) | (np.abs(xx - cx) > 12)
    assert far.mean() > 0.5
    imgh = packedf.unpack(packed)
    assert not np.isfinite(imgh.astype(np.float32)).all()
    for prec in (FP32, STRICT):
        for fused in (0, 1):
            got = _apply(packed, ow, oh, np.float16, precision=prec, fused=fused, radius=0.5)
            want = _apply(imgh, ow, oh, np.float16, precision=prec, fused=fused, radius=0.5)
            assert np.array_equal(got.view(np.uint16)[far], want.view(np.uint16)[far]), (prec, fused)


# ---- batches, pairs, ctx-owned output -----------------------------------------------------------------------------------------


def _pp(**cfg):
    import openvr_fsr_amd as A
    kw = dict(fsr_enabled=1, out_width=128, out_height=107, radius=0.5, sharpness=0.9)
    kw.update(cfg)
    return A.PostProcessor(**kw)


def _img(seed=7, w=96, h=80, s=1, scale=2.0):
    return packedf.make(w, h, "structured", seed, scale) if s == 1 else packedf.make_ms(w, h, s, "structured", seed, scale)


@pytest.mark.parametrize("samples", [1, 4])
def test_batch_of_alternating_eyes(gpu, samples):
    import torch
    import openvr_fsr_amd as A
    n = 6
    packed = np.stack([_img(30 + i, s=samples) for i in range(n)])
    dec = np.stack([_decoded(p) for p in packed])
    outs = []
    for src, fmt in ((packed, A.FORMAT_R11G11B10F), (dec, None)):
        pp = _pp()
        o = torch.zeros((n, 107, 128, 4), dtype=torch.float16, device="cuda")
        pp.apply_batch(_dev(src), o, in_format=fmt)
        torch.cuda.synchronize()
        outs.append(o.cpu().numpy())
        pp.close()
    assert outs[0].tobytes() == outs[1].tobytes()
    for i in range(n):  # and each image equals its own single apply (eye i & 1)
        assert outs[0][i].tobytes() == _apply(packed[i], 128, 107, np.float16, eye=i & 1, radius=0.5).tobytes(), i


def test_batch_shared(gpu):
    import torch
    import openvr_fsr_amd as A
    n = 3
    packed = np.stack([_img(50 + i, w=192) for i in range(n)])
    dec = np.stack([packedf.unpack(p) for p in packed])
    outs = []
    for src, fmt in ((packed, A.FORMAT_R11G11B10F), (dec, None)):
        pp = _pp(out_width=256, out_height=107)
        o = torch.zeros((n, 107, 256, 4), dtype=torch.uint8, device="cuda")
        pp.apply_batch(_dev(src), o, in_format=fmt, shared=True)
        torch.cuda.synchronize()
        outs.append(o.cpu().numpy())
        pp.close()
    assert outs[0].tobytes() == outs[1].tobytes()


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_pair_submit(gpu, order):
    import torch
    import openvr_fsr_amd as A
    frames = [(_img(70 + 2 * f), _img(71 + 2 * f)) for f in range(3)]
    res = []
    for decoded in (False, True):
        pp = _pp(pair_submit=1)
        got, paired = [], 0
        for f, (a, b) in enumerate(frames):
            imgs = {0: a, 1: b}
            outs = {}
            for eye in order:
                src = packedf.unpack(imgs[eye]) if decoded else imgs[eye]
                o = torch.zeros((107, 128, 4), dtype=torch.float16, device="cuda")
                t = _dev(src)
                pp.apply(eye, t, out=o, in_format=None if decoded else A.FORMAT_R11G11B10F)
                paired += pp.pair_pending()
                outs[eye] = (o, t)
            torch.cuda.synchronize()
            got.append([outs[e][0].cpu().numpy() for e in (0, 1)])
        pp.close()
        res.append((got, paired))
    assert res[0][1] == res[1][1]   # the packed submissions were recorded and paired as the RGBA16F ones were
    for f in range(len(frames)):
        for e in (0, 1):
            assert res[0][0][f][e].tobytes() == res[1][0][f][e].tobytes(), (f, e)


def test_pair_submit_with_a_format_change_between_the_eyes(gpu):
    """One eye R11G11B10F, the other RGBA16F: a format change un-pairs them (the recorded eye is flushed, the ctx rebuilt), and every
    eye still gets the bytes of its own fresh-ctx apply."""
    import torch
    import openvr_fsr_amd as A
    pp = _pp(pair_submit=1)
    held = []
    for f in range(3):
        for eye in (0, 1):
            packed = _img(80 + 2 * f + eye)
            src = packed if eye == 0 else packedf.unpack(packed)
            o = torch.zeros((107, 128, 4), dtype=torch.float16, device="cuda")
            t = _dev(src)
            pp.apply(eye, t, out=o, in_format=A.FORMAT_R11G11B10F if eye == 0 else None)
            held.append((o, t, packed, eye))
    pp.close()   # (flushes nothing: destroy drops a recorded eye, so the last one is checked only if it was launched)
    torch.cuda.synchronize()
    for o, t, packed, eye in held[:-1]:
        want = _apply(packedf.unpack(packed), 128, 107, np.float16, eye=eye, radius=0.5)
        assert o.cpu().numpy().tobytes() == want.tobytes(), eye


def test_ctx_owned_output(gpu):
    """out->data == NULL: the ctx-owned image an R11G11B10F submission gets is the RGBA16F one of the same values (header)."""
    import torch
    import openvr_fsr_amd as A
    for s in (1, 2):
        packed = _img(s=s)
        pp = _pp()
        got = pp.apply(0, _dev(packed), in_format=A.FORMAT_R11G11B10F)
        torch.cuda.synchronize()
        assert got.dtype == torch.float16 and tuple(got.shape) == (107, 128, 4)
        g = got.cpu().numpy()
        pp.close()
        assert g.tobytes() == _apply(_decoded(packed), 128, 107, np.float16, radius=0.5).tobytes()


# ---- refusals and rebuilds ----------------------------------------------------------------------------------------------------


def _desc(t, fmt, width=None, pitch=None):
    from openvr_fsr_amd import _capi as K
    return K.Image(t.data_ptr(), width if width is not None else t.shape[1], t.shape[0],
                   pitch if pitch is not None else t.stride(0) * t.element_size(), fmt)


def test_refusals_leave_the_ctx_enabled(gpu):
    import ctypes as C
    import torch
    from openvr_fsr_amd import _capi as K
    pp = _pp()
    lib = pp._lib
    packed = _img()
    t = _dev(packed)
    out = torch.zeros((107, 128, 4), dtype=torch.float16, device="cuda")
    ok_out = _desc(out, K.FORMAT_RGBA16F)
    ctx_owned = K.Image()

    def call(img, o=None):
        o = o if o is not None else ok_out
        return lib.ovrfsr_apply(pp._ctx, 0, C.byref(img), None, C.byref(o), pp._stream())

    good = _desc(t, K.FORMAT_R11G11B10F)
    # as an output: single-sample and multisampled
    out_p = torch.zeros((107, 128), dtype=torch.int32, device="cuda")
    assert call(good, _desc(out_p, K.FORMAT_R11G11B10F)) == 2
    out_ms = torch.zeros((107, 128 * 4), dtype=torch.int32, device="cuda")
    assert call(good, _desc(out_ms, K.format_ms(K.FORMAT_R11G11B10F, 4), width=128)) == 2
    assert call(_desc(_dev(packedf.unpack(packed)), K.FORMAT_RGBA16F), _desc(out_p, K.FORMAT_R11G11B10F)) == 2
    # value 5 stays unassigned and refused, and so are 7, 9 and a bad sample count of the new format
    for bad_fmt in (5, K.format_ms(5, 4), 7, 9, K.format_ms(K.FORMAT_R11G11B10F, 3), K.format_ms(K.FORMAT_R11G11B10F, 16), K.FORMAT_R11G11B10F | 1 << 20):
        assert call(_desc(t, bad_fmt)) == 2, hex(bad_fmt)
    # an RGB10A2 destination pairs with RGB10A2 images only: refused as for an RGBA16F input
    assert call(good, _desc(out_p, K.FORMAT_RGB10A2)) == 2
    # a pitch that does not hold the row; a misaligned base; input overlapping the output
    assert call(_desc(t, K.FORMAT_R11G11B10F, pitch=96 * 4 - 4)) == 1
    assert call(K.Image(t.data_ptr() + 2, 95, 80, 96 * 4, K.FORMAT_R11G11B10F)) == 1
    # still enabled: the good call works and matches, into a caller's image and into the ctx-owned one
    assert call(good) == 0
    torch.cuda.synchronize()
    want = _apply(packedf.unpack(packed), 128, 107, np.float16, radius=0.5)
    assert out.cpu().numpy().tobytes() == want.tobytes()
    assert call(good, ctx_owned) == 0 and ctx_owned.format == K.FORMAT_RGBA16F and ctx_owned.data
    pp.close()


def test_overlap_is_checked_against_the_submitted_words(gpu):
    """Sharpen-only, output size == input size: an RGBA16F output that starts inside the submitted 4-byte image is refused; one that
    starts right behind its last row is accepted, although an 8-byte image of that size would reach into it."""
    import ctypes as C
    import torch
    from openvr_fsr_amd import _capi as K
    w, h = 64, 48
    pp = _pp(out_width=w, out_height=h, stage_mask=2)
    buf = torch.zeros(w * h * 4 + w * h * 8 + 64, dtype=torch.uint8, device="cuda")
    packed = _img(w=w, h=h)
    buf[:w * h * 4] = _dev(packed).view(torch.uint8).reshape(-1)
    src = K.Image(buf.data_ptr(), w, h, w * 4, K.FORMAT_R11G11B10F)

    def call(off):
        o = K.Image(buf.data_ptr() + off, w, h, w * 8, K.FORMAT_RGBA16F)
        return pp._lib.ovrfsr_apply(pp._ctx, 0, C.byref(src), None, C.byref(o), pp._stream())

    assert call(w * h * 4 - 8) == 1
    assert call(w * h * 4) == 0
    torch.cuda.synchronize()
    got = buf[w * h * 4:w * h * 12].cpu().numpy().tobytes()
    pp.close()
    assert got == _apply(packedf.unpack(packed), w, h, np.float16, radius=0.5, stage_mask=2).tobytes()


def test_save_refuses_the_format(gpu, tmp_path):
    import ctypes as C
    from openvr_fsr_amd import _capi as K
    lib = K.library()
    t = _dev(_img())
    ms = _dev(_img(s=4))
    cases = [(_desc(t, K.FORMAT_R11G11B10F), 2), (_desc(t, K.format_ms(K.FORMAT_R11G11B10F, 1)), 2),
             (_desc(ms.view(80, 96 * 4), K.format_ms(K.FORMAT_R11G11B10F, 4), width=96), 2),
             # unknown values keep the answers they had: a bare unknown base is an invalid argument, with sample bits unsupported
             (_desc(t, 5), 1), (_desc(t, 7), 1), (_desc(t, 9), 1), (_desc(t, K.format_ms(5, 4)), 2)]
    for img, want in cases:
        assert lib.ovrfsr_save_ppm(C.byref(img), str(tmp_path / "a.ppm").encode(), None) == want, (hex(img.format), want)
        assert lib.ovrfsr_save_dds(C.byref(img), str(tmp_path / "a.dds").encode(), None) == want, (hex(img.format), want)
    assert not (tmp_path / "a.ppm").exists() and not (tmp_path / "a.dds").exists()
    # the ctx of an apply is untouched by a refused save
    assert _apply(_img(), 128, 107, np.float16).shape == (107, 128, 4)


def test_format_changes_rebuild(gpu):
    """R11G11B10F <-> RGBA16F input (and a change of sample count) on one ctx: each call rebuilds and gives its own fresh-ctx bytes."""
    import torch
    import openvr_fsr_amd as A
    pp = _pp()
    base = _img(90, s=4)
    for kind in ("packed", "half", "packed4", "packed", "half"):
        src = {"packed": base[:, :, 0], "half": packedf.unpack(base[:, :, 1]), "packed4": base}[kind]
        out = torch.zeros((107, 128, 4), dtype=torch.float16, device="cuda")
        pp.apply(0, _dev(src), out=out, in_format=None if kind == "half" else A.FORMAT_R11G11B10F)
        torch.cuda.synchronize()
        want = _apply(src if kind == "half" else _decoded(src), 128, 107, np.float16, radius=0.5)
        assert out.cpu().numpy().tobytes() == want.tobytes(), kind
    pp.close()


def test_fsr_disabled_forwards_the_descriptor(gpu):
    import ctypes as C
    import openvr_fsr_amd as A
    from openvr_fsr_amd import _capi as K
    pp = A.PostProcessor(fsr_enabled=0)
    t = _dev(_img(s=4))
    src = _desc(t.view(80, 96 * 4), K.format_ms(K.FORMAT_R11G11B10F, 4), width=96)
    out = K.Image()
    assert pp._lib.ovrfsr_apply(pp._ctx, 0, C.byref(src), None, C.byref(out), pp._stream()) == 0
    assert (out.data, out.width, out.height, out.pitch_bytes, out.format) == (src.data, 96, 80, 96 * 16, 0x406)
    pp.close()


@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_capture(gpu):
    """A first R11G11B10F call under capture must build (the RGBA16F copy, the pipeline): refused, capture intact, ctx enabled.  After one
    call outside, the same call replays from a graph to the same bytes."""
    import torch
    import openvr_fsr_amd as A
    src = _dev(np.stack([_img(95), _img(96)]))
    pp = _pp()
    out = torch.zeros((2, 107, 128, 4), dtype=torch.float16, device="cuda")
    ref = torch.zeros_like(out)
    side = torch.cuda.Stream()

    def capture():
        g = torch.cuda.CUDAGraph()
        side.wait_stream(torch.cuda.current_stream())
        err = None
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                try:
                    pp.apply_batch(src, out, in_format=A.FORMAT_R11G11B10F)
                except A.OvrFsrError as e:
                    err = e
        torch.cuda.synchronize()
        return g, err

    g, err = capture()
    assert err is not None and err.status == 1, err
    pp.apply_batch(src, ref, in_format=A.FORMAT_R11G11B10F)
    torch.cuda.synchronize()
    g, err = capture()
    assert err is None
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    pp.close()


# ---- checked build ------------------------------------------------------------------------------------------------------------

_CHILD = r"""
import ctypes, sys
sys.path.insert(0, %r)
import openvr_fsr_amd as A
from tests import test_gpu_packed_float as T
lib = A.library()
n = lib.ovrfsr_debug_bounds_slots()
buf = (ctypes.c_ulonglong * n)()
lib.ovrfsr_debug_bounds.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.c_int]
assert lib.ovrfsr_debug_bounds(buf, n, 1) == 0
bad, launched = [], 0
for s in (1, 2, 4, 8):
    r, l, b = T.matrix(s, T.SOURCES[:3] + T.SOURCES[4:])
    bad += b
    launched += l
import torch; torch.cuda.synchronize()
assert lib.ovrfsr_debug_bounds(buf, n, 0) == 0
nk = (n - 5) // 3
v = list(buf)
print("R11G11B10F checked: launched %%d, mismatches %%d, checked %%d, out of bounds %%d" %% (launched, len(bad), sum(v[2 * nk:3 * nk]), sum(v[:nk])))
"""


def test_checked_build_matrix(gpu):
    """The equality matrix at its small sizes against the -DOVRFSR_BOUNDS build: every access of the unpack kernels (and of everything
    behind them) through the checked accessors, 0 violations."""
    from tests.variants import variant
    lib = variant("bounds", "-DOVRFSR_BOUNDS")
    env = dict(os.environ, OVRFSR_LIB=lib, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    import re
    m = re.search(r"R11G11B10F checked: launched (\d+), mismatches (\d+), checked (\d+), out of bounds (\d+)", r.stdout)
    assert r.returncode == 0 and m, (r.stdout[-1500:], r.stderr[-1500:])
    assert int(m.group(1)) > 100 and int(m.group(2)) == 0 and int(m.group(3)) > 1e6 and int(m.group(4)) == 0, m.group(0)
