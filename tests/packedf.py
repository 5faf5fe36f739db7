"""R11G11B10F inputs (OVRFSR_FORMAT_R11G11B10F): the header's decode rule restated in numpy from the DXGI format definition, and packed
images built from the single-sample content generators.  One uint32 word per texel (held as int32, as torch has no uint32 images): R in
bits 0-10, G in bits 11-21, B in bits 22-31; each channel an unsigned float with a 5-bit exponent of bias 15 and a 6-bit (R, G) or
5-bit (B) mantissa.  A single-sample image is [H, W] int32, a multisampled one [H, W, S] int32 (samples interleaved per texel)."""
import numpy as np

from tests import msaa

SAMPLES = (1, 2, 4, 8)
MAX_RG, MAX_B = 65024.0, 64512.0  # largest finite values: (1 + 63/64) * 2^15, (1 + 31/32) * 2^15


def value_of(code, mbits):
    """The value of one channel code by the format's definition: exponent 0 -> m / 2^mbits * 2^-14; exponent 31 -> +Inf (m = 0) or NaN;
    otherwise (1 + m / 2^mbits) * 2^(e - 15).  float64, exact."""
    code = np.asarray(code, np.uint32)
    e = (code >> mbits).astype(np.int64)
    m = (code & ((1 << mbits) - 1)).astype(np.float64)
    den = float(1 << mbits)
    sub = m / den * 2.0 ** -14
    nrm = (1.0 + m / den) * np.exp2((e - 15).astype(np.float64))
    out = np.where(e == 0, sub, nrm)
    out = np.where(e == 31, np.where(m == 0, np.inf, np.nan), out)
    return out


def channels(packed):
    """packed words -> (R, G, B) channel codes (11, 11 and 10 bits)"""
    u = np.ascontiguousarray(packed).view(np.uint32)
    return u & 0x7FF, (u >> 11) & 0x7FF, u >> 22


def pack(r, g, b):
    """channel codes -> packed words (int32)"""
    r, g, b = (np.asarray(c, np.uint32) for c in (r, g, b))
    assert (r < 2048).all() and (g < 2048).all() and (b < 1024).all()
    return np.ascontiguousarray(r | (g << 11) | (b << 22)).view(np.int32)


def unpack(packed):
    """The decode rule: [...] packed words -> [..., 4] float16, each channel the half float whose bits are the channel's bits shifted
    left by 4 (R, G) or 5 (B); alpha 1.0."""
    r, g, b = channels(packed)
    out = np.empty(np.shape(packed) + (4,), np.uint16)
    out[..., 0] = r << 4
    out[..., 1] = g << 4
    out[..., 2] = b << 5
    out[..., 3] = 0x3C00
    return out.view(np.float16)


def encode(f):
    """[..., >= 3] non-negative floats -> packed words, every channel TRUNCATED to its code (the half float's low mantissa bits dropped,
    values past the largest finite one clamped to it): a way to make content, not a rounding rule of the library (the format is
    input-only)."""
    h = np.asarray(f, np.float32)[..., :3]
    assert (h >= 0).all()
    hb = np.minimum(h, np.float32(65504)).astype(np.float16).view(np.uint16).astype(np.uint32)
    r = np.minimum(hb[..., 0] >> 4, 0x7BF)
    g = np.minimum(hb[..., 1] >> 4, 0x7BF)
    b = np.minimum(hb[..., 2] >> 5, 0x3DF)
    return pack(r, g, b)


def resolve(ms):
    """[..., S] packed samples -> [..., 4] float16: the float resolve rule (fp32 sum in sample order, times 1/S, half rounded to nearest
    even) on the decoded samples.  S = 1 is the plain decode."""
    dec = unpack(ms)  # [..., S, 4]
    return dec[..., 0, :].copy() if ms.shape[-1] == 1 else msaa.resolve_float(dec)


def from_u8(u8, scale=1.0):
    """a uint8 [..., 4] image -> packed words of value u8 / 255 * scale"""
    return encode(u8.astype(np.float32) / np.float32(255) * np.float32(scale))


def make(w, h, content, seed, scale=1.0):
    """a single-sample packed image [h, w] of the content generators' texels"""
    return from_u8(msaa._base_u8(w, h, seed, content), scale)


def make_ms(w, h, s, content, seed, scale=1.0):
    """an S-sample packed image [h, w, s]: tests/msaa.py's sample sets (every sample the texel moved by its own noise), packed"""
    return from_u8(msaa.make_ms(w, h, s, "rgba8", content, seed), scale)
