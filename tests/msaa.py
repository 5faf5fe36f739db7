"""Multisampled inputs (OVRFSR_FORMAT_MS): the header's resolve rule restated in numpy, and sample sets built from the single-sample
content generators.  Samples are interleaved per texel: a uint8 / half / float image is [H, W, S, 4], an R10G10B10A2 one [H, W, S] int32."""
import numpy as np

from tests import natural, synth

FORMATS = ("rgba8", "bgra8", "rgba16f", "rgba32f", "rgb10a2")
SAMPLES = (2, 4, 8)


def _log2(s):
    assert s in SAMPLES, s
    return {2: 1, 4: 2, 8: 3}[s]


def resolve_unorm8(ms):
    """[..., S, 4] uint8 -> [..., 4] uint8: (sum + S/2) >> log2 S per channel."""
    s = ms.shape[-2]
    return ((ms.astype(np.uint32).sum(axis=-2) + s // 2) >> _log2(s)).astype(np.uint8)


def resolve_bgra8(ms):
    """B,G,R,A samples -> the resolved texel in R,G,B,A order (what the pipeline behind the resolve reads)."""
    return np.ascontiguousarray(resolve_unorm8(ms)[..., [2, 1, 0, 3]])


def resolve_rgb10a2(ms):
    """[..., S] packed int32 (R 0-9, G 10-19, B 20-29, A 30-31) -> [...] int32, the same rule per 10 / 2-bit channel."""
    s = ms.shape[-1]
    v = np.ascontiguousarray(ms).view(np.uint32).astype(np.uint64)
    out = np.zeros(ms.shape[:-1], np.uint64)
    for shift, mask in ((0, 1023), (10, 1023), (20, 1023), (30, 3)):
        c = (((v >> shift) & mask).sum(axis=-1) + s // 2) >> _log2(s)
        out |= c << shift
    return out.astype(np.uint32).view(np.int32)


def resolve_float(ms):
    """[..., S, 4] float16 / float32: fp32 sum in sample order s0 + s1 + ..., times 1/S, back to the input's type (half: nearest even)."""
    s = ms.shape[-2]
    f = ms.astype(np.float32)
    acc = f[..., 0, :].copy()
    for i in range(1, s):
        acc = (acc + f[..., i, :]).astype(np.float32)
    acc = (acc * np.float32(1.0 / s)).astype(np.float32)
    return acc.astype(ms.dtype)


def resolve(ms, fmt):
    return {"rgba8": resolve_unorm8, "bgra8": resolve_bgra8, "rgba16f": resolve_float, "rgba32f": resolve_float,
            "rgb10a2": resolve_rgb10a2}[fmt](ms)


def _base_u8(w, h, seed, content):
    if content == "structured":
        return synth.structured_u8(w, h, seed)
    if content == "random":
        return synth.random_u8(w, h, seed)
    if content == "natural":
        return natural.tiled_u8(w, h, seed)
    raise ValueError(content)


def make_ms(w, h, s, fmt, content, seed):
    """An S-sample image of format `fmt`: every sample is the content's texel moved by its own noise (uniform-random content: every
    sample drawn on its own), so that the resolve has something to average and ties to round."""
    rng = np.random.default_rng(seed)
    if content == "random":
        u8 = np.stack([synth.random_u8(w, h, seed * 16 + i) for i in range(s)], axis=2)
    else:
        base = _base_u8(w, h, seed, content).astype(np.int16)[:, :, None, :]
        u8 = np.clip(base + rng.integers(-24, 25, (h, w, s, 4)), 0, 255).astype(np.uint8)
    if fmt in ("rgba8", "bgra8"):
        return u8
    if fmt == "rgba16f":
        f = u8.astype(np.float32) / np.float32(255) + rng.uniform(-1e-3, 1e-3, u8.shape).astype(np.float32)
        return f.astype(np.float16)
    if fmt == "rgba32f":
        return (u8.astype(np.float32) / np.float32(255) + rng.uniform(-1e-3, 1e-3, u8.shape).astype(np.float32)).astype(np.float32)
    if fmt == "rgb10a2":
        q = np.clip(u8.astype(np.uint32) * 4 + rng.integers(0, 4, u8.shape), 0, 1023).astype(np.uint32)
        a = (u8[..., 3].astype(np.uint32) >> 6)
        return (q[..., 0] | (q[..., 1] << 10) | (q[..., 2] << 20) | (a << 30)).view(np.int32)
    raise ValueError(fmt)
