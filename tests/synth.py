"""Deterministic synthetic eye images: low-frequency sinusoid gradient + 45/135 degree
hard edges + +-4/255 uniform noise + a constant block, alpha = 255; and a uniform-random variant.
Seed convention: 0x5EED0000 + 2*pair + eye."""
import numpy as np


def seed_for(pair, eye):
    return 0x5EED0000 + 2 * pair + eye


def structured_u8(w, h, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    ph = rng.uniform(0, 6.28, 3).astype(np.float32)
    img = np.ones((h, w, 4), np.float32)
    for c in range(3):
        img[..., c] = 0.5 + 0.35 * np.sin(x * (0.011 + 0.004 * c) + ph[c]) * np.cos(y * (0.008 + 0.003 * c) - ph[c])
    period = max(16, min(w, h) // 6)
    d45 = ((x + y) % period) < (period / 2)
    d135 = ((x - y) % (period * 1.5)) < (period * 0.5)
    img[..., 0] = np.where(d45, img[..., 0] * 0.35, img[..., 0])
    img[..., 1] = np.where(d135, 1.0 - img[..., 1] * 0.5, img[..., 1])
    img[..., 2] = np.where(d45 & d135, 0.95, img[..., 2])
    noise = rng.integers(-4, 5, size=(h, w, 3)).astype(np.float32) / 255.0
    img[..., :3] += noise
    by, bx = h // 3, w // 3
    img[by:by + max(4, h // 8), bx:bx + max(4, w // 8), :3] = np.array([0.25, 0.5, 0.75], np.float32)
    out = np.clip(np.floor(img * 255.0 + 0.5), 0, 255).astype(np.uint8)
    out[..., 3] = 255
    return out


def random_u8(w, h, seed):
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    out[..., 3] = 255
    return out


def extremes_u8(w, h, seed):
    """Only 0 / 255 / a few mid values: exercises RCAS's 0*inf NaN paths and EASU's zero-gradient guard."""
    rng = np.random.default_rng(seed)
    vals = np.array([0, 0, 255, 255, 1, 254, 128], np.uint8)
    out = vals[rng.integers(0, len(vals), size=(h, w, 4))]
    blk = max(2, min(w, h) // 4)
    out[:blk, :blk, :3] = 0
    out[-blk:, -blk:, :3] = 255
    out[..., 3] = 255
    return out


FLAT_RECT = (0, 8, 72, 12)   # x, y, width, height of hdr_f32's noise-free constant rectangle
FLAT_UNIT, FLAT_SIGNED = (0.25, 0.5, 0.75), (-0.5, 0.5, 1.5)   # its colour: kinds "unit" / "highlights", kind "signed"


def hdr_f32(w, h, seed, scale, kind):
    """float32 RGBA eye image for the float formats, alpha 1.0, every texel exactly representable in half (one image serves as an
    RGBA16F and as an RGBA32F submission), built on structured_u8(w, h, seed) / 255:
      "unit"        the base as it is
      "highlights"  the base with 2 % of the texels set to scale * U(0.5, 1) per colour channel (taps tens of times their neighbours)
      "signed"      (base - 0.5) * scale: negative values and values above 1 in every neighbourhood
    Images that can hold it (w >= 72, h >= 20) carry one noise-free constant rectangle, FLAT_RECT: an aligned 32 x 2 span of pixels
    inside it has a flat 5 x 5 neighbourhood, which is what NVSharpen's wave-uniform no-edge shortcut needs to run.  Its colour is
    FLAT_UNIT, and for "signed" FLAT_SIGNED: values outside [0, 1] in the one place certain to take that shortcut."""
    base = structured_u8(w, h, seed).astype(np.float32) / np.float32(255)
    if kind == "unit":
        img = base
    elif kind == "highlights":
        rng = np.random.default_rng(seed)
        img = base.copy()
        hot = rng.random((h, w)) < 0.02
        img[hot, :3] = np.float32(scale) * rng.uniform(0.5, 1.0, (int(hot.sum()), 3)).astype(np.float32)
    elif kind == "signed":
        img = (base - np.float32(0.5)) * np.float32(scale)
    else:
        raise ValueError(kind)
    rx, ry, rw, rh = FLAT_RECT
    if w >= rx + rw and h >= ry + rh:
        # "signed": one channel below 0 and one above 1, so that the clamp of the shortcut's own store is exercised too
        img[ry:ry + rh, rx:rx + rw, :3] = np.array(FLAT_SIGNED if kind == "signed" else FLAT_UNIT, np.float32)
    img = img.astype(np.float16).astype(np.float32)
    img[..., 3] = 1.0
    return img


WILD_FINITE = ("half extremes, non-negative", "half extremes, negative values, no zeros", "up to 1e18, denormals, zeros", "zeros of both signs")
WILD_KINDS = WILD_FINITE + ("NaN / Inf / 1e30",)


def wild_f32(kind, w, h, rng):
    """float32 RGBA texels far from a colour image (WILD_KINDS; all but the last are finite)"""
    if kind == "half extremes, non-negative":
        img = rng.choice(np.array([65504.0, 6e-8, 0.0, 1.0, 1e-3, 3e4, 2.5, 0.5], np.float32), size=(h, w, 4))
    elif kind == "half extremes, negative values, no zeros":
        img = rng.choice(np.array([65504.0, -65504.0, 6e-8, -6e-8, 1.0, 1e-3, 3e4, -2.5], np.float32), size=(h, w, 4))
    elif kind == "zeros of both signs":
        img = rng.choice(np.array([65504.0, 0.0, -0.0, 1.0, 1e-3, 3e4, 2.5], np.float32), size=(h, w, 4))
    else:
        img = rng.standard_normal((h, w, 4)).astype(np.float32) * np.float32(10.0 ** rng.uniform(-3, 3))
        sel = rng.random((h, w, 4))
        img[sel < 0.05] = 0.0
        img[(sel >= 0.05) & (sel < 0.08)] = np.float32(1e-41)                      # fp32 denormals
        if kind == "up to 1e18, denormals, zeros":
            img *= np.float32(1e18 / float(np.abs(img).max()))
        if kind == "NaN / Inf / 1e30":
            img[(sel >= 0.08) & (sel < 0.10)] = np.float32(1e30)
            img[(sel >= 0.10) & (sel < 0.12)] = np.float32(-1e30)
            img[(sel >= 0.12) & (sel < 0.13)] = np.nan
            img[(sel >= 0.13) & (sel < 0.14)] = np.inf
            img[(sel >= 0.14) & (sel < 0.15)] = -np.inf
    img = np.ascontiguousarray(img, np.float32)
    img[..., 3] = 1.0
    return img
