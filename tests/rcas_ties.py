"""The tie-rich RCAS fixture of the exact-stores tests: a small RGBA8 image most of whose RCAS results (sharpness 0.9) land on, or within
2^-15 byte of, a UNORM8 rounding boundary k + 1/2 -- the pixels where the product build's arithmetic and rounding can store another byte than
the strict build, and where OVRFSR_PRECISION_FP32_EXACT has to re-evaluate.

Built from a seed with the oracle: RCAS over a 768 x 768 uniform-random image, the interior pixels with a channel of sat(out) * 255 (fp32)
within 2^-15 byte of a boundary harvested, and each one's 3 x 3 neighbourhood copied onto a stride-3 grid of a 96 x 96 image of other random
bytes.  RCAS reads only the five taps of the cross, so neighbourhoods next to each other do not disturb each other's centre pixel.  A plain
random image has 0.06 % of its pixels within 2^-13 byte; a smooth ramp has none."""
import functools

import numpy as np

from oracle import oracle as O

SHARP = 0.9
SIZE = 96          # the fixture: 96 x 96, two 62-column cells of rcas_dpp_kernel wide, the second partial
SOURCE = 768


def near(outf, bits):
    """[H, W] bool: a colour channel of sat(out) * 255, evaluated in fp32 as the store evaluates it, within 2^-bits byte of k + 1/2"""
    v = np.clip(outf[..., :3], np.float32(0), np.float32(1)) * np.float32(255)
    return (np.abs((v - np.floor(v)) - np.float32(0.5)) <= np.float32(2.0 ** -bits)).any(axis=2)


def rcas_f32(img8, sharp=SHARP):
    centre, rad = O.mask_constants(img8.shape[1], img8.shape[0])
    return O.rcas(O.unorm8_to_float(img8), O.rcas_con(sharp), centre, rad)


@functools.lru_cache(maxsize=4)
def fixture(seed=7):
    """(image uint8 [96, 96, 4], neighbourhoods harvested, pixels within 2^-15 byte, pixels within 2^-13 byte).  Treat the image as read-only."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, (SOURCE, SOURCE, 4), dtype=np.uint8)
    src[..., 3] = 255
    hit = near(rcas_f32(src), 15)
    hit[0, :] = hit[-1, :] = False
    hit[:, 0] = hit[:, -1] = False
    ys, xs = np.nonzero(hit)
    img = rng.integers(0, 256, (SIZE, SIZE, 4), dtype=np.uint8)
    img[..., 3] = 255
    slots = (SIZE // 3) * (SIZE // 3)
    n = min(len(ys), slots)
    for k in range(n):
        gy, gx = divmod(k, SIZE // 3)
        img[3 * gy:3 * gy + 3, 3 * gx:3 * gx + 3] = src[ys[k] - 1:ys[k] + 2, xs[k] - 1:xs[k] + 2]
    out = rcas_f32(img)
    n15, n13 = int(near(out, 15).sum()), int(near(out, 13).sum())
    assert n15 >= 50, "the fixture holds %d near-tie pixels (seed %d): too few to test anything" % (n15, seed)
    img.setflags(write=False)
    return img, n, n15, n13
