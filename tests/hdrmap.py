"""The mapping of OVRFSR_HDR_DOMAIN_SRTM (include/openvr_fsr_amd.h, "HDR domain") restated in numpy: float32 arithmetic, one rounding per
operator, as the header writes it.  forward / back take [..., >= 3] float32 arrays and map the first three channels; alpha, where there
is one, passes through.  to_dest is the back pass's store conversion."""
import numpy as np

ONE = np.float32(1.0)
FLOOR = ONE / np.float32(32768.0)   # the clamp of the back mapping's divisor


def _scaled(x, k):
    out = np.array(x, np.float32, copy=True)
    out[..., :3] = out[..., :3] * k[..., None]
    return out


def forward(x):
    """k = 1 / (max3 + 1); rgb *= k"""
    x = np.asarray(x, np.float32)
    m = np.maximum(np.maximum(x[..., 0], x[..., 1]), x[..., 2])
    with np.errstate(all="ignore"):
        return _scaled(x, ONE / (m + ONE))


def back(x):
    """k = 1 / max(1 / 32768, 1 - max3); rgb *= k"""
    x = np.asarray(x, np.float32)
    m = np.maximum(np.maximum(x[..., 0], x[..., 1]), x[..., 2])
    with np.errstate(all="ignore"):
        return _scaled(x, ONE / np.maximum(FLOOR, ONE - m))


def to_dest(x, dtype, float_to_unorm8=None):
    """[H, W, 4] float32 -> the destination's texels: float32 as is, float16 rounded to nearest even, uint8 through ``float_to_unorm8``
    (oracle.float_to_unorm8: saturate, x 255, + 0.5, truncate)"""
    x = np.asarray(x, np.float32)
    if dtype == np.float32:
        return x
    if dtype == np.float16:
        with np.errstate(over="ignore"):
            return x.astype(np.float16)
    assert dtype == np.uint8 and float_to_unorm8 is not None
    return float_to_unorm8(x)
