"""NVScaler / NVSharpen on float eye images: the cases tests/test_oracle_nis.py pins to the reference on the CPU and
tests/test_gpu_nis_formats.py then runs through the HIP kernels -- one list of shapes and content kinds, one way to ask the oracle."""
import numpy as np

from oracle import oracle as O
from tests import synth

# pitch 32 with a ragged edge; 2x; pitch 40; odd sizes
SHAPES = [(96, 80, 128, 107), (50, 40, 100, 80), (40, 33, 41, 34), (61, 47, 80, 63)]
# kind -> scale (synth.hdr_f32).  NOT a uniformly scaled bright image: NIS clamps every output to [0, 1], and 88-95 % of the oracle's
# colour values for base x 6 are exactly 1.0 -- a comparison on it passes whatever the kernel computes.
KINDS = {"unit": 1.0, "highlights": 40.0, "signed": 4.0}
PROJ = (0.45, 0.5, 0.55, 0.5)
SEED = 7
MIN_INSIDE = 0.25


def image(kind, w, h, seed=SEED):
    return synth.hdr_f32(w, h, seed, KINDS[kind], kind)


def inside_share(want):
    """share of an oracle output's colour values strictly inside (0, 1): the ones a comparison can learn something from"""
    c = np.asarray(want, np.float32)[..., :3]
    return float(((c > 0) & (c < 1)).mean())


def assert_informative(want, what=""):
    """a condition on the INPUTS of a comparison, checked on the oracle's output, never on the kernel's"""
    s = inside_share(want)
    assert s >= MIN_INSIDE, "only %.3f of the oracle's colour values lie inside (0, 1): %s says little" % (s, what)


def want_scaler(img, ow, oh, sharpness, radius=2.0, proj=(0.5,) * 4, eye=0, debug=0, tables=None, config=None):
    """the oracle's NVScaler output; tables / config default to the product's own (A.nis_coefs, A.nis_scaler_config)"""
    import openvr_fsr_amd as A
    ih, iw = img.shape[:2]
    cs, cu = tables if tables is not None else A.nis_coefs()
    ok, cfg = (config or A.nis_scaler_config)(sharpness, iw, ih, ow, oh)
    assert ok
    centre, rad = O.mask_constants(ow, oh, radius, proj, True, eye)
    return O.nis_upscale(img, ow, oh, O.nis_block(cfg, centre, rad, debug), cs, cu)


def want_sharpen(img, sharpness, radius=2.0, proj=(0.5,) * 4, eye=0, debug=0):
    """the oracle's NVSharpen output (render scale 1: the image's own size)"""
    import openvr_fsr_amd as A
    h, w = img.shape[:2]
    ok, cfg = A.nis_sharpen_config(sharpness, w, h)
    assert ok
    centre, rad = O.mask_constants(w, h, radius, proj, True, eye)
    return O.nis_sharpen(img, O.nis_block(cfg, centre, rad, debug))
