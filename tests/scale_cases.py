"""The per-axis scale regimes of the EASU kernels: one smallest shape per regime, and the footprint rule they are chosen by restated ONCE in
numpy -- what tests/test_scale_regimes.py (planner, CPU) and tests/test_gpu_scale_regimes.py (pixels, GPU) share.  No GPU, no library.

The rule, from the ORACLE's easu_con words (s = con[0] / con[1], c = con[2] / con[3] per axis): output pixel o samples about the texel
f(o) = floor(fl32(fl32(o * s) + c)) and reads the taps f - 1 .. f + 2.  A 32-pixel tile therefore stages f(last) - f(first) + 4 cells per
axis, the largest value over the tiles of the image.  For heights the last pixel is the partner row `| 1` of the last row pair (the product
kernel evaluates it even behind the image); the fused kernel runs EASU on the tile plus a one-pixel ring: f(min(o0 + 32, n - 1)) -
f(o0 - 1) + 4.  The width picks the kernel (csrc/fsr_sizes.h): up to 28 / 32 / 40 cells the fixed-pitch fast kernel, beyond 40 the
generic one whose pitch is the width itself.  The LDS byte formulas below are those of fsr_sizes.h; a plan is accepted where they give at
most 64 KiB (fused: 158 KiB and at most 40 cells across).  The row-pair step of the pair resolve is f(o + 1) - f(o) over even o.

Each case names its class; class_property(case) asserts, from the restatement alone, that the case still belongs to it -- at its own
shape and at the doubled shape the masked forms use (at least 3 x 3 tiles) -- so that a later edit of a shape cannot silently leave its
regime.  tests/test_scale_regimes.py confirms every figure through the planner probe."""
import numpy as np

from oracle import oracle as O

F32 = np.float32
TILE = 32
LDS_MAX, FUSED_LDS_MAX = 64 * 1024, 158 * 1024          # what one workgroup may use; csrc/fsr_params.h kFusedLdsMax
LUM_PAD_ROWS, FUSED_TIE_LIST_BYTES = 5, 4 * 5 * 64 * 2  # csrc/fsr_params.h kLumPadRows, kFusedTieListBytes
REFUSED_LDS = (2, "scale ratio needs more LDS than one tile may use")
REFUSED_FUSED = (2, "fused kernel: tile footprint does not fit LDS at this scale")
REFUSED_NIS = (2, "NIS scales 1x..2x only (NVScalerUpdateConfig returned false)")
RGBA8, RGBA16F, RGBA32F = "rgba8", "rgba16f", "rgba32f"
MASK_RADIUS, MASK_PROJ = 0.5, (0.42, 0.55, 0.61, 0.47)  # the masked forms: radius 0.5, unequal eye centres


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def _con(shape):
    iw, ih, ow, oh = shape
    con = O.easu_con(iw, ih, ow, oh).view(F32)
    return (con[0], con[2]), (con[1], con[3])    # (s, c) of x, of y


def texel(o, sc):
    """f(o) for an array of output coordinates: two float32 roundings, then floor"""
    s, c = sc
    t = (np.asarray(o, F32) * F32(s)).astype(F32)
    return np.floor((t + F32(c)).astype(F32)).astype(np.int64)


def cells(n, sc, pairs):
    o0 = np.arange(0, n, TILE)
    o1 = np.minimum(o0 + TILE - 1, n - 1)
    if pairs:
        o1 = o1 | 1
    return int((texel(o1, sc) - texel(o0, sc) + 4).max())


def fused_cells(n, sc):
    o0 = np.arange(0, n, TILE)
    o1 = np.minimum(o0 + TILE, n - 1)
    return int((texel(o1, sc) - texel(o0 - 1, sc) + 4).max())


def footprint(shape):
    """(cellsW, cellsH, fusedCellsW, fusedCellsH)"""
    x, y = _con(shape)
    return cells(shape[2], x, False), cells(shape[3], y, True), fused_cells(shape[2], x), fused_cells(shape[3], y)


def pair_steps(shape):
    """the set of f(o + 1) - f(o) over the row pairs (o even; the partner of the last pair may lie behind the image)"""
    o = np.arange(0, shape[3], 2)
    return set((texel(o + 1, _con(shape)[1]) - texel(o, _con(shape)[1])).tolist())


def fast_pitch(cw):
    return 32 if cw <= 32 else 40 if cw <= 40 else 0


def kernel_pitch(cw):
    """the LDS pitch of the EASU kernel a two-kernel form launches; 0: the generic kernel, pitch = cellsW"""
    return 28 if cw <= 28 else fast_pitch(cw)


def easu_lds_bytes(strict, src, cw, ch):
    if not strict and fast_pitch(cw):
        return fast_pitch(cw) * ch * (16 + 16 + 4) + fast_pitch(cw) * LUM_PAD_ROWS * 4
    wide = strict or src == RGBA32F
    n = cw * ch
    return ((n * (16 if wide else 8) + 15) & ~15) + n * 16 + n * 4


def fused_lds_bytes(strict, src, cw, ch):
    e = (easu_lds_bytes(strict, src, cw, ch) + 15) & ~15
    if not strict and fast_pitch(cw) and fast_pitch(cw) * ch * 4 < FUSED_TIE_LIST_BYTES:
        e += FUSED_TIE_LIST_BYTES
    return e + (TILE + 2) * (TILE + 2) * 16


def accepted(shape, strict=False, src=RGBA8):
    cw, ch, _, _ = footprint(shape)
    return easu_lds_bytes(strict, src, cw, ch) <= LDS_MAX


def fused_accepted(shape, strict=False, src=RGBA8):
    _, _, fw, fh = footprint(shape)
    return accepted(shape, strict, src) and (strict or fw <= 40) and fused_lds_bytes(strict, src, fw, fh) <= FUSED_LDS_MAX


def staged_outside(shape):
    """csrc/fsr_sizes.h outside_staged_ok for an RGBA8 source: no axis minifies"""
    iw, ih, ow, oh = shape
    return iw <= ow and ih <= oh


def nis_accepted(shape):
    iw, ih, ow, oh = shape
    kx, ky = F32(iw) / F32(ow), F32(ih) / F32(oh)
    return bool(F32(0.5) <= kx <= F32(1) and F32(0.5) <= ky <= F32(1))


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
class Case:
    """id; class; in -> out; the table's cells W x H; the EASU kernel's pitch (0: generic); the row-pair steps; staged outside kernel;
    product: the source formats the product build plans; strict: does the strict build plan; fused: does `fused = 1` plan (product, RGBA8)"""

    def __init__(self, cid, klass, shape, cells_wh, pitch, steps, staged, product, strict, fused):
        self.id, self.klass, self.shape, self.cells, self.pitch, self.steps = cid, klass, shape, cells_wh, pitch, set(steps)
        self.staged, self.product, self.strict, self.fused = staged, set(product), strict, fused

    @property
    def masked_shape(self):
        """the same ratios at an output of at least 3 x 3 tiles: all four numbers doubled"""
        return tuple(2 * v for v in self.shape)

    def plans(self, src=RGBA8, strict=False):
        return self.strict if strict else src in self.product


ALL, BYTE_HALF, NONE = (RGBA8, RGBA16F, RGBA32F), (RGBA8, RGBA16F), ()
CASES = [
    #    id                  class           in -> out              cells      pitch steps  staged product    strict fused
    Case("steep-8x",         "steep",        (8, 6, 64, 48),        (8, 8),    28, {0},     True,  ALL,       True,  True),
    Case("steep-6x-ragged",  "steep",        (12, 10, 67, 61),      (10, 9),   28, {0, 1},  True,  ALL,       True,  True),
    Case("steep-3x",         "steep",        (21, 17, 64, 52),      (14, 14),  28, {0, 1},  True,  ALL,       True,  True),
    Case("aniso-3x-1.1x",    "aniso-tall",   (30, 60, 90, 66),      (15, 33),  28, {0, 1},  True,  ALL,       True,  True),
    Case("aniso-1.1x-3x",    "aniso-wide",   (60, 30, 66, 90),      (33, 15),  40, {0, 1},  True,  ALL,       True,  True),
    Case("x-1to1",           "one-to-one-x", (64, 40, 64, 80),      (35, 20),  40, {1},     True,  ALL,       True,  True),
    Case("y-1to1",           "one-to-one-y", (40, 64, 80, 64),      (20, 35),  28, {1},     True,  ALL,       True,  True),
    Case("tall-32",          "tall",         (64, 70, 80, 64),      (29, 37),  32, {1, 2},  False, ALL,       True,  True),
    Case("tall-32-deep",     "tall",         (64, 90, 80, 64),      (29, 47),  32, {1, 2},  False, ALL,       True,  True),
    Case("tall-28-limit",    "tall-limit",   (40, 100, 64, 64),     (24, 52),  28, {1, 2},  False, ALL,       True,  True),
    Case("xmin-40",          "x-minify",     (72, 60, 64, 66),      (38, 33),  40, {0, 1},  False, ALL,       True,  False),
    Case("xmin-40-b",        "x-minify",     (110, 64, 100, 80),    (38, 29),  40, {0, 1},  False, ALL,       True,  False),
    Case("wide-47",          "wide",         (90, 64, 64, 80),      (47, 29),  0,  {0, 1},  False, ALL,       True,  False),
    Case("wide-72",          "wide-64",      (140, 40, 64, 80),     (72, 20),  0,  {1},     False, ALL,       True,  False),
    Case("wide-100",         "wide-64",      (200, 30, 64, 90),     (100, 15), 0,  {0, 1},  False, ALL,       True,  False),
    Case("iso-min-46",       "iso-minify",   (88, 88, 64, 64),      (46, 46),  0,  {1, 2},  False, BYTE_HALF, False, False),
    Case("iso-min-47",       "iso-minify",   (90, 90, 64, 64),      (47, 47),  0,  {1, 2},  False, BYTE_HALF, False, False),
    Case("refuse-tall-28",   "refuse-tall",  (40, 110, 64, 64),     (24, 57),  28, {1, 2},  False, NONE,      True,  False),
    Case("refuse-tall-40",   "refuse-tall",  (70, 100, 77, 64),     (33, 52),  40, {1, 2},  False, NONE,      True,  False),
    Case("refuse-iso-1.5",   "refuse-iso",   (96, 96, 64, 64),      (50, 50),  0,  {1},     False, NONE,      False, False),
    Case("refuse-iso-2",     "refuse-iso",   (128, 128, 64, 64),    (66, 66),  0,  {2},     False, NONE,      False, False),
]
BY_ID = {c.id: c for c in CASES}
CLASSES = {"steep", "aniso-tall", "aniso-wide", "one-to-one-x", "one-to-one-y", "tall", "tall-limit", "x-minify", "wide", "wide-64", "iso-minify",
           "refuse-tall", "refuse-iso"}
ACCEPTED = [c for c in CASES if c.product]                      # the product build plans an RGBA8 source
STRICT_ACCEPTED = [c for c in CASES if c.strict]
GPU_CASES = [c for c in CASES if c.product or c.strict]
HALF_IDS = ["steep-3x", "x-1to1", "tall-32", "tall-28-limit", "wide-72", "iso-min-46"]
PITCHED_IDS = [c.id for c in ACCEPTED if c.id.startswith(("tall-", "wide-"))]

# NVScaler: its own 32 x 24 groups and pitches; NVScalerUpdateConfig accepts all six
NIS_SHAPES = [(64, 40, 64, 80), (40, 64, 80, 64), (50, 60, 90, 66), (60, 50, 66, 90), (32, 24, 64, 48), (63, 47, 64, 48)]


def ratio(case):
    iw, ih, ow, oh = case.shape
    return ow / iw, oh / ih


def class_property(case):
    """asserts what the case is in the table FOR, from the restatement alone, at its shape and at the doubled shape of the masked forms"""
    k = case.klass
    assert k in CLASSES, (case.id, k)
    assert footprint(case.shape)[:2] == case.cells, (case.id, footprint(case.shape))
    rx, ry = ratio(case)
    for shape in (case.shape, case.masked_shape):
        cw, ch, fw, fh = footprint(shape)
        where = (case.id, shape, cw, ch, fw, fh)
        steps = pair_steps(shape)
        # the table's columns: kernel, row-pair steps, outside kernel, who plans it
        assert kernel_pitch(cw) == case.pitch, where
        assert steps == case.steps, where + (steps,)
        assert staged_outside(shape) == case.staged, where
        for src in ALL:
            assert accepted(shape, False, src) == (src in case.product), where + (src, easu_lds_bytes(False, src, cw, ch))
        assert accepted(shape, True) == case.strict, where + (easu_lds_bytes(True, RGBA8, cw, ch),)
        assert fused_accepted(shape) == case.fused, where + (fused_lds_bytes(False, RGBA8, fw, fh),)
        if case.product:
            assert fused_accepted(shape, False, RGBA16F) == case.fused, where
        # what the class is for
        if k == "steep":
            assert rx >= 3 and ry >= 3 and cw <= 16 and ch <= 16, where
            if case.steps == {0}:
                assert ry >= 4, where                                         # a pure same-row image needs 4x or more in y
        elif k in ("aniso-tall", "aniso-wide"):
            big, small = (rx, ry) if k == "aniso-tall" else (ry, rx)
            assert big >= 3 and 1 < small <= 1.2 and (ch > 2 * cw if k == "aniso-tall" else cw > 2 * ch), where
        elif k == "one-to-one-x":
            assert shape[0] == shape[2] and shape[3] == 2 * shape[1] and steps == {1}, where   # y at 2:1: every pair one row apart
        elif k == "one-to-one-y":
            assert shape[1] == shape[3] and shape[2] == 2 * shape[0] and steps == {1}, where   # y at 1:1: likewise
        elif k in ("tall", "tall-limit"):
            # y minifies while x still fits a fixed pitch: a pair two rows apart, drow >= 2 * PITCH in the mixed path
            assert rx > 1 and ry < 1 and case.pitch != 0 and 2 in steps and 0 not in steps and ch > 36, where
            if k == "tall-limit":                                             # the last few rows below the 64 KiB line (refuse-tall-28: + 5)
                assert easu_lds_bytes(False, RGBA8, cw, ch + 5) > LDS_MAX >= easu_lds_bytes(False, RGBA8, cw, ch), where
        elif k == "x-minify":
            assert rx < 1 < ry and 36 < cw <= 40 and fw > 40, where             # the widest fixed pitch; the fused ring no longer fits one
        elif k in ("wide", "wide-64"):
            assert rx < 1 < ry and cw > 40 and case.pitch == 0, where
            if k == "wide-64":
                assert cw > 64, where                                         # more cells across than a wave has lanes
        elif k == "iso-minify":
            # the generic layout of a byte / half source fits, the 16-byte colour plane of a float source or the strict build does not
            assert rx == ry < 1 and cw > 40 and 1 in steps and 2 in steps, where
            assert easu_lds_bytes(False, RGBA8, cw, ch) <= LDS_MAX < easu_lds_bytes(True, RGBA8, cw, ch), where
            assert easu_lds_bytes(False, RGBA32F, cw, ch) > LDS_MAX, where
        elif k == "refuse-tall":
            # sized by the fast kernel's pitch the product plan does not fit; the strict build's generic layout does
            assert case.pitch != 0 and ry < 1 < rx and easu_lds_bytes(True, RGBA8, cw, ch) <= LDS_MAX < easu_lds_bytes(False, RGBA8, cw, ch), where
        elif k == "refuse-iso":
            assert rx == ry < 1 and cw > 40 and easu_lds_bytes(False, RGBA8, cw, ch) > LDS_MAX, where
    for shape in NIS_SHAPES:
        assert nis_accepted(shape), shape
    tx, ty = (case.masked_shape[2] + TILE - 1) // TILE, (case.masked_shape[3] + TILE - 1) // TILE
    assert tx >= 3 and ty >= 3, (case.id, tx, ty)
