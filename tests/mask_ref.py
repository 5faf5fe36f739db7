"""The radius mask's per-group rule, restated ONCE in numpy, and the table of edge cases tests/test_mask_edges.py (planner, CPU) and
tests/test_gpu_mask_edges.py (pixels, GPU) share.

The rule (fsr_easu.hlsl:41-45, fsr_rcas.hlsl:32-36, NIS_Upscale.hlsl:98-101, NIS_Sharpen.hlsl:96-99): a dispatch group of gw x gh pixels
with origin (x0, y0) is INSIDE where, in uint32 arithmetic modulo 2^32, (cx - (x0 + gw/2))^2 + (cy - (y0 + gh/2))^2 <= R^2 for either of the
two centres of the constant buffer.  Group sizes: FSR 16 x 16, NVScaler 32 x 24, NVSharpen 32 x 32.  Only groups the reference dispatches
exist: ceil(outW / gw) x ceil(outH / gh); a 32-wide tile whose second group column starts behind the image has no such group.

Everything here is computed from the ORACLE's mask constants (oracle.mask_constants), never from the product's, and is itself checked
against the oracle's pixels in tests/test_mask_edges.py (the pixels a mask changes lie in outside groups; the debug tint marks exactly the
outside pixels)."""
import numpy as np

from oracle import oracle as O

GROUPS = {"fsr": (16, 16), "nvscaler": (32, 24), "nvsharpen": (32, 32)}
ALL_INSIDE, ALL_OUTSIDE, MIXED = 0, 1, 2   # csrc/fsr_params.h, MASK_*
U32 = 1 << 32


def group_map(centre, rad, gw, gh):
    """[groupsY, groupsX] bool: the groups of the dispatch that are inside.  Python integers reduced modulo 2^32 at every operation the
    shader performs in uint: the two differences, the two squares, their sum."""
    c = [int(v) for v in centre]
    r2, ow, oh = int(rad[1]), int(rad[2]), int(rad[3])
    gxn, gyn = (ow + gw - 1) // gw, (oh + gh - 1) // gh
    out = np.zeros((gyn, gxn), bool)
    for gy in range(gyn):
        for gx in range(gxn):
            cx, cy = (gx * gw + gw // 2) % U32, (gy * gh + gh // 2) % U32
            d = [(c[0] - cx) % U32, (c[1] - cy) % U32, (c[2] - cx) % U32, (c[3] - cy) % U32]
            q = [(v * v) % U32 for v in d]
            out[gy, gx] = (q[0] + q[1]) % U32 <= r2 or (q[2] + q[3]) % U32 <= r2
    return out


class MaskRef:
    """one eye's mask at one group size"""

    def __init__(self, centre, rad, gw, gh):
        self.centre, self.rad = np.asarray(centre, np.uint32).copy(), np.asarray(rad, np.uint32).copy()
        self.gw, self.gh = gw, gh
        self.outW, self.outH = int(rad[2]), int(rad[3])
        self.groups = group_map(centre, rad, gw, gh)
        self.pixels = np.repeat(np.repeat(self.groups, gh, axis=0), gw, axis=1)[:self.outH, :self.outW]
        self.mode = ALL_INSIDE if self.groups.all() else MIXED if self.groups.any() else ALL_OUTSIDE

    def tile_grid(self, tw, th):
        return (self.outW + tw - 1) // tw, (self.outH + th - 1) // th

    def tiles(self, tw, th):
        """(inside, outside): sets of tile indices (row-major over ceil(outW / tw) columns); inside = holds a pixel of an inside group"""
        tx, ty = self.tile_grid(tw, th)
        inside = {j * tx + i for j in range(ty) for i in range(tx) if self.pixels[j * th:(j + 1) * th, i * tw:(i + 1) * tw].any()}
        return inside, set(range(tx * ty)) - inside

    def ring(self, tw, th):
        """outside tiles that share an edge with an inside tile"""
        tx, ty = self.tile_grid(tw, th)
        inside, outside = self.tiles(tw, th)
        ring = set()
        for t in outside:
            i, j = t % tx, t // tx
            if any(0 <= a < tx and 0 <= b < ty and b * tx + a in inside for a, b in ((i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1))):
                ring.add(t)
        return ring

    def rcas_columns(self, tw=32, th=32):
        """[bands, outW] bool: per band of th rows, the columns RCAS's spans must cover -- those of the band's inside tiles, clipped to outW"""
        tx, ty = self.tile_grid(tw, th)
        cols = np.zeros((ty, self.outW), bool)
        for t in self.tiles(tw, th)[0]:
            cols[t // tx, (t % tx) * tw:(t % tx + 1) * tw] = True
        return cols


def constants(shape, radius, proj, one_eye, eye):
    return O.mask_constants(shape[2], shape[3], radius, proj, one_eye, eye)


def mask_ref(shape, radius, proj, one_eye=True, eye=0, kind="fsr"):
    centre, rad = constants(shape, radius, proj, one_eye, eye)
    return MaskRef(centre, rad, *GROUPS[kind])


# ---- the case table ------------------------------------------------------------------------------------------------------------------
# input -> output: the shapes of the hidden-area and the gaze tests.  S2 and S3 have partial last tiles and partial last groups on both axes.
S1, S2, S3 = (80, 64, 160, 128), (150, 110, 200, 147), (240, 200, 320, 267)


class Case:
    """id; class (the property class_property asserts); shape; radius; the left and the right centre (proj_centre's convention, gaze range
    [-1, 2]); per eye (one entry for a shared texture) `groups`: the number of inside FSR 16 x 16 groups, `pixels`: the inside pixels of FSR's
    groups, `nis_pixels`: of NVScaler's 32 x 24 groups -- what the GPU test asserts before it applies a tolerance; one eye per texture or a
    shared side-by-side texture"""

    def __init__(self, cid, klass, shape, radius, left, right, groups, pixels, nis_pixels, one_eye=True, **more):
        self.id, self.klass, self.shape, self.radius, self.left, self.right = cid, klass, shape, radius, left, right
        self.one_eye, self.groups, self.pixels, self.nis_pixels, self.more = one_eye, groups, pixels, nis_pixels, more

    @property
    def proj(self):
        return tuple(self.left) + tuple(self.right)

    def eyes(self):
        return (0, 1) if self.one_eye else (0,)

    def ref(self, eye, kind="fsr"):
        return mask_ref(self.shape, self.radius, self.proj, self.one_eye, eye, kind)

    def promised_pixels(self, eye, kind="fsr"):
        return (self.pixels if kind == "fsr" else self.nis_pixels)[eye if self.one_eye else 0]


CASES = [
    # centre on a corner: the disc's quarter (or less) on the image
    Case("corner-00-11-S1", "corner", S1, 0.5, (0.0, 0.0), (1.0, 1.0), [3, 3], [768, 768], [768, 1024]),
    Case("corner-11-10-S3", "corner", S3, 0.5, (1.0, 1.0), (1.0, 0.0), [14, 13], [3264, 3328], [4032, 3840], tiles=[6, 4], last=dict(eye=0, column=4, row=4)),
    Case("corner-00-01-S2", "corner", S2, 0.5, (0.0, 0.0), (0.0, 1.0), [4, 5], [1024, 864], [768, 864]),
    # a negative gaze saturates to 0: the constants, and so the bytes, of (0, 0)
    Case("negative-S3", "negative", S3, 0.5, (-1.0, -1.0), (-0.5, -0.25), [13, 13], [3328, 3328], [3840, 3840]),
    # centre past the edge, a sliver inside: left eye right of the image, right eye below it
    Case("sliver-S3", "sliver", S3, 0.9, (1.2, 0.5), (0.5, 1.25), [29, 34], [7424, 7744], [7680, 8256], last=[dict(axis=0, n=12), dict(axis=1, n=12)]),
    # exactly one group inside, in the partial corner tile -- for FSR's groups and for NVScaler's
    Case("one-group-S3", "one-group", S3, 0.9, (1.25, 1.25), (1.25, 1.25), [1, 1], [176, 176], [96, 96]),
    # disc wholly off the image, gaze still in range: the whole frame is the bilinear fallback.  (At 200 x 147 NVScaler's last group column
    # has its centre, 208, behind the image and 32 pixels from the disc's: two NVScaler groups are inside there.)
    Case("all-outside-S1", "all-outside", S1, 0.5, (1.2, 0.5), (1.2, 0.5), [0, 0], [0, 0], [0, 0]),
    Case("all-outside-S2", "all-outside", S2, 0.5, (1.2, 0.5), (1.2, 0.5), [0, 0], [0, 0], [384, 384]),
    Case("all-outside-S3", "all-outside", S3, 0.5, (1.2, 0.5), (1.2, 0.5), [0, 0], [0, 0], [0, 0]),
    # one eye all-outside, the other mixed
    Case("one-eye-out-S3", "one-eye-out", S3, 0.5, (1.2, 0.5), (0.8, 0.7), [0, 54], [0, 13824], [0, 13824]),
    # nearly everything inside: >= 75 % of the groups, an outside tile left, a ring
    Case("nearly-all-S2", "nearly-all", S2, 1.3, (0.5, 0.5), (0.5, 0.5), [103, 103], [24912, 24912], [24864, 24864], tiles=[29, 29]),
    Case("nearly-all-S3", "nearly-all", S3, 1.1, (0.5, 0.5), (0.5, 0.5), [260, 260], [65920, 65920], [64704, 64704], tiles=[74, 74]),
    # a tiny disc at the far corner and at the near one: one FSR group (and no NVScaler group: its centres are 16 and 12 pixels in)
    Case("tiny-far-S3", "one-group-fsr", S3, 0.07, (0.999, 0.999), (0.999, 0.999), [1, 1], [176, 176], [0, 0]),
    Case("tiny-near-S3", "one-group-fsr", S3, 0.05, (0.03, 0.03), (0.03, 0.03), [1, 1], [256, 256], [0, 0]),
    # radius 0 on a group centre: R = 0 and one group inside at distance 0 (<=, not <)
    Case("radius-0-S1", "radius-0", S1, 0.0, (0.05, 0.0625), (0.05, 0.0625), [1, 1], [256, 256], [0, 0]),
    Case("radius-0-S3", "radius-0", S3, 0.0, (0.025, 0.03), (0.025, 0.03), [1, 1], [256, 256], [0, 0]),
    # a shared side-by-side texture whose left centre lands in the right half, or left of the image
    Case("shared-left-2-S3", "shared", S3, 0.9, (2.0, 0.5), (0.5, 0.5), [160], [40960], [39936], one_eye=False, centres=[320, 133, 240, 133]),
    Case("shared-left-neg-S3", "shared", S3, 1.3, (-0.5, 0.5), (0.5, 0.5), [338], [85008], [85344], one_eye=False, centres=[0, 133, 240, 133]),
]
BY_ID = {c.id: c for c in CASES}


def class_property(case):
    """asserts what the case is in the table FOR, from the oracle's constants and the rule above alone; -> per eye the MaskRef (FSR groups)"""
    iw, ih, ow, oh = case.shape
    refs = [case.ref(eye) for eye in case.eyes()]
    k = case.klass
    for eye, r in zip(case.eyes(), refs):
        n = int(r.groups.sum())
        nis = case.ref(eye, "nvscaler")
        inside, outside = r.tiles(32, 32)
        assert n == case.groups[eye], (case.id, eye, n)
        assert int(r.pixels.sum()) == case.pixels[eye], (case.id, eye, int(r.pixels.sum()))
        assert int(nis.pixels.sum()) == case.nis_pixels[eye], (case.id, eye, int(nis.pixels.sum()))
        if "tiles" in case.more:
            assert len(inside) == case.more["tiles"][eye], (case.id, eye, len(inside))
        if k in ("corner", "negative"):
            # non-empty, and confined to one corner tile or its neighbours: within two 32 x 32 tiles of a corner of the tile grid
            tx, ty = r.tile_grid(32, 32)
            assert inside and r.mode == MIXED, case.id
            cols, rows = {t % tx for t in inside}, {t // tx for t in inside}
            assert (max(cols) <= 1 or min(cols) >= tx - 2) and (max(rows) <= 2 or min(rows) >= ty - 3), (case.id, eye, sorted(inside))
            assert int(r.centre[0]) in (0, ow) and int(r.centre[1]) in (0, oh), (case.id, r.centre)
        if k == "negative":
            zero = mask_ref(case.shape, case.radius, (0.0, 0.0, 0.0, 0.0), True, eye)
            assert np.array_equal(r.centre, zero.centre) and np.array_equal(r.rad, zero.rad) and not r.centre.any(), (case.id, r.centre)
        if k == "sliver":
            axis = case.more["last"][eye]["axis"]          # 0: the centre is right of the image, 1: below it
            assert int(r.centre[axis]) > (ow, oh)[axis], (case.id, r.centre)
            along = r.groups.any(axis=axis)                 # axis 0: per group column, axis 1: per group row -- any group inside?
            first = int(np.flatnonzero(along)[0])
            assert along[first:].all() and first > along.size // 2, (case.id, eye, along)   # the last columns (rows) only, the last one included
            last = r.groups[:, -1] if axis == 0 else r.groups[-1, :]
            assert int(last.sum()) == case.more["last"][eye]["n"], (case.id, eye, int(last.sum()))
        if k in ("one-group", "one-group-fsr", "radius-0"):
            assert n == 1 and r.mode == MIXED, (case.id, eye, n)
        if k == "one-group":
            assert int(nis.groups.sum()) == 1 and r.groups[-1, -1] and nis.groups[-1, -1], case.id   # the partial corner, for both group sizes
            assert oh % 16 and oh % 24, case.id
        if k == "radius-0":
            assert int(r.rad[0]) == 0 and int(r.rad[1]) == 0, (case.id, r.rad)
            gy, gx = (int(v[0]) for v in np.nonzero(r.groups))
            assert (int(r.centre[0]), int(r.centre[1])) == (16 * gx + 8, 16 * gy + 8), (case.id, r.centre)   # distance 0: <=, not <
        if k == "all-outside":
            assert n == 0 and r.mode == ALL_OUTSIDE and not r.pixels.any(), case.id
            assert -1.0 <= min(case.proj) and max(case.proj) <= 2.0
        if k == "nearly-all":
            assert r.mode == MIXED and n >= 0.75 * r.groups.size and len(outside) >= 1 and r.ring(32, 32), (case.id, n, len(outside))
        if k == "shared":
            assert [int(v) for v in r.centre] == case.more["centres"], (case.id, r.centre)
            assert r.mode == MIXED and (int(r.centre[0]) >= ow // 2 or int(r.centre[0]) == 0), case.id   # the left centre: right half, or saturated
    if k == "one-eye-out":
        assert [r.mode for r in refs] == [ALL_OUTSIDE, MIXED], (case.id, [r.mode for r in refs])
    if k == "corner" and "last" in case.more:
        m = case.more["last"]
        r = refs[m["eye"]]
        assert int(r.groups[:, -1].sum()) == m["column"] and int(r.groups[-1, :].sum()) == m["row"], case.id
    return refs
