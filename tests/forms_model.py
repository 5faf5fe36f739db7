"""The launch manager's pixel contract for the launch-form matrix (tools/debug/record_forms.py::cases()), restated once: numpy and the
CPU oracle, no GPU.

    decoded(src, w, h, seed)   the image the pipeline sees for one of the matrix's eight sources, read from the very array
                               record_forms.source_array hands to the upload
    expected(case)             the arrays record_forms.run_case hashes for the case -- dtype, shape and order -- and the contract class
                               the product build's output is held to
    check(case, got, ...)      one device output against expected(case) under its class (tests/test_gpu_launch_forms_oracle.py)

The composition (include/openvr_fsr_amd.h; csrc/pipeline_plan.cpp::plan_filtered for the stage and format rules):

    source -> decode / resolve -> [EASU | NVScaler] -> intermediate -> [RCAS | NVSharpen] -> destination encoding

  stages        upscale iff the output size differs from the input's (render_scale != 1), sharpen iff !use_nis or the sizes are equal;
                stage_mask 1 / 2 drops the sharpen / the upscale stage; neither stage left: the submitted image is handed back untouched
  intermediate  of an EASU + RCAS pipeline: fp32 with quantize_intermediate = 0, else the format of the ctx's own textures -- the
                pipeline format of the input (RGBA8, RGBA16F, RGBA32F, RGB10A2), UNORM8 for a float input under reference_formats = 1
  destination   the caller's image, or the ctx's own format (the rule above, whatever quantize_intermediate says)
  mask          oracle.mask_constants per eye and call kind: one eye per texture for apply / pair / batch4 (eyes alternating from 0),
                a shared side-by-side texture (both centres in one mask) for `shared`
  fused         changes the launch form, never the composition

Which cases are accepted is the record's and the planner tests' business; expected() predicts pixels for whatever it is asked.

Contract classes (header, "Arithmetic the kernels run in" and the format paragraphs; the constants are the ones the other GPU files assert):
  bits     byte for byte: every precision-2 and every accepted precision-3 case, product EASU-only into UNORM8, a case without a stage
  u8       product UNORM8 pipeline outputs: <= RCAS_LSB
  float    RGBA32F outputs behind an exact (UNORM8) or fp32 intermediate or of a single FSR stage: <= FLOAT_TOL
  half     a half rounding on the way (half intermediate or half destination): 99.9 % of the values within 1e-3, none beyond 2e-2
           (tests/test_gpu_fuzz.py::test_masked_product_fuzz_half)
  nis      NVScaler / NVSharpen: RGBA32F <= NIS_FLOAT_TOL x max(1, largest texel), RGBA16F that plus one half spacing, UNORM8 <= 1 LSB
           (tests/test_gpu_nis_formats.py)
  ten-bit  RGB10A2 outputs: <= 1.01 LSB of 10 bits, at most 4e-3 of the values beyond half an LSB, alpha equal
           (tests/test_gpu_formats.py::test_fsr_rgb10a2_product_tolerance)
Inside every class the pixels of groups outside the radius are the oracle's bytes in every RGBA8 form (the bilinear fallback behind a
UNORM8 store) and in NVScaler's / NVSharpen's DirectCopy groups, whatever the destination (tests/test_gpu_nis_formats.py).
"""
import functools
import importlib.util
import os

import numpy as np

from oracle import oracle as O
from tests import mask_ref, msaa, nis_cases, packedf
from tests.test_gpu_formats import oracle_fsr10, pack10, unpack10
from tests.test_gpu_nis_formats import HALF_SPACING
from tests.test_gpu_parity import FLOAT_TOL, NIS_FLOAT_TOL, RCAS_LSB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def record_forms():
    spec = importlib.util.spec_from_file_location("record_forms", os.path.join(ROOT, "tools", "debug", "record_forms.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    return R


BITS, U8, FLOAT, HALF, NIS, TEN_BIT = "bits", "u8", "float", "half", "nis", "ten-bit"
STRICT, EXACT = 2, 3
SHARPNESS_DEFAULT = 0.75

# the format the kernels read for each source (csrc/fsr_formats.h::pipeline_format)
PIPELINE_FORMAT = {"rgba8": "rgba8", "bgra8": "rgba8", "ms4_rgba8": "rgba8", "rgba16f": "rgba16f", "ms2_rgba16f": "rgba16f",
                   "r11g11b10f": "rgba16f", "rgba32f": "rgba32f", "rgb10a2": "rgb10a2"}
FLOAT_FORMATS = ("rgba16f", "rgba32f")

# Accepted product-build cells that no sentence of the header describes: each gets the class of its destination encoding.
#   * NIS on an RGB10A2 image: the header gives NIS bounds for UNORM8 and float outputs only -> ten-bit;
#   * an EASU-only pass into RGBA16F (the near-tie guard of half stores is on only in front of RCAS) -> half;
#   * an EASU-only pass into RGB10A2 -> ten-bit;
#   * an RGBA8 source through a UNORM8 intermediate into a caller-owned RGBA16F image -> half.
UNDESCRIBED = (
    "rgb10a2/p0-nis1-sm0-f-1-q1-rf0-m1", "rgb10a2/p0-nis0-sm1-f-1-q1-rf0-m1",
    "rgba16f/p0-nis0-sm1-f-1-q1-rf0-m0", "rgba16f/p0-nis0-sm1-f-1-q1-rf0-m1",
    "r11g11b10f/p0-nis0-sm1-f-1-q1-rf0-m1", "ms2_rgba16f/p0-nis0-sm1-f-1-q1-rf0-m1",
    "rgba8/p0-nis0-sm0-f-1-q1-rf0-m0/to-rgba16f",
)
# Cases with a hash in the record that expected() cannot model (at most 8, none with an RGBA8 or RGBA16F source)
UNMODELLED = {}


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def decoded(src, w, h, seed, content="structured"):
    """What the pipeline sees: uint8 [h, w, 4] (RGBA8, BGRA8 re-ordered, 4x RGBA8 resolved), packed int32 [h, w] (RGB10A2), float32
    [h, w, 4] (RGBA16F, RGBA32F, 2x RGBA16F resolved to half, R11G11B10F decoded to half), by the header's decode and resolve rules."""
    a, _ = record_forms().source_array(src, w, h, seed, content)
    if src == "rgba8" or src == "rgb10a2":
        out = a.copy()
    elif src == "bgra8":
        out = np.ascontiguousarray(a[..., [2, 1, 0, 3]])
    elif src == "ms4_rgba8":
        out = msaa.resolve_unorm8(a)
    elif src == "rgba16f":
        out = a.astype(np.float32)
    elif src == "rgba32f":
        out = a.copy()
    elif src == "ms2_rgba16f":
        out = msaa.resolve_float(a).astype(np.float32)
    elif src == "r11g11b10f":
        out = packedf.unpack(a).astype(np.float32)
    else:
        raise ValueError(src)
    return _frozen(out)


def _to_float(img, pf):
    return O.unorm8_to_float(img) if pf == "rgba8" else unpack10(img) if pf == "rgb10a2" else np.asarray(img, np.float32)


def encode(x, fmt):
    """the store conversion of a destination or an intermediate"""
    if fmt == "rgba8":
        return O.float_to_unorm8(x)
    if fmt == "rgba16f":
        return np.asarray(x, np.float32).astype(np.float16)
    if fmt == "rgba32f":
        return np.ascontiguousarray(x, np.float32)
    if fmt == "rgb10a2":
        return pack10(x)
    raise ValueError(fmt)


def _requantise(x, fmt):
    return _to_float(encode(x, fmt), fmt)


class Plan:
    """the fields of csrc/pipeline_plan.cpp's plan that decide pixels"""

    def __init__(self, case):
        cfg = case["cfg"]
        self.src, self.kind = case["src"], case["kind"]
        self.iw, self.ih = case["shape"][:2]
        self.nis = bool(cfg.get("use_nis", 0))
        self.sharpness = cfg.get("sharpness", SHARPNESS_DEFAULT)
        self.radius, self.proj = cfg["radius"], tuple(cfg.get("proj_centre", (0.5,) * 4))
        self.precision = cfg.get("precision", 0)
        self.pf = PIPELINE_FORMAT[self.src]
        rf, q, sm = cfg.get("reference_formats", 0), cfg.get("quantize_intermediate", 1), cfg.get("stage_mask", 0)
        self.owned = ("rgb10a2" if self.pf == "rgb10a2" else "rgba8") if rf else self.pf      # DetermineOutputFormat / the library's own rule
        self.mid = self.owned if q else "rgba32f"
        if cfg.get("out_width") and cfg.get("out_height"):
            self.ow, self.oh = cfg["out_width"], cfg["out_height"]
            scaled = (self.ow, self.oh) != (self.iw, self.ih)
        else:   # PostProcessor.cpp:512-518, float arithmetic truncated to uint
            s = np.float32(cfg["render_scale"])
            f = (lambda n: np.float32(n) / s) if s < 1 else (lambda n: np.float32(n) * s)
            self.ow, self.oh = int(f(self.iw)), int(f(self.ih))
            scaled = float(s) != 1.0
        self.upscale = scaled and sm != 2
        self.sharpen = (not self.nis or not scaled) and sm != 1
        self.dst = case["dst"] if case["dst"] != "owned" else self.owned
        self.one_eye = self.kind != "shared"

    @property
    def shape(self):
        return (self.iw, self.ih, self.ow, self.oh)

    def group_kind(self):
        return ("nvscaler" if self.upscale else "nvsharpen") if self.nis else "fsr"


def _image(plan, x, eye):
    """one submitted image through the composition -> the destination's array"""
    p = plan
    if not (p.upscale or p.sharpen):
        raise AssertionError("no stage: handled by expected()")
    if p.nis:
        f = _to_float(x, p.pf)
        assert p.one_eye, "nis_cases asks the oracle for one eye per texture"
        if p.upscale:
            out = nis_cases.want_scaler(f, p.ow, p.oh, p.sharpness, p.radius, p.proj, eye)
        else:
            out = nis_cases.want_sharpen(f, p.sharpness, p.radius, p.proj, eye)
        return encode(out, p.dst)
    stages = (1 if p.upscale else 0) | (2 if p.sharpen else 0)
    both = stages == 3
    if p.pf == "rgba8" and p.dst == "rgba8" and (not both or p.mid in ("rgba8", "rgba32f")):
        return O.fsr_pipeline_u8(x, p.ow, p.oh, sharpness=p.sharpness, radius=p.radius, proj=p.proj, eye=eye, one_eye_per_texture=p.one_eye,
                                 stages=stages, quantize_intermediate=p.mid == "rgba8")
    if p.pf == "rgb10a2" and p.one_eye and (not both or p.mid == "rgb10a2"):
        return encode(oracle_fsr10(x, p.ow, p.oh, p.sharpness, p.radius, p.proj, eye, 0, stages), p.dst)
    centre, rad = O.mask_constants(p.ow, p.oh, p.radius, p.proj, p.one_eye, eye)
    f = _to_float(x, p.pf)
    if p.upscale:
        f = O.easu(f, p.ow, p.oh, O.easu_con(p.iw, p.ih, p.ow, p.oh), centre, rad)
        if both:
            f = _requantise(f, p.mid)
    if p.sharpen:
        f = O.rcas(f, O.rcas_con(p.sharpness, 0), centre, rad)
    return encode(f, p.dst)


def eyes_and_seeds(kind):
    """per output image of a case: (eye, seed of its source) -- record_forms.run_case"""
    if kind == "batch4":
        return [(0, 3), (1, 4), (0, 3), (1, 4)]
    if kind == "shared":
        return [(0, 3), (0, 4)]
    if kind == "pair":
        return [(0, 3), (1, 4)]
    return [(0, 3)]


def contract(case):
    p = Plan(case)
    if p.precision in (STRICT, EXACT) or not (p.upscale or p.sharpen):
        return BITS
    if p.dst == "rgb10a2":
        return TEN_BIT
    if p.nis:
        return NIS
    if p.dst == "rgba8":
        # EASU alone: the near-tie guard makes the store the strict build's (RGBA8 sources; float sources under reference_formats)
        guarded = p.pf == "rgba8" or bool(case["cfg"].get("reference_formats", 0))
        return BITS if p.upscale and not p.sharpen and guarded else U8
    if p.dst == "rgba16f" or (p.upscale and p.sharpen and p.mid == "rgba16f"):
        return HALF
    return FLOAT


def auto_is_fused(case):
    """fused = -1 picks the fused kernel (csrc/pipeline_plan.cpp: masked product-build EASU + RCAS whose intermediate is not UNORM8);
    everywhere else fused = -1 and fused = 0 store the same bytes"""
    p = Plan(case)
    return (p.precision == 0 and case["mask"] and p.upscale and p.sharpen and not p.nis and p.mid != "rgba8" and p.pf != "rgb10a2")


@functools.lru_cache(maxsize=None)
def _expected(cid, content):
    case = BY_ID()[cid]
    p = Plan(case)
    imgs = []
    for eye, seed in eyes_and_seeds(p.kind):
        if not (p.upscale or p.sharpen):
            imgs.append(record_forms().source_array(p.src, p.iw, p.ih, seed, content)[0].copy())   # the submission handed back as it is
        else:
            imgs.append(_image(p, decoded(p.src, p.iw, p.ih, seed, content), eye))
    arrays = [np.stack(imgs)] if p.kind in ("batch4", "shared") else imgs
    return tuple(_frozen(np.ascontiguousarray(a)) for a in arrays)


@functools.lru_cache(maxsize=None)
def BY_ID():
    return {c["id"]: c for c in record_forms().cases()}


def expected(case, content="structured"):
    """-> (list of arrays as record_forms.run_case hashes them, contract class).  The arrays are shared and read-only."""
    return list(_expected(case["id"], content)), contract(case)


@functools.lru_cache(maxsize=None)
def _outside(cid):
    case = BY_ID()[cid]
    p = Plan(case)
    if not (p.upscale or p.sharpen):
        return None
    maps = [~mask_ref.mask_ref(p.shape, p.radius, p.proj, p.one_eye, eye, p.group_kind()).pixels for eye, _ in eyes_and_seeds(p.kind)]
    return tuple(_frozen(m) for m in maps)


def outside_pixels(case):
    """per output image: bool [oh, ow], the pixels of dispatch groups outside the radius (tests/mask_ref.py)"""
    return _outside(case["id"])


def texel_scale(case, content="structured"):
    """max(1, largest colour value the pipeline sees): what the NIS float bound scales with"""
    p = Plan(case)
    if p.pf not in FLOAT_FORMATS:
        return 1.0
    return max(1.0, max(float(decoded(p.src, p.iw, p.ih, seed, content)[..., :3].max()) for _, seed in eyes_and_seeds(p.kind)))


# ---- comparison -------------------------------------------------------------------------------------------------------------------
def _words(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _values(a):
    """an output array as float32 [..., 4] in the unit of its class (10-bit: LSBs of the colour channels, alpha in thirds)"""
    if a.dtype == np.int32:
        return unpack10(a) * np.array([1023, 1023, 1023, 3], np.float32)
    return a.astype(np.float32)


def distance(got, want):
    """-> dict: what reports/launch_forms_oracle.json records for one output array"""
    same = _words(got) == _words(want)
    d = np.abs(_values(got) - _values(want))
    key = "max_lsb" if got.dtype in (np.uint8, np.int32) else "max_abs"
    return {key: float(d.max()), "differing": float((~same).mean())}


def check(case, got, content="structured"):
    """device outputs `got` (run_case(..., arrays=True)["arrays"]) against expected(case) under its class -> list of distance records.
    Raises AssertionError with the case id and the figures."""
    want, klass = expected(case, content)
    cid = case["id"]
    assert got is not None and len(got) == len(want), (cid, "outputs", None if got is None else len(got), len(want))
    outside = outside_pixels(case)
    p = Plan(case)
    out = []
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (cid, k, g.dtype, g.shape, w.dtype, w.shape)
        same = _words(g) == _words(w)
        rec = dict(distance(g, w), output=k)
        out.append(rec)
        if klass == BITS:
            assert same.all(), (cid, content, klass, "%d of %d values differ from the oracle" % (int((~same).sum()), same.size), rec)
            continue
        # the bits sub-assertion: groups outside the radius -- every RGBA8 form, and NVScaler's / NVSharpen's DirectCopy groups
        if outside is not None and (p.dst == "rgba8" or (p.nis and p.dst in FLOAT_FORMATS)):
            m = np.stack(outside) if p.kind in ("batch4", "shared") else outside[k]
            bad = ~same[m]
            assert not bad.any(), (cid, content, klass, "%d values of groups outside the radius differ from the oracle" % int(bad.sum()), rec)
        gv, wv = _values(g), _values(w)
        assert not np.isnan(gv).any(), (cid, content, "NaN")
        d = np.abs(gv - wv)
        if klass == U8:
            assert g.dtype == np.uint8 and d.max() <= RCAS_LSB, (cid, content, klass, rec)
        elif klass == FLOAT:
            assert g.dtype == np.float32 and d.max() <= FLOAT_TOL, (cid, content, klass, rec)
        elif klass == HALF:
            assert (d <= 1e-3).mean() >= 0.999 and d.max() <= 2e-2, (cid, content, klass, float((d <= 1e-3).mean()), rec)
        elif klass == NIS:
            if g.dtype == np.uint8:
                assert d.max() <= 1, (cid, content, klass, rec)
            else:
                extra = HALF_SPACING if g.dtype == np.float16 else 0.0
                assert d.max() <= NIS_FLOAT_TOL * texel_scale(case, content) + extra, (cid, content, klass, rec)
        elif klass == TEN_BIT:
            c = d[..., :3]
            assert c.max() <= 1.01 and (c > 0.5).mean() <= 4e-3, (cid, content, klass, float((c > 0.5).mean()), rec)
            assert np.array_equal(gv[..., 3], wv[..., 3]), (cid, content, klass, "alpha")
        else:
            raise AssertionError(klass)
    return out
