"""tests/forms_model.py -- the launch-form matrix's pixels predicted from the CPU oracle -- checked without a GPU:
  * every case whose record (tests/golden/launch_forms_parent.json, taken on an MI355X) holds a hash has an expectation and a class;
  * for every case whose whole frame is promised byte for byte -- the strict build, exact stores, product EASU-only into UNORM8 -- the
    SHA-256 of the model's bytes IS the recorded hash: the model is pinned to device output, and those record entries to the oracle;
  * the expectations are not vacuous: every axis that should change pixels does, the mask is a mask, float outputs are not saturated;
  * on the cells other GPU files pin, the model returns what their helper returns, byte for byte."""
import json
import os
import re

import numpy as np
import pytest

from oracle import oracle as O
from tests import forms_model as M
from tests import mask_ref, nis_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = M.record_forms()


@pytest.fixture(scope="module")
def record():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "launch_forms_parent.json")))


@pytest.fixture(scope="module")
def accepted(record):
    return [c for c in R.cases() if record[c["id"]]["sha256"]]


def _by_id(accepted):
    return {c["id"]: c for c in accepted}


def test_every_accepted_case_has_an_expectation_and_a_class(record, accepted):
    assert len(accepted) == 446
    assert len(M.UNMODELLED) <= 8
    for cid, reason in M.UNMODELLED.items():
        assert record[cid]["sha256"] and reason.strip(), cid
        assert M.BY_ID()[cid]["src"] not in ("rgba8", "rgba16f"), cid
    classes = {}
    for c in accepted:
        if c["id"] in M.UNMODELLED:
            continue
        arrays, klass = M.expected(c)
        assert klass in (M.BITS, M.U8, M.FLOAT, M.HALF, M.NIS, M.TEN_BIT), c["id"]
        classes[klass] = classes.get(klass, 0) + 1
        # dtype, shape and order of what run_case hashes
        iw, ih, ow, oh = c["shape"]
        p = M.Plan(c)
        n = {"apply": 1, "pair": 2, "batch4": 1, "shared": 1}[c["kind"]]
        assert len(arrays) == n, c["id"]
        lead = {"batch4": (4,), "shared": (2,)}.get(c["kind"], ())
        for a in arrays:
            if not (p.upscale or p.sharpen):
                assert a.shape == (ih, iw, 4) and a.dtype == np.uint8, c["id"]
            elif p.dst == "rgb10a2":
                assert a.dtype == np.int32 and a.shape == lead + (p.oh, p.ow), (c["id"], a.shape)
            else:
                dt = {"rgba8": np.uint8, "rgba16f": np.float16, "rgba32f": np.float32}[p.dst]
                assert a.dtype == dt and a.shape == lead + (p.oh, p.ow, 4), (c["id"], a.dtype, a.shape)
        own = record[c["id"]]["owned_format"]
        if own is not None and (p.upscale or p.sharpen):
            assert R.FORMAT_NAMES[own] == p.dst, (c["id"], own, p.dst)
    assert set(classes) == {M.BITS, M.U8, M.FLOAT, M.HALF, M.NIS, M.TEN_BIT}, classes
    # the cells no sentence of the header describes are accepted product-build cases, classed by their destination encoding
    for cid in M.UNDESCRIBED:
        c = M.BY_ID()[cid]
        assert record[cid]["sha256"] and c["cfg"]["precision"] == 0, cid
        assert M.contract(c) == {"rgba16f": M.HALF, "rgb10a2": M.TEN_BIT}[M.Plan(c).dst], cid


def test_whole_frame_bits_cases_hash_to_the_record(record, accepted):
    """the model's bytes against what an MI355X stored: every precision-2 and precision-3 case, product EASU-only into UNORM8"""
    n, bad = 0, []
    strict = exact = product = 0
    for c in accepted:
        arrays, klass = M.expected(c)
        if klass != M.BITS:
            assert c["cfg"].get("precision", 0) == 0, c["id"]
            continue
        n += 1
        prec = c["cfg"].get("precision", 0)
        strict, exact, product = strict + (prec == 2), exact + (prec == 3), product + (prec == 0)
        if R.sha_of(arrays) != record[c["id"]]["sha256"]:
            bad.append(c["id"])
    assert not bad, "%d of %d whole-frame bits cases do not hash to the record: %r" % (len(bad), n, bad[:10])
    assert n == 231 and strict >= 140 and exact >= 40 and product >= 25, (n, strict, exact, product)


# ---- not vacuous --------------------------------------------------------------------------------------------------------------------
def _flip(cid, field, a, b):
    """the id of the case that differs from cid in one field of its configuration name, or None"""
    parts = cid.split("/")
    new, k = re.subn(r"(?<![a-z0-9])%s%d(?=-|$)" % (field, a), "%s%d" % (field, b), parts[1])
    if k != 1:
        return None
    return "/".join([parts[0], new] + parts[2:])


def _floats(arrays):
    return np.concatenate([M._values(a).ravel() for a in arrays])


def _differ(a, b):
    if len(a) != len(b) or any(x.shape != y.shape for x, y in zip(a, b)):
        return True
    return not np.array_equal(_floats(a), _floats(b))


def test_every_axis_that_should_change_pixels_does(accepted):
    ids = _by_id(accepted)
    counts = {}
    for cid, c in ids.items():
        p = M.Plan(c)
        if not (p.upscale or p.sharpen) or "render-scale" in cid:
            continue
        both = p.upscale and p.sharpen and not p.nis
        axes = []
        if both and p.pf != "rgba32f":
            axes.append(("q", "q", 1, 0))                     # a quantised intermediate against fp32
        if p.pf in M.FLOAT_FORMATS and (both or c["dst"] == "owned"):
            axes.append(("rf", "rf", 0, 1))                   # a float source: UNORM8 intermediate / ctx-owned output
        axes.append(("mask", "m", 0, 1))
        axes.append(("nis", "nis", 0, 1))
        if not p.nis:
            axes.append(("sm1", "sm", 0, 1))
        axes.append(("sm2", "sm", 0, 2))
        for name, field, a, b in axes:
            other = _flip(cid, field, a, b)
            if other is None or other not in ids:
                continue
            counts[name] = counts.get(name, 0) + 1
            assert _differ(M.expected(c)[0], M.expected(ids[other])[0]), (name, cid, other)
    assert all(counts.get(k, 0) >= n for k, n in (("q", 10), ("rf", 4), ("mask", 100), ("nis", 30), ("sm1", 30), ("sm2", 30))), counts


def test_the_matrix_mask_is_a_mask():
    """tests/test_pipeline_plan.py::test_matrix_mask_is_a_mask on the oracle's constants: at 160 x 128 each eye has a tile inside the
    radius, a ring tile and an outside tile that is not ring, for FSR's tiles and NVScaler's; the eyes' masks are unequal"""
    for kind, (tw, th) in (("fsr", (32, 32)), ("nvscaler", (32, 24))):
        refs = [mask_ref.mask_ref(R.BASE, R.MASK_ON["radius"], R.MASK_ON["proj_centre"], True, eye, kind) for eye in (0, 1)]
        for r in refs:
            inside, outside = r.tiles(tw, th)
            ring = r.ring(tw, th)
            assert len(inside) >= 1 and len(ring) >= 1 and len(outside) - len(ring) >= 1, (kind, len(inside), len(ring), len(outside))
            assert r.mode == mask_ref.MIXED
        assert not np.array_equal(refs[0].pixels, refs[1].pixels), kind
    # and MASK_OFF is none: every group inside
    assert mask_ref.mask_ref(R.BASE, R.MASK_OFF["radius"], (0.5,) * 4, True, 0).mode == mask_ref.ALL_INSIDE
    # the model's outside maps are those masks
    c = M.BY_ID()["rgba8/p0-nis0-sm0-f-1-q1-rf0-m1/pair"]
    out = M.outside_pixels(c)
    assert len(out) == 2 and all(0.2 < m.mean() < 0.95 for m in out) and not np.array_equal(out[0], out[1])
    shared = M.outside_pixels(M.BY_ID()["rgba8/p0-nis0-sm0-f-1-q1-rf0-m1/to-rgba8/shared"])
    assert np.array_equal(shared[0], shared[1]) and not np.array_equal(shared[0], out[0])


def test_float_source_expectations_are_not_saturated(accepted):
    n = 0
    for c in accepted:
        p = M.Plan(c)
        if p.pf not in M.FLOAT_FORMATS:
            continue
        for content in R.CONTENTS if c["cfg"].get("precision", 0) != 2 else ("structured",):
            for a in M.expected(c, content)[0]:
                v = M._values(a)[..., :3] / (255.0 if a.dtype == np.uint8 else 1.0)
                share = float(((v > 0) & (v < 1)).mean())
                assert share >= nis_cases.MIN_INSIDE, (c["id"], content, share)
                n += 1
    assert n >= 100, n


# ---- agreement with the helpers of the other GPU files -----------------------------------------------------------------------------------
def test_agrees_with_the_rgba8_two_pass_composition():
    """tests/test_gpu_parity.py's cell: float_to_unorm8(rcas(unorm8 intermediate of easu)), both eyes of the masked pair"""
    c = M.BY_ID()["rgba8/p0-nis0-sm0-f-1-q1-rf0-m1/pair"]
    got, klass = M.expected(c)
    assert klass == M.U8
    iw, ih, ow, oh = c["shape"]
    for eye in (0, 1):
        centre, rad = O.mask_constants(ow, oh, c["cfg"]["radius"], c["cfg"]["proj_centre"], True, eye)
        f = O.unorm8_to_float(M.decoded("rgba8", iw, ih, 3 + eye))
        mid = O.unorm8_to_float(O.float_to_unorm8(O.easu(f, ow, oh, O.easu_con(iw, ih, ow, oh), centre, rad)))
        assert np.array_equal(got[eye], O.float_to_unorm8(O.rcas(mid, O.rcas_con(0.9), centre, rad))), eye


def test_agrees_with_the_ten_bit_helper():
    from tests.test_gpu_formats import oracle_fsr10, pack10
    for cid, stages in (("rgb10a2/p2-nis0-sm0-f-1-q1-rf0-m1", 3), ("rgb10a2/p0-nis0-sm1-f-1-q1-rf0-m1", 1)):
        c = M.BY_ID()[cid]
        iw, ih, ow, oh = c["shape"]
        want = pack10(oracle_fsr10(M.decoded("rgb10a2", iw, ih, 3), ow, oh, 0.9, c["cfg"]["radius"], c["cfg"]["proj_centre"], 0, 0, stages))
        assert np.array_equal(M.expected(c)[0][0], want), cid


def test_agrees_with_the_reference_formats_helper():
    from tests.test_gpu_reference_formats import _oracle
    for src in ("rgba16f", "rgba32f", "r11g11b10f", "ms2_rgba16f"):
        cid = "%s/p0-nis0-sm0-f-1-q1-rf1-m%d" % (src, 0 if src == "rgba16f" else 1)
        c = M.BY_ID()[cid]
        iw, ih, ow, oh = c["shape"]
        got = M.expected(c)[0][0]
        assert got.dtype == np.uint8
        if not c["mask"]:       # (_oracle takes a radius, not a projection centre: the unmasked cell)
            assert np.array_equal(got, _oracle(M.decoded(src, iw, ih, 3), ow, oh, sharp=0.9)), cid
        else:
            centre, rad = O.mask_constants(ow, oh, c["cfg"]["radius"], c["cfg"]["proj_centre"], True, 0)
            mid = O.float_to_unorm8(O.easu(M.decoded(src, iw, ih, 3), ow, oh, O.easu_con(iw, ih, ow, oh), centre, rad))
            assert np.array_equal(got, O.float_to_unorm8(O.rcas(O.unorm8_to_float(mid), O.rcas_con(0.9), centre, rad))), cid
    c = M.BY_ID()["rgba16f/p0-nis0-sm1-f-1-q1-rf1-m0/to-rgba8"]
    assert np.array_equal(M.expected(c)[0][0], _oracle(M.decoded("rgba16f", 80, 64, 3), 160, 128, sharp=0.9, stages=1))


def test_agrees_with_the_nis_float_helper():
    for cid, dt in (("rgba16f/p0-nis1-sm0-f-1-q1-rf0-m1", np.float16), ("rgba32f/p0-nis1-sm0-f-1-q1-rf0-m1", np.float32)):
        c = M.BY_ID()[cid]
        iw, ih, ow, oh = c["shape"]
        want = nis_cases.want_scaler(M.decoded(c["src"], iw, ih, 3), ow, oh, 0.9, c["cfg"]["radius"], c["cfg"]["proj_centre"], 0)
        got, klass = M.expected(c)
        assert klass == M.NIS and got[0].dtype == dt and np.array_equal(got[0], want.astype(dt)), cid
    c = M.BY_ID()["rgba16f/p0-nis1-sm2-f-1-q1-rf0-m0"]
    want = nis_cases.want_sharpen(M.decoded("rgba16f", 96, 80, 3), 0.9)
    assert np.array_equal(M.expected(c)[0][0], want.astype(np.float16))


def test_decoded_is_what_is_uploaded():
    """decoded() reads record_forms.source_array's arrays; the upload half hands exactly those to the device"""
    from tests import msaa, packedf, synth
    u8 = synth.structured_u8(80, 64, 3)
    assert np.array_equal(M.decoded("rgba8", 80, 64, 3), u8) and np.array_equal(M.decoded("bgra8", 80, 64, 3), u8)
    f = u8.astype(np.float32) / np.float32(255)
    assert np.array_equal(M.decoded("rgba32f", 80, 64, 3), f)
    assert np.array_equal(M.decoded("rgba16f", 80, 64, 3), f.astype(np.float16).astype(np.float32))
    ten = M.decoded("rgb10a2", 80, 64, 3).view(np.uint32)
    assert np.array_equal(ten & 1023, u8[..., 0].astype(np.uint32) * 4 + (u8[..., 0] >> 6)) and (ten >> 30 == 3).all()
    words, fmt = R.source_array("r11g11b10f", 80, 64, 3)
    assert fmt == R.R11G11B10F
    r, g, b = packedf.channels(words)
    want = np.stack([packedf.value_of(r, 6), packedf.value_of(g, 6), packedf.value_of(b, 5)], axis=-1)
    assert np.array_equal(M.decoded("r11g11b10f", 80, 64, 3)[..., :3].astype(np.float64), want)
    ms, _ = R.source_array("ms4_rgba8", 80, 64, 3)
    assert ms.shape == (64, 80, 4, 4) and np.array_equal(M.decoded("ms4_rgba8", 80, 64, 3), msaa.resolve(ms, "rgba8"))
    assert np.array_equal(R.source_array("rgba8", 80, 64, 3, "random")[0], synth.random_u8(80, 64, 3))
