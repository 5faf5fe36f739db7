"""RCAS on the RGBA8 path evaluates ONE quotient per channel (fsr_device.inc: rcas_lobe_bytes) where FsrRcasF has two.

    max(-mn/(4 mx), (P-mx)/(4 mn - 4 P))  =  -min(mn, P-mx) / (4 min(mx, P-mn))        for 0 <= mn <= mx <= P

Checked here without a GPU, over all 32 896 pairs of byte extrema (P = 255):
  * the identity in exact rational arithmetic;
  * in fp32, with a correctly rounded 1/x standing in for v_rcp_f32: the per-channel value is the same bit pattern wherever mn != mx; for
    mn == mx both forms are below the clamp -LIMIT; for the two pairs with a zero denominator the new form is NaN ("does not limit");
  * the scope of the re-recorded machine-code fingerprints: only the byte-domain RCAS kernels changed, and easu_fast_kernel (the pair
    resolve's shared dering extrema, part of the same change).
tests/test_gpu_rcas_identity.py repeats the comparison on the device with the real v_rcp_f32 and the shipped helper."""
import os
import re
from fractions import Fraction

import numpy as np

from tests import isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 255
LIMIT = np.float32(0.25 - 1.0 / 16.0)
PAIRS = [(mn, mx) for mx in range(P + 1) for mn in range(mx + 1)]
DEGENERATE = [(0, 0), (P, P)]


def test_pair_count():
    assert len(PAIRS) == 32896


def test_rational_identity_over_all_pairs():
    """Exact: both quotients defined <=> the new denominator is not 0 <=> the pair is not (0,0) or (P,P); there the two sides are equal."""
    bad, undefined = [], []
    for mn, mx in PAIRS:
        n, d = min(mn, P - mx), min(mx, P - mn)
        if mx == 0 or mn == P:
            undefined.append((mn, mx))
            assert n == 0 and d == 0   # the new form is 0/0 exactly where one of the old quotients was
            continue
        assert d > 0
        old = max(Fraction(-mn, 4 * mx), Fraction(P - mx, 4 * mn - 4 * P))
        new = Fraction(-n, 4 * d)
        if old != new:
            bad.append((mn, mx))
        # the selection rule the helper's comment states
        assert ((n, d) == (mn, mx)) if mn + mx <= P else ((n, d) == (P - mx, P - mn))
    assert not bad, bad[:8]
    assert undefined == DEGENERATE


def _fp32_forms():
    """Per-channel value of both forms in fp32 (numpy float32 division is correctly rounded; every other operation here is either exact
    on these integers or a single rounded multiply, so the FMA contraction of the kernels changes nothing)."""
    mn = np.array([p[0] for p in PAIRS], np.float32)
    mx = np.array([p[1] for p in PAIRS], np.float32)
    one, four, peak = np.float32(1.0), np.float32(4.0), np.float32(P)
    with np.errstate(divide="ignore", invalid="ignore"):
        hit_min = mn * (one / (four * mx))
        hit_max = (peak - mx) * (one / (four * mn - four * peak))
        old = np.fmax(-hit_min, hit_max)                       # fmaxf: a NaN operand is dropped
        # the shipped form: the 4 folded out of the denominator (exact: a power of two), applied to the quotient afterwards
        q = np.minimum(mn, peak - mx) * (one / np.minimum(mx, peak - mn))
        new = -(q * np.float32(0.25))
    return mn, mx, old.astype(np.float32), new.astype(np.float32)


def test_fp32_forms_agree_bitwise_off_the_diagonal():
    mn, mx, old, new = _fp32_forms()
    off = mn != mx
    assert off.sum() == 32896 - 256
    diff = old[off].view(np.uint32) != new[off].view(np.uint32)
    assert not diff.any(), list(zip(mn[off][diff][:8], mx[off][diff][:8], old[off][diff][:8], new[off][diff][:8]))


def test_fp32_diagonal_is_below_the_clamp():
    """mn == mx: both forms are about -1/4, below -LIMIT = -3/16, so med3(x, -LIMIT, 0) is -LIMIT for both."""
    mn, mx, old, new = _fp32_forms()
    diag = (mn == mx) & (mn != 0) & (mn != P)
    assert diag.sum() == 254
    assert (old[diag] < -LIMIT).all() and (new[diag] < -LIMIT).all()
    assert np.abs(old[diag] + 0.25).max() < 1e-6 and np.abs(new[diag] + 0.25).max() < 1e-6


def test_fp32_degenerate_pairs():
    """(0,0) and (P,P): the old form drops its 0 * inf against the other quotient's -1/4 (the channel does not limit the lobe); the new form
    is NaN there, which the min over the channels has to drop (pinned on the device by tests/test_gpu_rcas_identity.py)."""
    mn, mx, old, new = _fp32_forms()
    for pair in DEGENERATE:
        i = PAIRS.index(pair)
        assert abs(old[i] + 0.25) < 1e-6 and old[i] < -LIMIT, (pair, old[i])
        assert np.isnan(new[i]), (pair, new[i])


# ---- the re-recorded fingerprints ---------------------------------------------------------------------------------------------

CHANGED_FAMILIES = (
    r"^void ovrfsr_fast::rcas_dpp_kernel<",             # RGBA8 input by construction
    r"^void ovrfsr_fast::rcas_direct_kernel<0, ",       # IN_FMT == FMT_RGBA8
    r"^void ovrfsr_fast::fused_kernel<\d+, 0, ",        # MID_FMT == FMT_RGBA8: the byte-domain RCAS stage
    r"^void ovrfsr_fast::easu_fast_kernel<",            # the one kernel that instantiates easu_resolve_fast2 (shared dering extrema of a pixel pair)
)


_record = isa.record


def test_fingerprint_scope():
    before = _record("rcas_one_quotient_fingerprint_before.json")
    after = _record("isa_fingerprint.json")
    assert sorted(before) == sorted(after)
    changed = sorted(k for k in before if before[k] != after[k])
    assert changed, "the one-quotient form must have changed the byte-domain RCAS kernels"
    outside = [k for k in changed if not any(re.match(p, k) for p in CHANGED_FAMILIES)]
    assert not outside, outside
    assert not [k for k in changed if "ovrfsr_strict::" in k or "nis" in k.lower()]
    # fused_kernel resolves its EASU stage without easu_resolve_fast2: only its byte-domain RCAS instances moved
    assert sum("fused_kernel" in k for k in changed) == sum(bool(re.match(CHANGED_FAMILIES[2], k)) for k in before)
    # the kernel the headline workload runs is among them, and it lost instructions
    dpp = "void ovrfsr_fast::rcas_dpp_kernel<0, false, 32>(ovrfsr::RcasArgs)"
    assert dpp in changed and after[dpp]["n"] < before[dpp]["n"], (before[dpp], after[dpp])
    # the older, shorter record moved with it: same entries re-recorded, nothing else
    r06_after = _record("r06_isa_fingerprint_r06.json")
    assert set(r06_after) <= set(after)
    assert not [k for k in r06_after if r06_after[k] != after[k]]
