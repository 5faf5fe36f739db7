"""The one-quotient RCAS lobe (fsr_device.inc: rcas_lobe_bytes) against the two-quotient form it replaces, on the device.

tests/test_rcas_identity.py shows the identity in exact arithmetic and with a correctly rounded reciprocal; v_rcp_f32 is neither, and the
helper leans on v_min3_f32 / v_med3_f32 dropping a NaN, so the claim "the clamped lobe is the same bit pattern" is settled here:
  * tests/debug/rcas_lobe_probe.hip is compiled at test time; it restates the old form beside a call of the shipped helper and evaluates both
    for every case of a table this test writes -- all 32 896 (mn, mx) byte pairs, for sharpness 0, 0.9 and 1, in every channel position and in
    mixed triples, and the pairs with a zero denominator, (0,0) and (255,255), in one, two and all three channels;
  * images that are all 0, all 255 or saturated in one channel go through RCAS alone and through EASU + RCAS (separate kernels, fused
    kernel, masked) and are compared with the oracle: <= 1 LSB, the tolerance of every UNORM8 RCAS output (tests/test_gpu_parity.py).
The probe is one child process under its own `timeout`, started only if its compilation succeeded (`&&`)."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests import synth
from tests.util import run_gpu, lsb_stats

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openvr_fsr_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
P = 255
PAIRS = np.array([(mn, mx) for mx in range(P + 1) for mn in range(mx + 1)], np.float32)
DEGENERATE = [(0.0, 0.0), (255.0, 255.0)]
REGULAR = [(0.0, 255.0), (10.0, 200.0), (100.0, 120.0), (0.0, 1.0), (254.0, 255.0), (127.0, 128.0), (3.0, 3.0), (250.0, 250.0), (0.0, 128.0)]
SHARPNESS = (0.0, 0.9, 1.0)
LIMIT = np.float32(0.25 - 1.0 / 16.0)


def _sharp(sharpness):
    """The factor the kernels multiply the lobe with: FsrRcasCon's const0[0] for this sharpness setting."""
    return O.rcas_con(sharpness)[:1].view(np.float32)[0]


def _pair_cases():
    """[n, 6]: every pair in all three channels; in one channel beside two channels that never limit; in pseudo-random triples."""
    n = len(PAIRS)
    idle = np.tile(np.array([127.0, 128.0], np.float32), (n, 1))   # quotient 127/128: limits nothing below the clamp
    g = PAIRS[(np.arange(n) * 7919 + 13) % n]
    b = PAIRS[(np.arange(n) * 104729 + 71) % n]
    return np.concatenate([np.hstack([PAIRS, PAIRS, PAIRS]), np.hstack([PAIRS, idle, idle]), np.hstack([idle, PAIRS, idle]),
                           np.hstack([idle, idle, PAIRS]), np.hstack([PAIRS, g, b]), np.hstack([b, PAIRS, g])])


def _degenerate_cases():
    """[n, 6] and the number of degenerate channels of each row: (0,0) / (255,255) in one, two and all three channels, every regular pair in
    the others."""
    rows, count = [], []
    for mask in range(1, 8):
        slots = [DEGENERATE if (mask >> c) & 1 else REGULAR for c in range(3)]
        for r in slots[0]:
            for g in slots[1]:
                for b in slots[2]:
                    rows.append(r + g + b)
                    count.append(bin(mask).count("1"))
    return np.array(rows, np.float32), np.array(count)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """Compile the probe, then run it once over the whole table: (cases [n,8] float32, degenerate channels per row [n], results [n,2] uint32)."""
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not installed: the probe kernel cannot be compiled")
    d = tmp_path_factory.mktemp("rcas_probe")
    pairs, (deg, deg_n) = _pair_cases(), _degenerate_cases()
    body = np.concatenate([pairs, deg])
    ndeg = np.concatenate([np.zeros(len(pairs), int), deg_n])
    cases = np.zeros((len(body) * len(SHARPNESS), 8), np.float32)
    for i, s in enumerate(SHARPNESS):
        cases[i * len(body):(i + 1) * len(body), :6] = body
        cases[i * len(body):(i + 1) * len(body), 6] = _sharp(s)
    ndeg = np.tile(ndeg, len(SHARPNESS))
    cases.tofile(str(d / "cases.bin"))
    exe, out = str(d / "rcas_lobe_probe"), str(d / "out.bin")
    # the kernel translation units' flags (csrc/Makefile); the two GPU-free and GPU steps chained, the GPU step under its own time limit
    cmd = ("%s --offload-arch=gfx950 -O3 -std=c++17 -Wall -Wno-unused-function -ffp-contract=on -fno-slp-vectorize -I%s %s -o %s"
           " && timeout -k 10 120 %s %s %s" % (HIPCC, CSRC, os.path.join(ROOT, "tests", "debug", "rcas_lobe_probe.hip"), exe, exe, str(d / "cases.bin"), out))
    r = subprocess.run(cmd, shell=True, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    res = np.fromfile(out, np.uint32).reshape(-1, 2)
    assert len(res) == len(cases)
    return cases, ndeg, res


def _report(cases, res, sel):
    bad = sel & (res[:, 0] != res[:, 1])
    return [(tuple(cases[i, :7]), hex(res[i, 0]), hex(res[i, 1])) for i in np.flatnonzero(bad)[:8]], int(bad.sum())


def test_probe_covers_every_pair_and_sharpness(probe):
    cases, ndeg, res = probe
    assert len(PAIRS) == 32896
    for s in SHARPNESS:
        rows = cases[(cases[:, 6] == _sharp(s)) & (ndeg == 0)]
        assert len(rows) == 6 * 32896
        assert len(np.unique(rows[:32896, :2], axis=0)) == 32896
    assert _sharp(1.0) == 1.0 and _sharp(0.0) == 0.25


def test_lobe_is_bitwise_the_two_quotient_lobe_over_all_pairs(probe):
    cases, ndeg, res = probe
    first, n = _report(cases, res, ndeg == 0)
    print("pair cases: %d, differing %d" % (int((ndeg == 0).sum()), n))
    assert n == 0, first
    lobe = res[:, 1].view(np.float32)
    assert not np.isnan(lobe).any()
    assert (lobe <= 0).all() and (lobe >= -LIMIT * cases[:, 6]).all()


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_degenerate_channels_do_not_limit(probe, channels):
    """A channel with mn = mx in {0, 255} computes 0 * rcp(0) = NaN in the one-quotient form: it must leave the lobe to the other channels, and
    with all three channels degenerate the lobe is the clamp itself, -LIMIT * sharp -- as the two-quotient form answers."""
    cases, ndeg, res = probe
    sel = ndeg == channels
    assert sel.sum() > 0
    first, n = _report(cases, res, sel)
    print("%d degenerate channel(s): %d cases, differing %d" % (channels, int(sel.sum()), n))
    assert n == 0, first
    if channels == 3:
        want = (-LIMIT * cases[sel, 6]).astype(np.float32)
        assert np.array_equal(res[sel, 1], want.view(np.uint32))


# ---- saturated images against the oracle ---------------------------------------------------------------------------------------

def _images(w, h):
    rnd = synth.random_u8(w, h, 5)
    out = {"all0": np.zeros((h, w, 4), np.uint8), "all255": np.full((h, w, 4), 255, np.uint8)}
    for c, name in enumerate("RGB"):
        for v in (0, 255):
            img = rnd.copy()
            img[..., c] = v
            out["%s=%d" % (name, v)] = img
    for img in out.values():
        img[..., 3] = 255
    return out


IMAGES = sorted(_images(8, 8))


@pytest.mark.parametrize("sharpness", [0.9, 1.0])
@pytest.mark.parametrize("name", IMAGES)
def test_rcas_only_saturated_images(gpu, name, sharpness):
    w, h = 200, 83   # more than three 62-column waves wide, ragged in both directions
    img8 = _images(w, h)[name]
    centre, rad = O.mask_constants(w, h, 2.0, (0.5, 0.5, 0.5, 0.5), True, 0)
    want = O.float_to_unorm8(O.rcas(O.unorm8_to_float(img8), O.rcas_con(sharpness, 0), centre, rad))
    got = run_gpu(img8, w, h, np.uint8, render_scale=1.0, sharpness=sharpness)
    mx, frac = lsb_stats(got[..., :3], want[..., :3])
    print("rcas only %s sharpness %.1f: max %d LSB, differing %.5f" % (name, sharpness, mx, frac))
    assert mx <= 1, (mx, frac)


@pytest.mark.parametrize("fused,radius", [(0, 2.0), (1, 2.0), (0, 0.6)])
@pytest.mark.parametrize("name", IMAGES)
def test_pipeline_saturated_images(gpu, name, fused, radius):
    iw, ih, ow, oh = 150, 120, 200, 160
    img8 = _images(iw, ih)[name]
    want = O.fsr_pipeline_u8(img8, ow, oh, sharpness=0.9, radius=radius)
    got = run_gpu(img8, ow, oh, np.uint8, sharpness=0.9, radius=radius, fused=fused)
    mx, frac = lsb_stats(got, want)
    print("pipeline %s fused %d radius %.1f: max %d LSB, differing %.5f" % (name, fused, radius, mx, frac))
    assert mx <= 1, (mx, frac)
