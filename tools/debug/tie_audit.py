#!/usr/bin/env python3
"""tools/debug/tie_audit.py -- drive an AUDIT build of the library (tools/build_variant.sh audit "-DOVRFSR_TIE_AUDIT") over a content campaign.

The product build claims that its quantised EASU stores (the UNORM8 / half intermediate, an EASU-only UNORM8 output) are the strict build's:
pixels whose re-associated result lies within the near-tie band of a rounding boundary are re-resolved in the reference's operator order, all
others are stored as they are.  The audit build re-resolves EVERY pixel in reference order inside the same kernels and counts, on the device,
the pixels that were NOT listed by the guard and whose stored value differs from the strict build's ("flips"): the claim is flips == 0.
It also records the largest |product - strict| it met (bytes of the UNORM8 domain; half spacings for half stores): the band is 2^-9 byte /
2^-6 spacing.

    OVRFSR_LIB=$PWD/ab/audit.so python tools/debug/tie_audit.py [scale=1.0] [seed_offset=0]      (GPU; `scale` multiplies the images per
    configuration, `seed_offset` moves every generator seed: a further campaign on content no earlier one saw)

Content: natural images (round 6: tests/golden/natural_*.npz, mirror-tiled), the bench's structured and uniform-random generators, 0 / 255-heavy images, and a mosaic of 8x8-texel patches of the families the
adversarial search (tools/debug/easu_err_search.py) mutates -- two-level edges at random angles, ramps with noise, near-constant patches with
outliers, extremes --; for the half pipelines the same content as half(b / 255 * s), s in {1, 6, 40} (unit range and HDR).
Shapes: BASELINE C2 (x4/3), C4 (x1.3), C5 (x4/3, masked and unmasked, half), and odd ratios (x1.7, x1.11, x2).

    OVRFSR_LIB=$PWD/ab/audit.so python tools/debug/tie_audit.py --reference-formats [scale=1.0] [seed_offset=0]

runs ONLY the campaign of cfg.reference_formats = 1 (the default campaign, whose totals tests/test_gpu_adversarial.py asserts, holds none of
it): UNORM8 stores of FLOAT sources -- the UNORM8 intermediate of an RGBA16F / RGBA32F pipeline and the EASU-only RGBA8 output -- on unit-range
content and every HDR kind of tests/test_gpu_formats.py::_hdr_image (the structured image scaled x2 / x6 / x40; a dark image with 2 % highlights
at x6 / x40 / x400), masked (mask-sorted form, radius 0.5) and unmasked, at the three LDS pitches of easu_fast_kernel (28: x4/3, 32: x1.3,
40: x1.11).  The guard's band there is 2^-9 byte x max(1, largest texel of the tile's footprint): the distance is reported as a fraction of
the band of the pixel it was met at.

    OVRFSR_LIB=$PWD/ab/audit.so python tools/debug/tie_audit.py --rcas [scale=1.0] [seed_offset=0]

runs ONLY the campaign of OVRFSR_PRECISION_FP32_EXACT (exact stores): the guarded RCAS instances re-evaluate every stored pixel in the
reference's operator order and count the unlisted ones whose product byte differs.  Structured, uniform-random and natural content and the
tie-rich fixture (tests/rcas_ties.py); sharpness 0, 0.5, 0.9 and 1; the unmasked pipeline, the mask-sorted one (radius 0.5: span records) and
RCAS alone; each as one image per call and as a batch, so that rcas_dpp_kernel runs in its 16-row and its 32-row form.  BASELINE's C2 shape at
scale >= 1, a quarter of it per axis below.  The largest |product - reference-order| distance this prints at scale 1 is what the band
(kRcasTieBits, fsr_kernels.inc) is derived from: the smallest power of two that is at least 3 times it (profiles/exact_stores.txt)."""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import openvr_fsr_amd as A  # noqa: E402

DEV = torch.device("cuda")


def counters(reset=False):
    lib = A.library()
    fn = lib.ovrfsr_debug_tie_audit      # AttributeError: not an audit build
    fn.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    buf = (ctypes.c_ulonglong * 6)()
    assert fn(buf, 1 if reset else 0) == 0
    v = list(buf)
    f = lambda bits: float(np.uint32(bits & 0xffffffff).view(np.float32))  # noqa: E731
    return {"audited": v[0], "listed": v[1], "flips": v[2], "small_half_diffs": v[3], "max_dist_bytes": f(v[4]), "max_dist_half_spacings": f(v[5])}


def extremes_batch(n, w, h, seed):
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    vals = torch.tensor([0, 0, 255, 255, 1, 254, 128], dtype=torch.uint8, device=DEV)
    out = vals[torch.randint(0, 7, (n, h, w, 4), generator=g, device=DEV)]
    out[..., 3] = 255
    return out


def mosaic_batch(n, w, h, seed, P=8):
    """every 8x8-texel patch from one of the adversarial search's families, chosen at random"""
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    ph, pw = (h + P - 1) // P, (w + P - 1) // P
    r = lambda *shape: torch.rand(shape, generator=g, device=DEV)  # noqa: E731
    ri = lambda lo, hi, *shape: torch.randint(lo, hi, shape, generator=g, device=DEV)  # noqa: E731
    yy = (torch.arange(ph * P, device=DEV) % P).float()[None, :, None, None] - P / 2
    xx = (torch.arange(pw * P, device=DEV) % P).float()[None, None, :, None] - P / 2
    up = lambda t: t.repeat_interleave(P, 1).repeat_interleave(P, 2)  # noqa: E731  -- per-patch value -> per-texel
    fam = up(ri(0, 5, n, ph, pw, 1))
    # two levels split by a random line
    th = up(r(n, ph, pw, 1) * 3.14159)
    side = (torch.cos(th) * (xx + up(r(n, ph, pw, 1) * 2 - 1)) + torch.sin(th) * (yy + up(r(n, ph, pw, 1) * 2 - 1))) > 0
    two = torch.where(side, up(ri(0, 256, n, ph, pw, 3)).float(), up(ri(0, 256, n, ph, pw, 3)).float())
    # ramp + noise
    ramp = up(ri(0, 256, n, ph, pw, 3)).float() + up(r(n, ph, pw, 1) * 60 - 30) * xx + up(r(n, ph, pw, 1) * 60 - 30) * yy + ri(-4, 5, n, ph * P, pw * P, 3).float()
    # near-constant with outliers
    flat = up(ri(0, 40, n, ph, pw, 1)).float() + ri(0, 3, n, ph * P, pw * P, 3).float()
    flat = torch.where(r(n, ph * P, pw * P, 1) < 0.05, ri(200, 256, n, ph * P, pw * P, 1).float().expand(-1, -1, -1, 3), flat)
    ext = (ri(0, 2, n, ph * P, pw * P, 3) * 255).float()
    rnd = ri(0, 256, n, ph * P, pw * P, 3).float()
    img = torch.where(fam == 0, two, torch.where(fam == 1, ramp, torch.where(fam == 2, flat, torch.where(fam == 3, ext, rnd))))
    out = torch.empty((n, h, w, 4), dtype=torch.uint8, device=DEV)
    out[..., :3] = img[:, :h, :w].clamp_(0, 255).to(torch.uint8)
    out[..., 3] = 255
    return out


CONTENT = {
    # round 6: NATURAL content -- the fixtures of tests/golden/natural_*.npz (rendered game art, a rendered UI with text, a photograph), mirror-tiled
    "natural": lambda n, w, h, s: bench.natural_batch(n, w, h, torch.uint8, DEV, s),
    "structured": lambda n, w, h, s: bench.synth_batch(n, w, h, torch.uint8, DEV, s),
    "random": lambda n, w, h, s: bench.random_batch(n, w, h, torch.uint8, DEV, s),
    "extremes": extremes_batch,
    "mosaic": mosaic_batch,
}


def run(tag, inW, inH, outW, outH, content, n, seed, half_scale=None, **cfg):
    texs = CONTENT[content](n, inW, inH, seed)
    if half_scale is not None:
        texs = (texs.float() * (half_scale / 255.0)).to(torch.float16)
        texs[..., 3] = 1.0
    outs = torch.empty((n, outH, outW, 4), dtype=texs.dtype, device=DEV)
    pp = A.PostProcessor(fsr_enabled=1, out_width=outW, out_height=outH, sharpness=0.9, quantize_intermediate=1, **cfg)
    counters(reset=True)
    pp.apply_batch(texs, outs, first_eye=A.EYE_LEFT, alternate_eyes=True)
    torch.cuda.synchronize()
    c = counters()
    pp.close()
    print("%-58s %-10s n=%3d  audited %12d  listed %9d (%.2f %%)  FLIPS %d  small-channel half diffs %d  max dist %.3e byte  %.3e half spacings"
          % (tag, content + ("" if half_scale is None else " x%g" % half_scale), n, c["audited"], c["listed"], 100.0 * c["listed"] / max(1, c["audited"]),
             c["flips"], c["small_half_diffs"], c["max_dist_bytes"], c["max_dist_half_spacings"]), flush=True)
    return c


def hdr_batch(n, w, h, seed, scale, kind, dtype):
    """tests/test_gpu_formats.py::_hdr_image on the device: the structured generator scaled as a whole, or a dark image (values <= 1) with
    2 % of its texels at scale x U(0.5, 1)"""
    img = bench.synth_batch(n, w, h, torch.uint8, DEV, seed).float() / 255.0
    if kind == "scaled":
        img = img * scale
    else:
        g = torch.Generator(device=DEV); g.manual_seed(seed ^ 0x9E3779B9)
        hot = torch.rand((n, h, w, 1), generator=g, device=DEV) < 0.02
        lit = scale * (0.5 + 0.5 * torch.rand((n, h, w, 4), generator=g, device=DEV))
        img = torch.where(hot, lit, img)
    img = img.to(torch.float16).to(dtype)   # (RGBA32F images hold half-representable values too: one content, two staging paths)
    img[..., 3] = 1.0
    return img


def run_reference_formats(tag, inW, inH, outW, outH, n, seed, scale, kind, dtype, **cfg):
    texs = hdr_batch(n, inW, inH, seed, scale, kind, dtype)
    outs = torch.empty((n, outH, outW, 4), dtype=torch.uint8, device=DEV)
    pp = A.PostProcessor(fsr_enabled=1, out_width=outW, out_height=outH, sharpness=0.9, quantize_intermediate=1, reference_formats=1, **cfg)
    counters(reset=True)
    pp.apply_batch(texs, outs, first_eye=A.EYE_LEFT, alternate_eyes=True)
    torch.cuda.synchronize()
    c = counters()
    pp.close()
    print("%-44s %-16s %-7s n=%3d  audited %11d  listed %10d (%6.2f %%)  FLIPS %d  max dist %.3f of the band"
          % (tag, "%s x%g" % (kind, scale), str(dtype).split(".")[-1], n, c["audited"], c["listed"], 100.0 * c["listed"] / max(1, c["audited"]), c["flips"],
             c["max_dist_half_spacings"]), flush=True)   # (slot [5] holds band fractions for these stores: tie_audit_px<.., UNIT8>)
    return c


def main_reference_formats(argv):
    k = float(argv[0]) if argv else 1.0
    N = lambda n: max(2, int(round(n * k)) & ~1)  # noqa: E731
    seed = 0x5EED0000 + (int(argv[1], 0) if len(argv) > 1 else 0)
    total = {"audited": 0, "listed": 0, "flips": 0, "dist": 0.0}
    t0 = time.time()
    shapes = ((1683, 1869, 2244, 2492, "x4/3 pitch 28"), (1000, 900, 1300, 1170, "x1.3 pitch 32"), (1000, 900, 1111, 1000, "x1.11 pitch 40"))
    kinds = ((1.0, "scaled"), (2.0, "scaled"), (6.0, "scaled"), (40.0, "scaled"), (6.0, "highlights"), (40.0, "highlights"), (400.0, "highlights"))
    i = 0
    for (iw, ih, ow, oh, name) in shapes:
        for (scale, kind) in kinds:
            for (form, cfg) in (("two-pass", dict(radius=2.0)), ("mask-sorted", dict(radius=0.5)), ("EASU only", dict(radius=2.0, stage_mask=1))):
                seed += 1000
                i += 1
                dtype = torch.float32 if i % 3 == 0 else torch.float16
                c = run_reference_formats("%s %s" % (name, form), iw, ih, ow, oh, N(4), seed, scale, kind, dtype, **cfg)
                for key in ("audited", "listed", "flips"):
                    total[key] += c[key]
                total["dist"] = max(total["dist"], c["max_dist_half_spacings"])
    print("TOTAL audited %d pixels, listed %d (%.2f %%), FLIPS %d, max |product - strict| %.3f of the band (2^-9 byte x max(1, tile maximum))   [%.0f s]"
          % (total["audited"], total["listed"], 100.0 * total["listed"] / max(1, total["audited"]), total["flips"], total["dist"], time.time() - t0))
    sys.exit(1 if total["flips"] else 0)


def counters_rcas(reset=False):
    fn = A.library().ovrfsr_debug_tie_audit_rcas      # AttributeError: not an audit build
    fn.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    buf = (ctypes.c_ulonglong * 5)()
    assert fn(buf, 1 if reset else 0) == 0
    v = list(buf)
    return {"audited": v[0], "listed": v[1], "flips": v[2], "dist": float(np.uint32(v[3] & 0xffffffff).view(np.float32)), "band_bits": v[4]}


def dpp_rows(ow, oh, n):
    """rows per workgroup rcas_dpp_kernel takes for an unmasked launch of n images (fsr_sizes.h, rcas_dpp_small)"""
    wgs = ((ow + 61) // 62) * ((oh + 31) // 32) * n
    full, half = (wgs + 2047) // 2048, (2 * wgs + 2047) // 2048
    return 16 if wgs < 16 * 2048 and 103 * half < 200 * full else 32


def run_rcas(tag, texs, outW, outH, content, sharp, **cfg):
    n = texs.shape[0]
    outs = torch.empty((n, outH, outW, 4), dtype=torch.uint8, device=DEV)
    pp = A.PostProcessor(fsr_enabled=1, out_width=outW, out_height=outH, sharpness=sharp, precision=A.PRECISION_FP32_EXACT, **cfg)
    counters_rcas(reset=True)
    pp.apply_batch(texs, outs, first_eye=A.EYE_LEFT, alternate_eyes=True)
    torch.cuda.synchronize()
    c = counters_rcas()
    pp.close()
    print("%-34s %-10s sharp %-4g n=%3d  audited %11d  listed %9d (%6.3f %%)  FLIPS %d  max dist %.3e byte"
          % (tag, content, sharp, n, c["audited"], c["listed"], 100.0 * c["listed"] / max(1, c["audited"]), c["flips"], c["dist"]), flush=True)
    return c


def main_rcas(argv):
    from tests import rcas_ties
    k = float(argv[0]) if argv else 1.0
    seed = 0x5EED0000 + (int(argv[1], 0) if len(argv) > 1 else 0)
    iw, ih, ow, oh = (1683, 1869, 2244, 2492) if k >= 1.0 else (420, 467, 560, 623)
    want = max(2, int(round(8 * k)) & ~1)
    n32 = next(n for n in range(want, want + 64, 2) if dpp_rows(ow, oh, n) == 32)   # a batch that takes the 32-row form
    assert dpp_rows(ow, oh, 1) == 16
    total = {"audited": 0, "listed": 0, "flips": 0, "dist": 0.0}
    per = {}
    t0 = time.time()

    def acc(content, c):
        p = per.setdefault(content, [0, 0])
        p[0] += c["audited"]; p[1] += c["listed"]
        for key in ("audited", "listed", "flips"):
            total[key] += c[key]
        total["dist"] = max(total["dist"], c["dist"])
        total["band_bits"] = c["band_bits"]

    for content in ("structured", "random", "natural"):
        for sharp in (0.0, 0.5, 0.9, 1.0):
            for n, rows in ((1, 16), (n32, 32)):
                seed += 1000
                acc(content, run_rcas("pipeline unmasked, %d-row" % rows, CONTENT[content](n, iw, ih, seed), ow, oh, content, sharp, radius=2.0))
                acc(content, run_rcas("RCAS only, %d-row" % rows, CONTENT[content](n, ow, oh, seed + 1), ow, oh, content, sharp, radius=2.0, stage_mask=2))
            seed += 1000
            acc(content, run_rcas("pipeline radius 0.5 (spans)", CONTENT[content](n32, iw, ih, seed), ow, oh, content, sharp, radius=0.5))
            acc(content, run_rcas("RCAS only radius 0.5", CONTENT[content](2, ow, oh, seed + 1), ow, oh, content, sharp, radius=0.5, stage_mask=2))
    fix = torch.from_numpy(np.ascontiguousarray(rcas_ties.fixture(7)[0])).to(DEV)
    S = rcas_ties.SIZE
    assert dpp_rows(S, S, 1) == 16 and dpp_rows(S, S, 192) == 32
    for sharp in (0.0, 0.5, 0.9, 1.0):
        for n in (1, 192):
            acc("tie-rich", run_rcas("RCAS only, %d-row" % dpp_rows(S, S, n), fix[None].expand(n, -1, -1, -1).contiguous(), S, S, "tie-rich", sharp, radius=2.0, stage_mask=2))
    band = 2.0 ** -total["band_bits"]
    for content, (a, l) in per.items():
        print("LISTED %-10s %.4f %% of %d pixels (band 2^-%d byte)" % (content, 100.0 * l / max(1, a), a, total["band_bits"]))
    print("TOTAL audited %d pixels, listed %d (%.3f %%), FLIPS %d, max |product - reference-order| %.3e byte = %.3f of the band (2^-%d byte)   [%.0f s]"
          % (total["audited"], total["listed"], 100.0 * total["listed"] / max(1, total["audited"]), total["flips"], total["dist"], total["dist"] / band,
             total["band_bits"], time.time() - t0))
    sys.exit(1 if total["flips"] else 0)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--reference-formats":
        return main_reference_formats(sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "--rcas":
        return main_rcas(sys.argv[2:])
    k = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    N = lambda n: max(2, int(round(n * k)) & ~1)  # noqa: E731
    total = {"audited": 0, "listed": 0, "flips": 0, "small_half_diffs": 0, "max_dist_bytes": 0.0, "max_dist_half_spacings": 0.0}

    def acc(c):
        for key in ("audited", "listed", "flips", "small_half_diffs"):
            total[key] += c[key]
        for key in ("max_dist_bytes", "max_dist_half_spacings"):
            total[key] = max(total[key], c[key])

    t0 = time.time()
    seed = 0x5EED0000 + (int(sys.argv[2], 0) if len(sys.argv) > 2 else 0)
    C2 = (1683, 1869, 2244, 2492)
    for content in ("structured", "random", "extremes", "mosaic", "natural"):
        for rep in range(2):
            seed += 1000
            acc(run("C2 two-pass RGBA8 (easu_fast_kernel -> UNORM8 intermediate)", *C2, content, N(24), seed, radius=2.0))
    for content in ("structured", "mosaic", "random", "natural"):
        seed += 1000
        acc(run("C2 fused=1 (fused_kernel, UNORM8 plane)", *C2, content, N(8), seed, radius=2.0, fused=1))
        seed += 1000
        acc(run("C2r masked sorted (radius 0.5)", *C2, content, N(16), seed, radius=0.5))
        seed += 1000
        acc(run("C2 EASU only -> UNORM8 output", *C2, content, N(8), seed, radius=2.0, stage_mask=1))
    for content in ("structured", "mosaic", "random", "natural"):
        seed += 1000
        acc(run("C4 x1.3 two-pass RGBA8", 2244, 2492, 2916, 3240, content, N(8), seed, radius=2.0))
    for (iw, ih, ow, oh, name) in ((1000, 900, 1695, 1525, "x1.7"), (1000, 900, 1111, 1000, "x1.11"), (1000, 900, 2000, 1800, "x2"), (997, 811, 1329, 1081, "x4/3 odd")):
        for content in ("mosaic", "random"):
            seed += 1000
            acc(run("odd ratio %s two-pass RGBA8" % name, iw, ih, ow, oh, content, N(16), seed, radius=2.0))
    C5 = (2370, 2370, 3160, 3160)
    for hs in (1.0, 6.0, 40.0):
        for content in ("structured", "mosaic", "random", "natural"):
            seed += 1000
            acc(run("C5 masked half pipeline (fused_kernel, half plane)", *C5, content, N(6), seed, half_scale=hs, radius=0.5))
            seed += 1000
            acc(run("C5 shape unmasked two-pass half (easu_fast_kernel -> half)", *C5, content, N(2), seed, half_scale=hs, radius=2.0, fused=0))
    print("TOTAL audited %d pixels, listed %d (%.2f %%), FLIPS %d, small-channel half differences %d (outside the contract: below xmin), "
          "max |product - strict| %.3e byte = %.2f of the 2^-9 band, %.3e half spacings = %.2f of the 2^-6 band   [%.0f s]"
          % (total["audited"], total["listed"], 100.0 * total["listed"] / max(1, total["audited"]), total["flips"], total["small_half_diffs"],
             total["max_dist_bytes"], total["max_dist_bytes"] * 512.0, total["max_dist_half_spacings"], total["max_dist_half_spacings"] * 64.0, time.time() - t0))
    sys.exit(1 if total["flips"] else 0)


if __name__ == "__main__":
    main()
