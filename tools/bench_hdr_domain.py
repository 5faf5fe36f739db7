#!/usr/bin/env python3
"""OVRFSR_HDR_DOMAIN_SRTM against the default at two RGBA16F shapes, one process, one device.  Prints one JSON line.

    C5   2370^2 -> 3160^2, radius 0.5: bench.py's C5 (masked; the fused kernel beside the outside-tile kernel)
    C2h  bench.py's C2 shape, 1683x1869 -> 2244x2492, unmasked, as an RGBA16F submission (two-pass through a half intermediate)

Per shape two ctxs, one with the setting and one without, run the same ovrfsr_apply_batch of PAIRS stereo pairs; both are warmed up, then
timed with HIP events over windows of at least --window seconds, interleaved round by round (A, A', B: the ctx without the setting twice,
so that the A/A' ratio shows the spread the B/A ratio has to be read against); the figure is the median window.  Content: uniform noise
scaled to 0 ... 16 (the passes' cost does not depend on the values).

The library is the one OVRFSR_LIB names (tools/ab.sh, tools/abn.sh).  A library from before ovrfsr_set_hdr_domain -- the parent commit's,
the baseline the step without the setting is read against -- has no B: the line then holds A and A' alone (as it does for any library
with --linear-only).  Interleave the two libraries the way tools/abn.sh interleaves bench.py: for each round, one run of this script per
library.

(The CPU-only picture of why the setting exists -- a 1-texel highlight filtered as submitted and in the mapped domain, from the oracle alone --
is tests/debug/hdr_picture.py: the oracle is test infrastructure, and no tool outside tests/ imports it.)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


SHAPES = {
    "C5": (2370, 2370, 3160, 3160, 0.5),
    "C2h": (1683, 1869, 2244, 2492, 2.0),
}


def timed(torch, fn, window, est):
    """run fn k times between two events, k chosen from the estimate so that the window lasts >= `window` s; returns s per call"""
    k = max(1, int(window / max(est, 1e-6)) + 1)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--shapes", default="C5,C2h")
    ap.add_argument("--linear-only", action="store_true", help="time the ctx without the setting alone, whatever the library has (A and A': no B between the windows)")
    args = ap.parse_args()
    import torch
    import openvr_fsr_amd as A
    from openvr_fsr_amd import _capi as K
    dev = torch.device("cuda:0")
    has_setting = hasattr(A.library(), "ovrfsr_set_hdr_domain") and not args.linear_only
    rec = {"library": os.path.relpath(A.library_path(), ROOT), "has_hdr_domain": has_setting, "pairs_per_call": args.pairs, "rounds": args.rounds,
           "window_s": args.window, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name in args.shapes.split(","):
        iw, ih, ow, oh, radius = SHAPES[name]
        n = 2 * args.pairs
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        src = (torch.randint(0, 256, (n, ih, iw, 4), dtype=torch.uint8, device=dev, generator=g).to(torch.float32) * (16.0 / 255.0)).to(torch.float16)
        kw = dict(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, radius=radius)
        linear = A.PostProcessor(**kw)
        out_a = torch.zeros((n, oh, ow, 4), dtype=torch.float16, device=dev)
        variants = {"A": lambda: linear.apply_batch(src, out_a)}
        variants["A2"] = variants["A"]
        srtm = None
        if has_setting:
            srtm = A.PostProcessor(**kw)
            srtm.set_hdr_domain(K.HDR_DOMAIN_SRTM)
            out_b = torch.zeros_like(out_a)
            variants["B"] = lambda: srtm.apply_batch(src, out_b)
        for f in variants.values():
            f()
        torch.cuda.synchronize()
        if has_setting and (torch.equal(out_a.view(torch.int16), out_b.view(torch.int16)) or not bool(torch.isfinite(out_b.float()).all())):
            raise SystemExit("%s: the result with the setting equals the one without, or is not finite" % name)
        est = {k: timed(torch, f, 0.2, 1e-3) for k, f in variants.items()}   # warm-up + estimate
        res = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, f in variants.items():
                res[k].append(timed(torch, f, args.window, est[k]))
        med = {k: statistics.median(v) for k, v in res.items()}
        shape = {"shape": "%dx%d -> %dx%d float16 radius %.1f" % (iw, ih, ow, oh, radius),
                 "step_ms": {k: round(v * 1e3, 4) for k, v in med.items()}, "none_over_none_time": round(med["A2"] / med["A"], 4),
                 "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in res.items()}}
        if has_setting:
            shape["srtm_over_linear_time"] = round(med["B"] / med["A"], 4)
            # what the three added passes move per image: read in + write mapped, (pipeline), read result + write out
            extra = ih * iw * (8 + 16) + oh * ow * (16 + 8)
            shape["added_bytes_per_image"] = extra
            shape["added_ms_per_call"] = round((med["B"] - med["A"]) * 1e3, 4)
            shape["added_passes_GBps"] = round(extra * n / max(med["B"] - med["A"], 1e-9) / 1e9, 1)
            srtm.close()
        rec["shapes"][name] = shape
        linear.close()
        del src, out_a
        torch.cuda.empty_cache()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
