#!/usr/bin/env python3
"""OVRFSR_PRECISION_FP32_EXACT (exact stores) against the product build (precision 0) and the strict build (precision 2), one process, one
device.  Prints one JSON line per (shape, pairs per call).

Shapes: C2 (1683x1869 -> 2244x2492, unmasked), C2r (the same, radius 0.5: mask-sorted form) and C2s (2244x2492, RCAS only); sharpness 0.9;
64 stereo pairs per apply_batch call, and one pair per call; content: the bench's structured, natural or uniform-random generator
(--content).  The variants are warmed up, then timed with HIP events over windows of at least --window seconds, interleaved round by
round -- p0, p3, p2 and a second ctx of precision 0 ("p0b"): the A/A pair whose ratio is the spread every other ratio is read against.
The figure is the median window.  `rcas_us_per_eye`: RCAS's own launch, timed the same way on a ctx with stage_mask = 2 at the output size
(for C2r with the mask: the per-lane kernel, not the span form the pipeline takes).

The mode's one condition: p3's C2 step takes less time than p2's in the same run (`p3_faster_than_p2`)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"C2": (1683, 1869, 2244, 2492, 2.0, 0), "C2r": (1683, 1869, 2244, 2492, 0.5, 0), "C2s": (2244, 2492, 2244, 2492, 2.0, 2)}


def timed(fn, window, est):
    """run fn k times between two events, k chosen from the estimate so that the window lasts >= `window` s; returns s per call"""
    import torch
    k = max(1, int(window / max(est, 1e-6)) + 1)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / k


def interleaved(variants, args):
    est = {k: timed(f, 0.05 if args.quick else 0.2, 1e-3) for k, f in variants.items()}  # warm-up + estimate
    res = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, f in variants.items():
            res[k].append(timed(f, args.window, est[k]))
    return {k: statistics.median(v) for k, v in res.items()}, {k: (max(v) - min(v)) / statistics.median(v) for k, v in res.items()}


def run_shape(name, pairs, args, dev):
    import torch
    import bench
    import openvr_fsr_amd as A
    iw, ih, ow, oh, radius, stage_mask = SHAPES[name]
    n = 2 * pairs
    gen = {"structured": bench.synth_batch, "natural": bench.natural_batch, "random": bench.random_batch}[args.content]
    texs = gen(n, iw, ih, torch.uint8, dev, 0x5EED0000)
    outs = torch.empty((n, oh, ow, 4), dtype=torch.uint8, device=dev)
    kw = dict(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, radius=radius, stage_mask=stage_mask)
    pps = {"p0": A.PostProcessor(precision=0, **kw), "p3": A.PostProcessor(precision=3, **kw), "p2": A.PostProcessor(precision=2, **kw),
           "p0b": A.PostProcessor(precision=0, **kw)}
    med, spread = interleaved({k: (lambda pp=pp: pp.apply_batch(texs, outs)) for k, pp in pps.items()}, args)
    for pp in pps.values():
        pp.close()
    # RCAS's own launch: the sharpen stage alone on an image of the output size
    mids = gen(n, ow, oh, torch.uint8, dev, 0x5EED0001)
    kw.update(stage_mask=2)
    rps = {"p0": A.PostProcessor(precision=0, **kw), "p3": A.PostProcessor(precision=3, **kw), "p0b": A.PostProcessor(precision=0, **kw)}
    rmed, _ = interleaved({k: (lambda pp=pp: pp.apply_batch(mids, outs)) for k, pp in rps.items()}, args)
    for pp in rps.values():
        pp.close()
    rec = {
        "shape": "%s: %dx%d -> %dx%d, radius %g%s" % (name, iw, ih, ow, oh, radius, ", RCAS only" if stage_mask == 2 else ""),
        "content": args.content, "pairs_per_call": pairs, "rounds": args.rounds, "window_s": args.window,
        "us_per_eye": {k: round(v / n * 1e6, 3) for k, v in med.items()},
        "p3_over_p0": round(med["p3"] / med["p0"], 4), "p2_over_p0": round(med["p2"] / med["p0"], 4),
        "aa_p0b_over_p0": round(med["p0b"] / med["p0"], 4), "p3_faster_than_p2": bool(med["p3"] < med["p2"]),
        "spread": {k: round(v, 4) for k, v in spread.items()},
        "rcas_us_per_eye": {k: round(v / n * 1e6, 3) for k, v in rmed.items()},
        "rcas_p3_over_p0": round(rmed["p3"] / rmed["p0"], 4), "rcas_aa_p0b_over_p0": round(rmed["p0b"] / rmed["p0"], 4),
        "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="64,1", help="stereo pairs per call, comma-separated")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--shapes", default="C2,C2r,C2s")
    ap.add_argument("--content", default="structured", choices=("structured", "natural", "random"))
    ap.add_argument("--quick", action="store_true", help="one short round")
    args = ap.parse_args()
    if args.quick:
        args.rounds, args.window = 1, 0.05
    import torch
    dev = torch.device("cuda:0")
    ok = True
    for name in args.shapes.split(","):
        for pairs in (int(p) for p in args.pairs.split(",")):
            rec = run_shape(name, pairs, args, dev)
            if name == "C2":
                ok = ok and rec["p3_faster_than_p2"]
            torch.cuda.empty_cache()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
