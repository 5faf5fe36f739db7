#!/usr/bin/env python3
"""A hidden-area mesh against no mesh at the C2, C2r and C5 shapes (bench.py's), one process, one device.  Prints one JSON line.

The mesh is SYNTHETIC -- no headset mesh exists on the machines this runs on --: four corner wedges per eye, right triangles with legs of
--wedge (default 0.30: a sixth of the tiles, what headsets typically hide) of the image's width and height, the same for both eyes.  The line states the share of tiles it hides.

Per shape two ctxs, one with the mesh and one without, run the same ovrfsr_apply_batch of PAIRS stereo pairs; both are warmed up, then
timed with HIP events over windows of at least --window seconds, interleaved round by round (A, A', B: the ctx without a mesh twice, so
that the A/A' ratio shows the spread the A/B ratio has to be read against); the figure is the median window.  Before timing, the outputs
are compared: equal outside the skipped tiles, untouched inside them.  EASU's own kernel time comes from a separate kernel-trace run
(--only none / --only mesh: ten calls of one variant per shape, so that the trace's per-kernel totals belong to that variant).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import openvr_fsr_amd as A  # noqa: E402
from openvr_fsr_amd import _capi as K  # noqa: E402

# bench.py's WORKLOADS: input and output size, dtype, radius
SHAPES = {
    "C2": (1683, 1869, 2244, 2492, torch.uint8, 2.0),
    "C2r": (1683, 1869, 2244, 2492, torch.uint8, 0.5),
    "C5": (2370, 2370, 3160, 3160, torch.float16, 0.5),
}


def corner_wedges(a):
    return np.asarray([[(0, 0), (a, 0), (0, a)], [(1, 0), (1 - a, 0), (1, a)], [(0, 1), (a, 1), (0, 1 - a)], [(1, 1), (1 - a, 1), (1, 1 - a)]], np.float32)


def timed(fn, window, est):
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
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--wedge", type=float, default=0.30)
    ap.add_argument("--shapes", default="C2,C2r,C5")
    ap.add_argument("--only", choices=["none", "mesh"], default=None,
                    help="launch the ctx without / with the mesh alone, ten calls per shape, no comparison: the kernel-trace runs, one per variant")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    mesh = corner_wedges(args.wedge)
    rec = {"mesh": "synthetic: four corner wedges per eye, legs %.2f of width / height" % args.wedge, "pairs_per_call": args.pairs,
           "rounds": args.rounds, "window_s": args.window, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name in args.shapes.split(","):
        iw, ih, ow, oh, dtype, radius = SHAPES[name]
        n = 2 * args.pairs
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        src = torch.randint(0, 256, (n, ih, iw, 4), dtype=torch.uint8, device=dev, generator=g)
        if dtype != torch.uint8:
            src = (src.to(torch.float32) / 255.0).to(dtype)
        kw = dict(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, radius=radius)
        plain, hidden = A.PostProcessor(**kw), A.PostProcessor(**kw)
        for eye in (0, 1):
            hidden.set_hidden_area(eye, mesh)
        out_a = torch.zeros((n, oh, ow, 4), dtype=dtype, device=dev)
        out_b = torch.zeros((n, oh, ow, 4), dtype=dtype, device=dev)
        run_a = lambda: plain.apply_batch(src, out_a)    # noqa: E731
        run_b = lambda: hidden.apply_batch(src, out_b)   # noqa: E731
        if args.only:
            for _ in range(10):
                (run_a if args.only == "none" else run_b)()
            torch.cuda.synchronize()
            rec["shapes"][name] = {"only": args.only, "calls": 10}
            plain.close()
            hidden.close()
            continue
        # correctness first: equal outside the skipped tiles, untouched (zero) inside them
        run_a()
        run_b()
        torch.cuda.synchronize()
        total, skipped = hidden.hidden_area_stats(0)
        tiles = torch.from_numpy(K.hidden_tiles(mesh, ow, oh).astype(bool)).to(dev)
        skip = tiles.repeat_interleave(32, 0).repeat_interleave(32, 1)[:oh, :ow]
        if int(tiles.sum()) != skipped:
            raise SystemExit("%s: %d tiles skipped, the rule hides %d" % (name, skipped, int(tiles.sum())))
        if not torch.equal(out_b[:, ~skip], out_a[:, ~skip]) or bool((out_b[:, skip] != 0).any()):
            raise SystemExit("%s: the result under the mesh differs outside the skipped tiles, or a skipped tile was written" % name)
        variants = {"A": run_a, "A2": run_a, "B": run_b}
        est = {k: timed(f, 0.2, 1e-3) for k, f in variants.items()}   # warm-up + estimate
        res = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, f in variants.items():
                res[k].append(timed(f, args.window, est[k]))
        med = {k: statistics.median(v) for k, v in res.items()}
        rec["shapes"][name] = {
            "shape": "%dx%d -> %dx%d %s radius %.1f" % (iw, ih, ow, oh, str(dtype).replace("torch.", ""), radius),
            "tiles": total, "tiles_skipped": skipped, "hidden_share": round(skipped / total, 4),
            "step_ms": {k: round(v * 1e3, 4) for k, v in med.items()},
            "mesh_over_none_time": round(med["B"] / med["A"], 4), "none_over_none_time": round(med["A2"] / med["A"], 4),
            "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in res.items()},
        }
        plain.close()
        hidden.close()
        del src, out_a, out_b
        torch.cuda.empty_cache()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
