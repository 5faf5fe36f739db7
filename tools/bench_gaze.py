#!/usr/bin/env python3
"""What a moving gaze costs per frame, at the C2r and C5 shapes (bench.py's), one stereo pair per frame.  Prints one JSON line per leg and
round, then a summary line.

Legs (each in a child process of its own, since a process loads one library; the legs are alternated round by round in one call):
  a   the gaze set once and never moved                                     this library
  b   the gaze moved every frame by more than a tile                        this library
  bh  b on a build that uploads host-built records (--host-records LIB)     -DOVRFSR_GAZE_HOST_RECORDS: decides kernel against upload
  c   ovrfsr_set_config with the new centre, then apply: the only way       the parent commit's library (--parent LIB)
      to move the mask without ovrfsr_set_gaze
  d   a with no gaze                                                        the parent commit's library; run twice per round (d, d2): the
                                                                            spread of d against d2 is what a - d has to be read against
Per leg: --frames frames after --warmup, timed by device events around the whole run and by the host clock to a final synchronise;
ms per frame each.  --only LEG runs that leg in this process (the kernel-trace run: the program goes behind `rocprofv3 ... --`).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {   # bench.py's WORKLOADS: input and output size, dtype name, radius
    "C2r": (1683, 1869, 2244, 2492, "uint8", 0.5),
    "C5": (2370, 2370, 3160, 3160, "float16", 0.5),
}
# more than a tile apart from frame to frame, all with a mixed mask
GAZES = [(0.5, 0.5), (0.3, 0.35), (0.65, 0.6), (0.4, 0.7), (0.7, 0.3), (0.25, 0.55), (0.55, 0.25), (0.6, 0.75)]


def run_leg(leg, shape, frames, warmup):
    import numpy as np
    import torch
    import openvr_fsr_amd as A
    iw, ih, ow, oh, dt, radius = SHAPES[shape]
    dtype = getattr(torch, dt)
    rng = np.random.default_rng(5)
    texs = [torch.from_numpy(rng.integers(0, 256, (ih, iw, 4), dtype=np.uint8)).cuda() for _ in range(2)]
    if dtype != torch.uint8:
        texs = [(t.to(torch.float32) / 255.0).to(dtype) for t in texs]
    outs = [torch.empty((oh, ow, 4), dtype=dtype, device="cuda") for _ in range(2)]
    cfg = dict(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, radius=radius)
    pp = A.PostProcessor(**cfg)
    moving = leg in ("b", "bh", "c")
    if leg in ("a", "b", "bh"):
        for eye in (0, 1):
            pp.set_gaze(eye, *GAZES[0])

    def frame(i):
        if moving:
            g = GAZES[i % len(GAZES)]
            if leg == "c":
                pp.set_config(A.Config.default(proj_centre=g + (1.0 - g[0], g[1]), **cfg))
            else:
                pp.set_gaze(0, *g)
                pp.set_gaze(1, 1.0 - g[0], g[1])
        for eye in (0, 1):
            pp.apply(eye, texs[eye], out=outs[eye])

    for i in range(warmup):
        frame(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for i in range(frames):
        frame(i)
    b.record()
    torch.cuda.synchronize()
    host = (time.perf_counter() - t0) * 1e3 / frames
    dev = a.elapsed_time(b) / frames
    stats = pp.gaze_stats() if hasattr(A.library(), "ovrfsr_gaze_stats") else None
    pp.close()
    return {"leg": leg, "shape": shape, "frames": frames, "device_ms_per_frame": round(dev, 5), "host_ms_per_frame": round(host, 5), "gaze_stats": stats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="C2r,C5")
    ap.add_argument("--parent", default=None, help="the parent commit's library (legs c, d)")
    ap.add_argument("--host-records", default=None, help="a -DOVRFSR_GAZE_HOST_RECORDS build (leg bh)")
    ap.add_argument("--only", default=None, help="run this leg in this process, every shape, and print its lines")
    args = ap.parse_args()
    shapes = args.shapes.split(",")
    if args.only:
        for s in shapes:
            print(json.dumps(run_leg(args.only, s, args.frames, args.warmup)), flush=True)
        return 0
    legs = [("d", args.parent), ("a", None), ("b", None), ("bh", args.host_records), ("c", args.parent), ("d2", args.parent)]
    legs = [(leg, lib) for leg, lib in legs if lib or leg in ("a", "b")]
    results = {}
    for _ in range(args.rounds):
        for leg, lib in legs:
            env = dict(os.environ, PYTHONPATH=ROOT)
            if lib:
                env["OVRFSR_LIB"] = os.path.abspath(lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", leg.rstrip("2"), "--frames", str(args.frames), "--warmup", str(args.warmup),
                                "--shapes", args.shapes], capture_output=True, text=True, timeout=600, env=env)
            if r.returncode != 0:
                print(json.dumps({"leg": leg, "error": r.stderr[-400:]}), flush=True)
                return 1
            for line in r.stdout.splitlines():
                rec = json.loads(line)
                rec["leg"] = leg
                print(json.dumps(rec), flush=True)
                results.setdefault((leg, rec["shape"]), []).append((rec["device_ms_per_frame"], rec["host_ms_per_frame"]))
    summary = {"%s/%s" % k: {"device_ms": round(statistics.median(x[0] for x in v), 5), "host_ms": round(statistics.median(x[1] for x in v), 5)}
               for k, v in results.items()}
    print(json.dumps({"summary": summary}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
