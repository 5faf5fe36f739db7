#!/usr/bin/env python3
"""What a moving input size costs per frame, at the C2 output (2244 x 2492, RGBA8, masked) and the C5 output (3160 x 3160, RGBA16F, masked),
one stereo pair per frame.  Prints one JSON line per leg and round, then a summary line.

Legs (each in a child process of its own, since a process loads one library; the legs are alternated round by round in one call):
  p1   the size changes every frame: every change a reset and rebuild                 the parent commit's library (--parent LIB)
  p8   ... every 8th frame                                                            the parent commit's library
  k1   the size changes every frame, a maximum set: re-scales, taps by the kernel     this library
  k8   ... every 8th frame                                                            this library
  u1   k1 with the taps uploaded through a staging slot (--upload LIB)                -DOVRFSR_RESCALE_UPLOAD_TAPS: decides kernel against upload
  u8   k8 likewise
  f    a fixed size (the first of the cycle), a maximum set                           this library
  pf   a fixed size, no maximum                                                       the parent commit's library; run twice per round (pf, pf2):
                                                                                      the spread of pf against pf2 is what every difference is read against
Per leg: --frames frames after --warmup, timed by device events around the whole run and by the host clock to a final synchronise, and the
host time spent inside the applies that changed the size (the re-scale's or rebuild's host cost); ms per frame each.  --only LEG runs that
leg in this process (the kernel-trace run: the program goes behind `rocprofv3 ... --`).
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

SHAPES = {   # output size, the cycle of input sizes (the first is the maximum), dtype name, radius
    "C2": (2244, 2492, [(1683, 1869), (1571, 1744), (1346, 1495)], "uint8", 0.5),
    "C5": (3160, 3160, [(2370, 2370), (2212, 2212), (1896, 1896)], "float16", 0.5),
}


def run_leg(leg, shape, frames, warmup):
    import numpy as np
    import torch
    import openvr_fsr_amd as A
    ow, oh, sizes, dt, radius = SHAPES[shape]
    dtype = getattr(torch, dt)
    rng = np.random.default_rng(5)
    texs = {}
    for iw, ih in sizes:
        pair = [torch.from_numpy(rng.integers(0, 256, (ih, iw, 4), dtype=np.uint8)).cuda() for _ in range(2)]
        texs[(iw, ih)] = pair if dtype == torch.uint8 else [(t.to(torch.float32) / 255.0).to(dtype) for t in pair]
    outs = [torch.empty((oh, ow, 4), dtype=dtype, device="cuda") for _ in range(2)]
    pp = A.PostProcessor(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, radius=radius)
    if leg[0] in "kuf":
        pp.set_max_input_size(*sizes[0])
    every = {"1": 1, "8": 8}.get(leg[-1], 0)
    change_host = [0.0, 0]

    def frame(i, timed):
        size = sizes[(i // every) % len(sizes)] if every else sizes[0]
        changes = bool(every) and i % every == 0
        t0 = time.perf_counter() if changes and timed else 0.0
        pp.apply(0, texs[size][0], out=outs[0])
        if changes and timed:
            change_host[0] += time.perf_counter() - t0
            change_host[1] += 1
        pp.apply(1, texs[size][1], out=outs[1])

    for i in range(warmup):
        frame(i, False)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for i in range(warmup, warmup + frames):
        frame(i, True)
    b.record()
    torch.cuda.synchronize()
    host = (time.perf_counter() - t0) * 1e3 / frames
    dev = a.elapsed_time(b) / frames
    stats = pp.rescale_stats() if hasattr(A.library(), "ovrfsr_rescale_stats") else None
    pp.close()
    return {"leg": leg, "shape": shape, "frames": frames, "device_ms_per_frame": round(dev, 5), "host_ms_per_frame": round(host, 5),
            "host_ms_per_changing_apply": round(change_host[0] * 1e3 / change_host[1], 5) if change_host[1] else None, "rescale_stats": stats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="C2,C5")
    ap.add_argument("--parent", default=None, help="the parent commit's library (legs p1, p8, pf)")
    ap.add_argument("--upload", default=None, help="a -DOVRFSR_RESCALE_UPLOAD_TAPS build (legs u1, u8)")
    ap.add_argument("--only", default=None, help="run this leg in this process, every shape, and print its lines")
    args = ap.parse_args()
    shapes = args.shapes.split(",")
    if args.only:
        for s in shapes:
            print(json.dumps(run_leg(args.only, s, args.frames, args.warmup)), flush=True)
        return 0
    legs = [("pf", args.parent), ("p1", args.parent), ("k1", None), ("u1", args.upload), ("p8", args.parent), ("k8", None), ("u8", args.upload), ("f", None),
            ("pf2", args.parent)]
    legs = [(leg, lib) for leg, lib in legs if lib or leg in ("k1", "k8", "f")]
    results = {}
    for _ in range(args.rounds):
        for leg, lib in legs:
            env = dict(os.environ, PYTHONPATH=ROOT)
            if lib:
                env["OVRFSR_LIB"] = os.path.abspath(lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", leg[:2] if leg == "pf2" else leg, "--frames", str(args.frames),
                                "--warmup", str(args.warmup), "--shapes", args.shapes], capture_output=True, text=True, timeout=600, env=env)
            if r.returncode != 0:
                print(json.dumps({"leg": leg, "error": r.stderr[-400:]}), flush=True)
                return 1
            for line in r.stdout.splitlines():
                rec = json.loads(line)
                rec["leg"] = leg
                print(json.dumps(rec), flush=True)
                results.setdefault((leg, rec["shape"]), []).append((rec["device_ms_per_frame"], rec["host_ms_per_frame"], rec["host_ms_per_changing_apply"]))
    summary = {"%s/%s" % k: {"device_ms": round(statistics.median(x[0] for x in v), 5), "host_ms": round(statistics.median(x[1] for x in v), 5),
                             "host_ms_per_changing_apply": v[0][2] if v[0][2] is None else round(statistics.median(x[2] for x in v), 5)}
               for k, v in results.items()}
    print(json.dumps({"summary": summary}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
