#!/usr/bin/env python3
"""What the mask feather costs per frame, at the C2r and C5 shapes (bench.py's), one stereo pair per frame.  Prints one JSON line per leg
and round, then the geometry of the pass per shape and width, then a summary line.

Legs (each in a child process of its own, since a process loads one library; the legs are alternated round by round in one call):
  p, p2  no feather, the parent commit's library (--parent LIB), twice per round: the spread of p against p2 is what w0 - p has to be
         read against (the A/A spread of the visit)
  w0     ovrfsr_set_mask_feather(0): off                                   this library
  w01    width 0.1                                                         this library
  w03    width 0.3                                                         this library
Per leg: --frames frames after --warmup, timed by device events around the whole run and by the host clock to a final synchronise; ms per
frame each.  The pass's own time is read as the device time of a feathered leg minus w0's (two launches per frame, one per eye); --only
LEG runs that leg in this process (a kernel-trace run: the program goes behind `rocprofv3 ... --`).
The geometry lines need no GPU: from ovrfsr_mask_constants and ovrfsr_mask_feather_weights, per eye image -- the tiles the pass launches
(the box of the disc), the tiles of them that hold a band pixel, and the band's share of the pixels.
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
WIDTHS = {"p": None, "w0": 0.0, "w01": 0.1, "w03": 0.3}
GUARD = 12


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
    pp = A.PostProcessor(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, radius=radius)
    if WIDTHS[leg] is not None:
        pp.set_mask_feather(WIDTHS[leg])

    def frame():
        for eye in (0, 1):
            pp.apply(eye, texs[eye], out=outs[eye])

    for _ in range(warmup):
        frame()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(frames):
        frame()
    b.record()
    torch.cuda.synchronize()
    host = (time.perf_counter() - t0) * 1e3 / frames
    dev = a.elapsed_time(b) / frames
    launches = pp.mask_feather_stats() if WIDTHS[leg] is not None else None
    pp.close()
    return {"leg": leg, "shape": shape, "frames": frames, "device_ms_per_frame": round(dev, 5), "host_ms_per_frame": round(host, 5), "feather_launches": launches}


def geometry(shape, width):
    """per eye image: tiles launched, tiles with a band pixel, the band's share of the pixels"""
    import numpy as np
    import openvr_fsr_amd as A
    from openvr_fsr_amd import _capi as K
    _, _, ow, oh, _, radius = SHAPES[shape]
    centre, rad = A.mask_constants(ow, oh, (0.5, 0.5, 0.5, 0.5), radius, 1, 0)
    R = int(rad[0])
    F = int(np.float32(np.float32(0.5) * np.float32(width)) * np.float32(oh))
    w8, inside = K.mask_feather_weights(centre, R, F, ow, oh)
    b = (inside != 0) & (w8 < 256)
    reach = R + GUARD
    x0, y0 = max(int(centre[0]) - reach, 0) // 32, max(int(centre[1]) - reach, 0) // 32
    x1, y1 = (min(int(centre[0]) + reach + 1, ow) + 31) // 32, (min(int(centre[1]) + reach + 1, oh) + 31) // 32
    ty, tx = (oh + 31) // 32, (ow + 31) // 32
    pad = np.zeros((ty * 32, tx * 32), bool)
    pad[:oh, :ow] = b
    with_band = int(pad.reshape(ty, 32, tx, 32).any(axis=(1, 3)).sum())
    return {"shape": shape, "width": width, "R": R, "F": F, "tiles_launched": (x1 - x0) * (y1 - y0), "tiles_with_a_band_pixel": with_band,
            "tiles_of_the_image": tx * ty, "band_share_of_pixels": round(float(b.mean()), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="C2r,C5")
    ap.add_argument("--parent", default=None, help="the parent commit's library (legs p, p2)")
    ap.add_argument("--only", default=None, help="run this leg in this process, every shape, and print its lines")
    args = ap.parse_args()
    shapes = args.shapes.split(",")
    if args.only:
        for s in shapes:
            print(json.dumps(run_leg(args.only, s, args.frames, args.warmup)), flush=True)
        return 0
    legs = [("p", args.parent), ("w0", None), ("w01", None), ("w03", None), ("p2", args.parent)]
    legs = [(leg, lib) for leg, lib in legs if lib or leg.startswith("w")]
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
    for s in shapes:
        for w in (0.1, 0.3):
            print(json.dumps({"geometry": geometry(s, w)}), flush=True)
    summary = {"%s/%s" % k: {"device_ms": round(statistics.median(x[0] for x in v), 5), "host_ms": round(statistics.median(x[1] for x in v), 5)}
               for k, v in results.items()}
    print(json.dumps({"summary": summary}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
