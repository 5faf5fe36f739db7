#!/usr/bin/env python3
"""Multisampled (4x MSAA RGBA8) input against single-sample input at C2's shape, one process, one device.  Prints one JSON line.

    A   C2 single-sample apply_batch, PAIRS stereo pairs per call (radius 2.0, sharpness 0.9)
    B   the same images as 4x MSAA RGBA8: the product path, the resolve inside easu_fast_kernel's staging sweep
    B'  B through the resolve pass (resolve_kernel, then the single-sample pipeline): a ctx of the -DOVRFSR_MSAA_RESOLVE_PASS build
        (ab/msaa_pass.so, tools/build_variant.sh msaa_pass -DOVRFSR_MSAA_RESOLVE_PASS), loaded beside the product library
    C   what a host pays without the feature: a torch-side resolve of the samples, then A
    D   the reference's call pattern, one stereo pair per call at the shipped radius 0.5 (C2r shape): D1 single-sample, D2 4x MSAA --
        GPU ms per frame (two ovrfsr_apply calls)
Every variant is warmed up, then timed with HIP events over windows of at least --window seconds, the variants interleaved round by round;
the figure is the median window.  The resolve kernel's own time comes from a separate kernel-trace run (--quick: one short round).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import openvr_fsr_amd as A  # noqa: E402
from openvr_fsr_amd import _capi as K  # noqa: E402

IW, IH, OW, OH = 1683, 1869, 2244, 2492
S = 4


def make_inputs(pairs, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    ms = torch.randint(0, 256, (2 * pairs, IH, IW, S, 4), dtype=torch.uint8, device=dev, generator=g)
    ss = resolve_torch(ms)
    return ms, ss


def resolve_torch(ms):
    """the header's rule, as a host would write it in torch: (sum + S/2) >> log2 S"""
    return ((ms.sum(dim=3, dtype=torch.int32) + S // 2) >> 2).to(torch.uint8)


def pass_library(path):
    """the measurement build, loaded beside the product library (own handle: its ctxs run its own kernels)"""
    if not os.path.exists(path):
        raise SystemExit("%s is missing: tools/build_variant.sh msaa_pass -DOVRFSR_MSAA_RESOLVE_PASS" % path)
    product = K.library()
    saved = os.environ.get("OVRFSR_LIB")
    os.environ["OVRFSR_LIB"] = path
    K._LIB = None
    try:
        lib = K.library()
    finally:
        K._LIB = product
        if saved is None:
            del os.environ["OVRFSR_LIB"]
        else:
            os.environ["OVRFSR_LIB"] = saved
    return lib


def make_pp(lib, **kw):
    """a PostProcessor whose ctx lives in `lib`"""
    product = K.library()
    K._LIB = lib
    try:
        return A.PostProcessor(**kw)
    finally:
        K._LIB = product


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
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--quick", action="store_true", help="one short round (for the kernel-trace run)")
    ap.add_argument("--pass-lib", default=os.path.join(ROOT, "ab", "msaa_pass.so"), help="the -DOVRFSR_MSAA_RESOLVE_PASS build (B')")
    args = ap.parse_args()
    if args.quick:
        args.rounds, args.window = 1, 0.05
    dev = torch.device("cuda:0")
    ms, ss = make_inputs(args.pairs, dev)
    n = 2 * args.pairs
    kw = dict(fsr_enabled=1, out_width=OW, out_height=OH, sharpness=0.9)
    out = torch.empty((n, OH, OW, 4), dtype=torch.uint8, device=dev)
    ppA = A.PostProcessor(radius=2.0, **kw)
    ppB = A.PostProcessor(radius=2.0, **kw)
    ppBp = make_pp(pass_library(args.pass_lib), radius=2.0, **kw)
    ppC = A.PostProcessor(radius=2.0, **kw)
    ppD1 = A.PostProcessor(radius=0.5, **kw)
    ppD2 = A.PostProcessor(radius=0.5, **kw)
    outL, outR = out[0], out[1]

    def frame(pp, src):
        pp.apply(A.EYE_LEFT, src[0], out=outL)
        pp.apply(A.EYE_RIGHT, src[1], out=outR)

    variants = {
        "A": lambda: ppA.apply_batch(ss, out),
        "B": lambda: ppB.apply_batch(ms, out),
        "Bp": lambda: ppBp.apply_batch(ms, out),
        "C": lambda: ppC.apply_batch(resolve_torch(ms), out),
        "D1": lambda: frame(ppD1, ss),
        "D2": lambda: frame(ppD2, ms),
    }
    # correctness first: B and C equal A bit for bit (the feature's contract), D2 equals D1
    ref = None
    for name in ("A", "B", "Bp", "C"):
        variants[name]()
        torch.cuda.synchronize()
        if ref is None:
            ref = out.clone()
        elif not torch.equal(out, ref):
            raise SystemExit("variant %s differs from A" % name)
    variants["D1"]()
    d1 = out[:2].clone()
    variants["D2"]()
    torch.cuda.synchronize()
    if not torch.equal(out[:2], d1):
        raise SystemExit("variant D2 differs from D1")
    est = {k: timed(f, 0.2 if not args.quick else 0.01, 1e-3) for k, f in variants.items()}  # warm-up + estimate
    res = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, f in variants.items():
            res[k].append(timed(f, args.window, est[k]))
    med = {k: statistics.median(v) for k, v in res.items()}
    pairs_s = {k: args.pairs / med[k] for k in ("A", "B", "Bp", "C")}
    rec = {
        "shape": "%dx%d -> %dx%d, RGBA8, %dx MSAA for B/C/D2" % (IW, IH, OW, OH, S),
        "pairs_per_call": args.pairs, "rounds": args.rounds, "window_s": args.window,
        "pairs_per_s": {k: round(v, 1) for k, v in pairs_s.items()},
        "B_over_A_time": round(med["B"] / med["A"], 4),
        "Bp_over_A_time": round(med["Bp"] / med["A"], 4),
        "B_gain_over_Bp": round(med["Bp"] / med["B"] - 1.0, 4),
        "C_over_B_time": round(med["C"] / med["B"], 4),
        "D_ms_per_frame": {"D1_single": round(med["D1"] * 1e3, 4), "D2_msaa": round(med["D2"] * 1e3, 4)},
        "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in res.items()},
        "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
