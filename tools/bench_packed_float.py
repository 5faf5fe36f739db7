#!/usr/bin/env python3
"""R11G11B10F input against the same values submitted as RGBA16F, one process, one device.  Prints one JSON line per shape.

Shapes: C5 (2370x2370 -> 3160x3160, radius 0.5) and C2's, unmasked (1683x1869 -> 2244x2492, radius 2.0); RGBA16F output, sharpness 0.9,
PAIRS stereo pairs per apply_batch call.
    A1  the decoded images as RGBA16F (what the library took before the format existed: the baseline)
    P1  the same values as R11G11B10F: the unpack pass (packed_resolve_kernel<1>), then A1's pipeline
    H1  what a host pays without the format: a torch-side unpack to an RGBA16F tensor, then A1
    A4 / P4 / H4  the same with 4 samples per texel: A4 takes the resolved RGBA16F images, P4 the packed samples, H4 unpacks and resolves
        (fp32, sample order) in torch
    copy  a device-to-device copy that moves the bytes the unpack pass moves (4 read + 8 written per texel, as 6 + 6)
Every variant is warmed up, then timed with HIP events over windows of at least --window seconds, the variants interleaved round by round;
the figure is the median window.  P - A is the cost of the pass inside a step; the kernels' own times come from a separate
kernel-trace run (--quick: one short round).

--ab LIB: the shipped library (single-sample words decoded inside kernel staging) against a pass build of the same sources
(tools/build_variant.sh packed_pass -DOVRFSR_PACKED_RESOLVE_PASS -> ab/packed_pass.so: the unpack pass everywhere), as tools/abn.sh compares
builds: one child process per (round, build) on one box, the builds alternated round by round through OVRFSR_LIB, each child timing P1 and
A1 (--child).  Every round runs the shipped build twice, first and last: the two series are the run's own A/A spread.  Prints one JSON
line per shape: medians, P1 of each build over A1, in place over pass, and the A/A spread next to it.
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

SHAPES = {"C5": (2370, 2370, 3160, 3160, 0.5), "C2": (1683, 1869, 2244, 2492, 2.0)}
S = 4
# --ab only: the other forms that decode in staging, as a recorded shape plus configuration and destination
#   C5 fused kernel + outside tiles (masked default)   C2 two-pass (unmasked)   C5r mask-sorted (reference_formats: UNORM8 intermediate and output)
#   C5e EASU only, masked   C2f the fused kernel on request, unmasked
FORMS = {"C5": ("C5", {}, torch.float16), "C2": ("C2", {}, torch.float16), "C5r": ("C5", {"reference_formats": 1}, torch.uint8),
         "C5e": ("C5", {"stage_mask": 1}, torch.float16), "C2f": ("C2", {"fused": 1}, torch.float16)}


def unpack_torch(p):
    """the header's decode as a host would write it in torch: [...] int32 words -> [..., 4] float16"""
    r = (p & 0x7FF) << 4
    g = ((p >> 11) & 0x7FF) << 4
    b = ((p >> 22) & 0x3FF) << 5
    a = torch.full_like(p, 0x3C00)
    return torch.stack((r, g, b, a), dim=-1).to(torch.int16).view(torch.float16)


def resolve_torch(ms):
    """[..., S] packed samples -> [..., 4] float16: decode, fp32 sum in sample order, times 1/S, half"""
    f = unpack_torch(ms).float()
    acc = f[..., 0, :]
    for i in range(1, ms.shape[-1]):
        acc = acc + f[..., i, :]
    return (acc * (1.0 / ms.shape[-1])).half()


def make_inputs(n, iw, ih, dev):
    """finite codes only (exponents below 31), values up to 4: HDR scene colour"""
    g = torch.Generator(device=dev)
    g.manual_seed(1)

    def codes(shape, ebits_max, mbits):
        e = torch.randint(0, ebits_max, shape, dtype=torch.int32, device=dev, generator=g)
        m = torch.randint(0, 1 << mbits, shape, dtype=torch.int32, device=dev, generator=g)
        return (e << mbits) | m

    shape = (n, ih, iw, S)
    ms = codes(shape, 18, 6) | (codes(shape, 18, 6) << 11) | (codes(shape, 18, 5) << 22)
    return ms


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


def run_shape(name, args, dev):
    iw, ih, ow, oh, radius = SHAPES[name]
    n = 2 * args.pairs
    ms = make_inputs(n, iw, ih, dev)
    p1 = ms[..., 0].contiguous()
    h1 = unpack_torch(p1)
    h4 = resolve_torch(ms)
    kw = dict(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, radius=radius)
    out = torch.empty((n, oh, ow, 4), dtype=torch.float16, device=dev)
    pps = {k: A.PostProcessor(**kw) for k in ("A1", "P1", "H1", "A4", "P4", "H4")}
    texels = n * ih * iw
    cp_src = torch.empty(texels * 6, dtype=torch.uint8, device=dev)
    cp_dst = torch.empty_like(cp_src)
    fmt = A.FORMAT_R11G11B10F
    variants = {
        "A1": lambda: pps["A1"].apply_batch(h1, out),
        "P1": lambda: pps["P1"].apply_batch(p1, out, in_format=fmt),
        "H1": lambda: pps["H1"].apply_batch(unpack_torch(p1), out),
        "A4": lambda: pps["A4"].apply_batch(h4, out),
        "P4": lambda: pps["P4"].apply_batch(ms, out, in_format=fmt),
        "H4": lambda: pps["H4"].apply_batch(resolve_torch(ms), out),
        "copy": lambda: cp_dst.copy_(cp_src),
    }
    # correctness first: P and H equal A byte for byte (the format's contract)
    for base, others in (("A1", ("P1", "H1")), ("A4", ("P4", "H4"))):
        variants[base]()
        torch.cuda.synchronize()
        ref = out.clone()
        for k in others:
            out.zero_()
            variants[k]()
            torch.cuda.synchronize()
            if not torch.equal(out.view(torch.int16), ref.view(torch.int16)):
                raise SystemExit("%s: variant %s differs from %s" % (name, k, base))
        del ref
    est = {k: timed(f, 0.2 if not args.quick else 0.01, 1e-3) for k, f in variants.items()}  # warm-up + estimate
    res = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, f in variants.items():
            res[k].append(timed(f, args.window, est[k]))
    med = {k: statistics.median(v) for k, v in res.items()}
    pass1, pass4 = med["P1"] - med["A1"], med["P4"] - med["A4"]
    copy_rate = texels * 12 / med["copy"]
    rec = {
        "shape": "%s: %dx%d -> %dx%d, radius %g, RGBA16F out" % (name, iw, ih, ow, oh, radius),
        "pairs_per_call": args.pairs, "rounds": args.rounds, "window_s": args.window,
        "ms_per_call": {k: round(v * 1e3, 4) for k, v in med.items()},
        "P1_over_A1_time": round(med["P1"] / med["A1"], 4),
        "P4_over_A4_time": round(med["P4"] / med["A4"], 4),
        "P1_over_H1_time": round(med["P1"] / med["H1"], 4),
        "P4_over_H4_time": round(med["P4"] / med["H4"], 4),
        "pass_us_per_eye_in_step": {"S1": round(pass1 / n * 1e6, 3), "S4": round(pass4 / n * 1e6, 3)},
        "copy_TBps": round(copy_rate * 1e-12, 3),
        # (P - A) / bytes: the pass as the step sees it, overlap with the pipeline's own launches included
        "pass_rate_over_copy_in_step": {"S1": round(texels * 12 / pass1 / copy_rate, 3) if pass1 > 0 else None,
                                        "S4": round(texels * (4 * S + 8) / pass4 / copy_rate, 3) if pass4 > 0 else None},
        "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in res.items()},
        "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(rec), flush=True)
    for pp in pps.values():
        pp.close()


def run_child(name, args, dev):
    """P1 and A1 of one shape with whatever library OVRFSR_LIB names: one JSON line"""
    shape, extra, out_dt = FORMS[name]
    iw, ih, ow, oh, radius = SHAPES[shape]
    n = 2 * args.pairs
    g = torch.Generator(device=dev)
    g.manual_seed(1)

    def codes(ebits_max, mbits):   # make_inputs' codes, one sample per texel
        e = torch.randint(0, ebits_max, (n, ih, iw), dtype=torch.int32, device=dev, generator=g)
        m = torch.randint(0, 1 << mbits, (n, ih, iw), dtype=torch.int32, device=dev, generator=g)
        return (e << mbits) | m

    p1 = codes(18, 6) | (codes(18, 6) << 11) | (codes(18, 5) << 22)
    h1 = unpack_torch(p1)
    kw = dict(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, radius=radius, **extra)
    out = torch.empty((n, oh, ow, 4), dtype=out_dt, device=dev)
    pps = {k: A.PostProcessor(**kw) for k in ("A1", "P1")}
    variants = {"A1": lambda: pps["A1"].apply_batch(h1, out), "P1": lambda: pps["P1"].apply_batch(p1, out, in_format=A.FORMAT_R11G11B10F)}
    variants["A1"]()
    torch.cuda.synchronize()
    ref = out.clone()
    out.zero_()
    variants["P1"]()
    torch.cuda.synchronize()
    if not torch.equal(out.view(torch.uint8), ref.view(torch.uint8)):
        raise SystemExit("%s: P1 differs from A1" % name)
    del ref
    est = {k: timed(f, 0.2, 1e-3) for k, f in variants.items()}
    res = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, f in variants.items():
            res[k].append(timed(f, args.window, est[k]))
    print(json.dumps({"shape": name, "ms": {k: statistics.median(v) * 1e3 for k, v in res.items()}}), flush=True)
    for pp in pps.values():
        pp.close()


def run_ab(args):
    """the parent of --ab: starts the children, never touches the device itself"""
    import subprocess
    shipped = os.path.join(ROOT, "openvr_fsr_amd", "libopenvr_fsr_amd.so")
    builds = (("in_place", shipped), ("pass", os.path.abspath(args.ab)), ("in_place_again", shipped))
    for name in args.shapes.split(","):
        ms = {b: {"A1": [], "P1": []} for b, _ in builds}
        for _ in range(args.rounds):
            for b, lib in builds:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--shapes", name, "--pairs", str(args.pairs),
                                    "--rounds", str(args.child_rounds), "--window", str(args.window)],
                                   env=dict(os.environ, OVRFSR_LIB=lib), capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise SystemExit("child (%s, %s) failed: %s" % (name, b, r.stderr[-800:]))   # nothing more is started
                got = json.loads(r.stdout.strip().splitlines()[-1])["ms"]
                for k in ("A1", "P1"):
                    ms[b][k].append(got[k])
                print("%s %s: A1 %.4f P1 %.4f ms" % (name, b, got["A1"], got["P1"]), file=sys.stderr, flush=True)
        med = {b: {k: statistics.median(v) for k, v in d.items()} for b, d in ms.items()}
        iw, ih, ow, oh, radius = SHAPES[FORMS[name][0]]
        a1 = statistics.median([med[b]["A1"] for b, _ in builds])
        rec = {
            "shape": "%s: %dx%d -> %dx%d, radius %g, %s, %s out" % (name, iw, ih, ow, oh, radius, FORMS[name][1] or "default cfg",
                                                                   str(FORMS[name][2]).replace("torch.", "")),
            "pairs_per_call": args.pairs, "rounds": args.rounds, "child_rounds": args.child_rounds, "window_s": args.window,
            "ms_per_call": {b: {k: round(v, 4) for k, v in d.items()} for b, d in med.items()},
            "P1_over_A1": {b: round(med[b]["P1"] / a1, 4) for b, _ in builds},
            "in_place_over_pass": round(med["in_place"]["P1"] / med["pass"]["P1"], 4),
            "aa_spread": round(abs(med["in_place"]["P1"] - med["in_place_again"]["P1"]) / med["in_place"]["P1"], 4),
            "round_spread": {b: round((max(d["P1"]) - min(d["P1"])) / med[b]["P1"], 4) for b, d in ms.items()},
            "gain_us_per_eye": round((med["pass"]["P1"] - med["in_place"]["P1"]) / (2 * args.pairs) * 1e3, 3),
        }
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--shapes", default="C5,C2")
    ap.add_argument("--quick", action="store_true", help="one short round (for the kernel-trace run)")
    ap.add_argument("--ab", metavar="LIB", help="the shipped library against this pass build (ab/packed_pass.so), alternated round by round")
    ap.add_argument("--child-rounds", type=int, default=3, help="--ab: windows per variant inside one child")
    ap.add_argument("--child", action="store_true", help="(what --ab starts) P1 and A1 only, with the library OVRFSR_LIB names")
    args = ap.parse_args()
    if args.ab:
        return run_ab(args)
    if args.quick:
        args.rounds, args.window = 1, 0.05
    dev = torch.device("cuda:0")
    for name in args.shapes.split(","):
        (run_child if args.child else run_shape)(name, args, dev)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
