#!/usr/bin/env python3
"""cfg.reference_formats = 1 (the reference's rule: float submissions through a UNORM8 intermediate to an RGBA8 output) against the
default, one process, one device.  Prints one JSON line per shape.

Shapes: C5 (2370x2370 -> 3160x3160, radius 0.5) and C2's, unmasked (1683x1869 -> 2244x2492, radius 2.0); sharpness 0.9, PAIRS stereo pairs
per apply_batch call, structured content x2 (half of the intermediate saturates).
    off16   RGBA16F input, rule off: the half pipeline, RGBA16F out (C5: fused kernel + outside-tile kernel on two streams)
    on16    RGBA16F input, rule on: UNORM8 intermediate, RGBA8 out (C5: the mask-sorted form -- EASU on the tiles touching the radius,
            easu_outside_kernel<1, 0, 0> on the rest, rcas_dpp_kernel on the span records; C2: easu_fast_kernel<1, 0, ..> + rcas_dpp_kernel)
    offP / onP   the same values submitted as R11G11B10F (the unpack pass in front)
Every variant is warmed up, then timed with HIP events over windows of at least --window seconds, the variants interleaved round by round;
the figure is the median window.

    --guard [--lib-b other.so]   the near-tie guard's cost: EASU alone (stage_mask = 1), RGBA16F -> RGBA8, rule on, per eye image, on
        unit-range content and on the highlights x40 content (whose tiles list many pixels); with --lib-b the two libraries alternate
        round by round, each measurement in a fresh child process (a library older than the field ignores it: its unguarded kernel)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"C5": (2370, 2370, 3160, 3160, 0.5), "C2": (1683, 1869, 2244, 2492, 2.0)}


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


def content(n, iw, ih, dev, kind):
    """RGBA16F batch: the bench's structured generator at unit range ('unit'), scaled x2 ('x2'), or dark with 2 % highlights at x40 ('hl40')"""
    import torch
    import bench
    img = bench.synth_batch(n, iw, ih, torch.uint8, dev, 0x5EED0000).float() / 255.0
    if kind == "x2":
        img = img * 2.0
    elif kind == "hl40":
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        hot = torch.rand((n, ih, iw, 1), generator=g, device=dev) < 0.02
        img = torch.where(hot, 40.0 * (0.5 + 0.5 * torch.rand((n, ih, iw, 4), generator=g, device=dev)), img)
    img = img.half()
    img[..., 3] = 1.0
    return img


def pack_torch(h):
    """[..., 4] float16 (non-negative, finite) -> R11G11B10F words, mantissas truncated"""
    import torch
    b = h.view(torch.int16).to(torch.int32) & 0x7FFF
    return ((b[..., 0] >> 4) | ((b[..., 1] >> 4) << 11) | ((b[..., 2] >> 5) << 22)).contiguous()


def run_shape(name, args, dev):
    import torch
    import openvr_fsr_amd as A
    iw, ih, ow, oh, radius = SHAPES[name]
    n = 2 * args.pairs
    h = content(n, iw, ih, dev, "x2")
    p = pack_torch(h)
    kw = dict(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, radius=radius)
    out16 = torch.empty((n, oh, ow, 4), dtype=torch.float16, device=dev)
    out8 = torch.empty((n, oh, ow, 4), dtype=torch.uint8, device=dev)
    pps = {k: A.PostProcessor(reference_formats=int(k.startswith("on")), **kw) for k in ("off16", "on16", "offP", "onP")}
    fmt = A.FORMAT_R11G11B10F
    variants = {
        "off16": lambda: pps["off16"].apply_batch(h, out16),
        "on16": lambda: pps["on16"].apply_batch(h, out8),
        "offP": lambda: pps["offP"].apply_batch(p, out16, in_format=fmt),
        "onP": lambda: pps["onP"].apply_batch(p, out8, in_format=fmt),
    }
    est = {k: timed(f, 0.2 if not args.quick else 0.01, 1e-3) for k, f in variants.items()}  # warm-up + estimate
    res = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, f in variants.items():
            res[k].append(timed(f, args.window, est[k]))
    med = {k: statistics.median(v) for k, v in res.items()}
    rec = {
        "shape": "%s: %dx%d -> %dx%d, radius %g" % (name, iw, ih, ow, oh, radius),
        "pairs_per_call": args.pairs, "rounds": args.rounds, "window_s": args.window,
        "ms_per_call": {k: round(v * 1e3, 4) for k, v in med.items()},
        "us_per_eye": {k: round(v / n * 1e6, 3) for k, v in med.items()},
        "on16_over_off16_time": round(med["on16"] / med["off16"], 4),
        "onP_over_offP_time": round(med["onP"] / med["offP"], 4),
        "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in res.items()},
        "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(rec), flush=True)
    for pp in pps.values():
        pp.close()


def guard_child(args):
    """EASU alone, RGBA16F -> RGBA8, rule on: us per eye image on both contents, and the share of pixels the guard lists where the library
    can say (audit builds only: the product library keeps no counters)"""
    import torch
    import openvr_fsr_amd as A
    dev = torch.device("cuda:0")
    iw, ih, ow, oh, _ = SHAPES["C2"]
    n = 2 * args.pairs
    out = torch.empty((n, oh, ow, 4), dtype=torch.uint8, device=dev)
    rec = {"lib": os.path.basename(A.library_path())}
    for kind in ("unit", "hl40"):
        h = content(n, iw, ih, dev, kind)
        pp = A.PostProcessor(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, radius=2.0, stage_mask=1, reference_formats=1)
        f = lambda: pp.apply_batch(h, out)  # noqa: E731
        est = timed(f, 0.2, 1e-3)
        rec[kind + "_us_per_eye"] = round(statistics.median(timed(f, args.window, est) for _ in range(3)) / n * 1e6, 3)
        if hasattr(A.library(), "ovrfsr_debug_tie_audit"):
            import ctypes
            buf = (ctypes.c_ulonglong * 6)()
            A.library().ovrfsr_debug_tie_audit(buf, 1)
            f()
            torch.cuda.synchronize()
            A.library().ovrfsr_debug_tie_audit(buf, 0)
            rec[kind + "_listed_share"] = round(buf[1] / max(1, buf[0]), 5)
        pp.close()
    print(json.dumps(rec), flush=True)


def guard(args):
    libs = [None] + ([args.lib_b] if args.lib_b else [])
    rows = {lib: [] for lib in libs}
    for _ in range(args.rounds):
        for lib in libs:
            env = dict(os.environ)
            if lib:
                env["OVRFSR_LIB"] = os.path.abspath(lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--guard-child", "--pairs", str(args.pairs), "--window", str(args.window)],
                               capture_output=True, text=True, env=env, timeout=600)
            if r.returncode != 0:
                raise SystemExit("child failed: " + r.stderr[-800:])
            row = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps(row), flush=True)
            rows[lib].append(row)
    summary = {}
    for lib, rs in rows.items():
        summary[rs[0]["lib"] if lib else "this build"] = {k: statistics.median(r[k] for r in rs) for k in ("unit_us_per_eye", "hl40_us_per_eye")}
    print(json.dumps({"guard_cost_median_us_per_eye": summary, "rounds": args.rounds}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--shapes", default="C5,C2")
    ap.add_argument("--quick", action="store_true", help="one short round (for the kernel-trace run)")
    ap.add_argument("--guard", action="store_true")
    ap.add_argument("--guard-child", action="store_true")
    ap.add_argument("--lib-b", default=None)
    args = ap.parse_args()
    if args.quick:
        args.rounds, args.window = 1, 0.05
    if args.guard_child:
        return guard_child(args)
    if args.guard:
        return guard(args)
    import torch
    dev = torch.device("cuda:0")
    for name in args.shapes.split(","):
        run_shape(name, args, dev)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
