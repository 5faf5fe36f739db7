#!/usr/bin/env python3
"""tools/debug/host_enqueue.py -- host-side cost of one ovrfsr_apply_batch call from Python (ctypes + the torch plumbing of
openvr_fsr_amd.PostProcessor.apply_batch) with 1, 2, 4, 8 host threads, each with its own ctx and stream.

bench.py's direct multi-GPU launcher (`python bench.py --gpus N`, one process) drives every device from its own Python
thread; the ctypes call releases the GIL but the Python around it (image_of, struct packing, status check) does not.  This
measures that ceiling: calls per second the host can issue, on images so small (one 32x32 tile) that the GPU side of a call
is a few microseconds.  All threads target device 0 (a gpurun box has one GPU): the host path is the same as with one
device per thread, and the device never becomes the bottleneck before the host does at these sizes.
The torchrun launcher (what the round driver uses for N > 1) has one process, hence one GIL, per GPU: there the
single-thread row applies.

    python tools/debug/host_enqueue.py --c2
One thread, C2's shape (1683x1869 -> 2244x2492), ONE EYE PER CALL through PostProcessor.apply -- the reference's call pattern -- unmasked
(radius 2.0: two-pass) and masked (radius 0.5: mask-sorted): host time per call (400 calls, the queue drained every 8), and the wall time
of the first apply of a fresh ctx, synchronised (plan + upload + launch: the rebuild; median of 8 fresh ctxs, the process's first one
discarded because it loads the code objects); and the masked configuration once more with cfg.pair_submit = 1, L,R per frame (host time
per call: the submission sequencer's path, csrc/submit_sequence.cpp).  Prints one line "C2 {json}".  OVRFSR_LIB selects the library, so two builds can be run
alternately, one process per run (profiles/pipeline_plan.txt)."""
import os
import sys
import threading
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import openvr_fsr_amd as A  # noqa: E402

CALLS = 3000


def worker(i, gate, out):
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        pp = A.PostProcessor(device=0, fsr_enabled=1, out_width=32, out_height=32, sharpness=0.9, radius=2.0)
        texs = torch.randint(0, 255, (2, 24, 24, 4), dtype=torch.uint8, device="cuda")
        outs = torch.empty((2, 32, 32, 4), dtype=torch.uint8, device="cuda")
        for _ in range(50):
            pp.apply_batch(texs, outs, first_eye=A.EYE_LEFT, alternate_eyes=True)
        stream.synchronize()
        gate.wait()
        t0 = time.perf_counter()
        for k in range(CALLS):
            pp.apply_batch(texs, outs, first_eye=A.EYE_LEFT, alternate_eyes=True)
            if (k & 255) == 255:
                stream.synchronize()   # keep the launch queue shallow: a full queue would make enqueue wait for the device
        t1 = time.perf_counter()
        stream.synchronize()
        out[i] = (t1 - t0) / CALLS
        pp.close()


def c2_single_eye():
    import json
    iw, ih, ow, oh = 1683, 1869, 2244, 2492
    tex = [torch.randint(0, 255, (ih, iw, 4), dtype=torch.uint8, device="cuda") for _ in range(2)]
    out = [torch.empty((oh, ow, 4), dtype=torch.uint8, device="cuda") for _ in range(2)]
    res = {}
    for name, radius in (("unmasked", 2.0), ("masked", 0.5)):
        cfg = dict(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, radius=radius)
        firsts = []
        for _ in range(9):
            pp = A.PostProcessor(**cfg)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pp.apply(0, tex[0], out=out[0])
            torch.cuda.synchronize()
            firsts.append((time.perf_counter() - t0) * 1e3)
            pp.close()
        res["first_apply_ms_" + name] = sorted(firsts[1:])[len(firsts[1:]) // 2]
        pp = A.PostProcessor(**cfg)
        for k in range(20):
            pp.apply(k & 1, tex[k & 1], out=out[k & 1])
        torch.cuda.synchronize()
        calls, host = 400, 0.0
        for k in range(calls):
            t0 = time.perf_counter()
            pp.apply(k & 1, tex[k & 1], out=out[k & 1])
            host += time.perf_counter() - t0
            if (k & 7) == 7:
                torch.cuda.synchronize()   # keep the launch queue shallow
        torch.cuda.synchronize()
        res["host_us_per_call_" + name] = host / calls * 1e6
        pp.close()
    # cfg.pair_submit = 1, masked: L,R per frame -- the first eye of a frame is only recorded, the second launches both as a batch of two
    pp = A.PostProcessor(fsr_enabled=1, out_width=ow, out_height=oh, sharpness=0.9, radius=0.5, pair_submit=1)
    for k in range(20):
        pp.apply(k & 1, tex[k & 1], out=out[k & 1])
    torch.cuda.synchronize()
    calls, host = 400, 0.0
    for k in range(calls):
        t0 = time.perf_counter()
        pp.apply(k & 1, tex[k & 1], out=out[k & 1])
        host += time.perf_counter() - t0
        if (k & 7) == 7:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    res["host_us_per_call_pair_submit"] = host / calls * 1e6
    pp.close()
    print("C2 " + json.dumps(res), flush=True)


if "--c2" in sys.argv[1:]:
    c2_single_eye()
    sys.exit(0)

print("threads  us_per_call(mean over threads)  calls_per_s(all threads)   [EASU + RCAS apply_batch of 2 images 24x24 -> 32x32, %d calls per thread]" % CALLS)
for n in (1, 2, 4, 8):
    gate = threading.Barrier(n)
    res = [0.0] * n
    ts = [threading.Thread(target=worker, args=(i, gate, res)) for i in range(n)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    mean = sum(res) / n
    print("%7d  %28.1f  %24.0f" % (n, mean * 1e6, n / mean))
