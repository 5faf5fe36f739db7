#!/usr/bin/env python3
"""tools/debug/record_forms.py -- what the launch manager DOES for a matrix of configurations, as a record two builds can be compared by.

Every case is a fresh ctx driven through the C ABI.  Recorded per case: the status and error text of every call (a refused call is made a
second time: the record then shows whether the refusal disabled the ctx), the format of a ctx-owned output, and the SHA-256 of the output
bytes.  tests/golden/launch_forms_parent.json is this record taken at the commit BEFORE the pipeline planner (csrc/pipeline_plan.cpp);
tests/test_gpu_launch_forms.py runs the same matrix on the tree under test and asserts equality, tests/test_pipeline_plan.py checks the
planner's predictions (status, text, owned format) against it without a GPU.

    python tools/debug/record_forms.py OUT.json        (GPU)

run_case(case, content=..., arrays=True) also hands back the output arrays it hashed, and runs the case on uniform-random content where asked:
tests/test_gpu_launch_forms_oracle.py compares those arrays with the CPU oracle (tests/forms_model.py, which reads the eye images from
source_array(), the numpy half of the upload).  The record itself is always taken on the structured content and holds no arrays.

The matrix (cases()):
  * RGBA8 source, ctx-owned output: the full factorial of precision {0, 2, 3} x use_nis x stage_mask {0, 1, 2} x fused {-1, 0, 1} x
    quantize_intermediate x reference_formats x mask {off, on};
  * RGBA16F source: that factorial cut to what changes the form of a half pipeline (the full factorial of two sources does not fit the
    size the record may have);
  * the other sources (BGRA8, RGBA32F, RGB10A2, R11G11B10F, 4x RGBA8, 2x RGBA16F): a set that reaches every form the source can take;
  * destinations: ctx-owned throughout, and per source a caller-owned image of the owned format, a float one for RGBA8 and RGB10A2, an RGBA8
    one for RGB10A2, a BGRA8 one;
  * shapes: 80x64 -> 160x128; 96x80 -> 96x80 where stage_mask = 2 (sharpen-only needs equal sizes); 128x96 -> 96x72 for the LDS-fit refusals
    and the runtime-pitch kernels; and one case per refusal the factorial does not reach;
  * one batch of four with alternating eyes per form, one shared side-by-side batch, a pair_submit L,R pair, and one with a BGRA8 destination.
"""
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# ovrfsr_format values (include/openvr_fsr_amd.h)
RGBA8, RGBA16F, RGBA32F, RGB10A2, BGRA8, R11G11B10F = 0, 1, 2, 3, 4, 6
MS4_RGBA8, MS2_RGBA16F = RGBA8 | 4 << 8, RGBA16F | 2 << 8
SOURCES = {"rgba8": RGBA8, "bgra8": BGRA8, "rgba16f": RGBA16F, "rgba32f": RGBA32F, "rgb10a2": RGB10A2, "r11g11b10f": R11G11B10F,
           "ms4_rgba8": MS4_RGBA8, "ms2_rgba16f": MS2_RGBA16F}
FORMAT_NAMES = {RGBA8: "rgba8", RGBA16F: "rgba16f", RGBA32F: "rgba32f", RGB10A2: "rgb10a2", BGRA8: "bgra8"}

BASE, EQUAL, MINIFY = (80, 64, 160, 128), (96, 80, 96, 80), (128, 96, 96, 72)
# masked: one radius and projection centre, the eyes' centres unequal -- at 160x128 each eye has tiles inside the radius, ring tiles
# and outside tiles that are not ring (asserted on the planner's tile lists by tests/test_pipeline_plan.py)
MASK_ON = dict(radius=0.5, proj_centre=(0.2, 0.3, 0.8, 0.7))
MASK_OFF = dict(radius=2.0)


def _case(cid, src, shape, cfg, mask, dst="owned", kind="apply"):
    c = dict(fsr_enabled=1, sharpness=0.9)
    c.update(cfg)
    c.update(MASK_ON if mask else MASK_OFF)
    iw, ih, ow, oh = shape
    if "render_scale" not in c:
        c.update(out_width=ow, out_height=oh)
    return dict(id=cid, src=src, shape=list(shape), cfg=c, mask=bool(mask), dst=dst, kind=kind)


def _cfg_id(p, nis, sm, fu, q, rf, m):
    return "p%d-nis%d-sm%d-f%d-q%d-rf%d-m%d" % (p, nis, sm, fu, q, rf, m)


def cases():
    out = []

    def add(src, p, nis, sm, fu, q, rf, m, dst="owned", kind="apply", shape=None, tag=""):
        shape = shape or (EQUAL if sm == 2 else BASE)
        cfg = dict(precision=p, use_nis=nis, stage_mask=sm, fused=fu, quantize_intermediate=q, reference_formats=rf)
        cid = "%s/%s%s%s%s" % (src, _cfg_id(p, nis, sm, fu, q, rf, m), "" if dst == "owned" else "/to-" + dst, "" if kind == "apply" else "/" + kind, tag)
        out.append(_case(cid, src, shape, cfg, m, dst, kind))

    for p, nis, sm, fu, q, rf, m in itertools.product((0, 2, 3), (0, 1), (0, 1, 2), (-1, 0, 1), (0, 1), (0, 1), (0, 1)):
        add("rgba8", p, nis, sm, fu, q, rf, m)
    # RGBA16F: the factorial cut to what changes the form of a half pipeline
    for p, nis, rf, m in itertools.product((0, 2, 3), (0, 1), (0, 1), (0, 1)):
        add("rgba16f", p, nis, 0, -1, 1, rf, m)
    for fu, rf, m in itertools.product((0, 1), (0, 1), (0, 1)):
        add("rgba16f", 0, 0, 0, fu, 1, rf, m)
    for sm, m in itertools.product((1, 2), (0, 1)):
        add("rgba16f", 0, 0, sm, -1, 1, 0, m)
    add("rgba16f", 0, 0, 0, -1, 0, 0, 0)
    add("rgba16f", 0, 0, 0, -1, 0, 0, 1)
    add("rgba16f", 3, 0, 0, 1, 1, 0, 0)
    add("rgba16f", 0, 1, 2, -1, 1, 0, 0)
    # the other sources: two-pass, mask-sorted / fused with masked outside tiles, fused on request, EASU-only, sharpen-only, NIS, strict,
    # and the reference format rule
    reduced = [(0, 0, 0, -1, 1, 0, 0), (0, 0, 0, -1, 1, 0, 1), (0, 0, 0, 1, 1, 0, 1), (0, 0, 1, -1, 1, 0, 1), (0, 0, 2, -1, 1, 0, 0),
               (0, 1, 0, -1, 1, 0, 1), (2, 0, 0, -1, 1, 0, 1), (0, 0, 0, -1, 1, 1, 1)]
    for src in ("bgra8", "rgba32f", "rgb10a2", "r11g11b10f", "ms4_rgba8", "ms2_rgba16f"):
        for t in reduced:
            add(src, *t)
    # destinations
    owned = {"rgba8": "rgba8", "bgra8": "rgba8", "rgba16f": "rgba16f", "rgba32f": "rgba32f", "rgb10a2": "rgb10a2", "r11g11b10f": "rgba16f",
             "ms4_rgba8": "rgba8", "ms2_rgba16f": "rgba16f"}
    for src in SOURCES:
        for m in ((0, 1) if src in ("rgba8", "rgba16f") else (1,)):
            add(src, 0, 0, 0, -1, 1, 0, m, dst=owned[src])
    for src, dst in (("rgba8", "rgba32f"), ("rgba8", "rgba16f"), ("rgb10a2", "rgba32f"), ("rgb10a2", "rgba8"), ("rgba8", "rgb10a2"),
                     ("rgba8", "bgra8"), ("rgba16f", "bgra8"), ("rgba16f", "rgba8")):
        add(src, 0, 0, 0, -1, 1, 0, 0, dst=dst)
    add("rgba8", 0, 0, 0, -1, 1, 0, 1, dst="rgba32f")
    add("rgb10a2", 0, 0, 0, -1, 0, 0, 0, dst="rgb10a2")       # a float intermediate in front of a 10-bit destination
    add("rgba8", 3, 0, 0, -1, 1, 0, 0, dst="rgba32f")         # exact stores into a float destination
    add("rgba8", 3, 0, 0, -1, 1, 0, 1, dst="rgba16f")
    add("rgba8", 3, 0, 0, -1, 1, 0, 0, dst="bgra8")
    add("ms4_rgba8", 0, 0, 1, -1, 1, 0, 0, dst="rgba32f")     # EASU-only into float: the resolve pass, not the staging resolve
    add("rgba16f", 0, 0, 1, -1, 1, 1, 0, dst="rgba8")
    # 128x96 -> 96x72: the LDS-fit refusals and the runtime-pitch kernels
    for p, nis, sm, fu, m in ((0, 0, 0, -1, 0), (0, 0, 0, -1, 1), (0, 0, 0, 1, 0), (2, 0, 0, 1, 0), (2, 0, 0, -1, 1), (0, 0, 1, -1, 0),
                              (0, 1, 0, -1, 0), (3, 0, 0, -1, 1)):
        add("rgba8", p, nis, sm, fu, 1, 0, m, shape=MINIFY, tag="/minify")
    for p, fu, m in ((0, -1, 1), (0, 1, 0), (2, 1, 0)):
        add("rgba16f", p, 0, 0, fu, 1, 0, m, shape=MINIFY, tag="/minify")
    add("ms4_rgba8", 0, 0, 0, -1, 1, 0, 0, shape=MINIFY, tag="/minify")
    # refusals the factorial does not reach
    add("rgba8", 0, 0, 2, -1, 1, 0, 0, shape=BASE, tag="/unequal")
    add("rgba8", 0, 0, 3, -1, 1, 0, 0, tag="/bad-stage-mask")
    add("rgba8", 1, 0, 0, -1, 1, 0, 0, tag="/bad-precision")
    add("rgba8", 0, 0, 0, -1, 1, 0, 0, shape=(4096, 8, 32, 8), tag="/easu-lds")
    add("rgba8", 0, 0, 1, -1, 1, 0, 1, shape=(4096, 8, 32, 8), tag="/easu-lds")
    out.append(_case("rgba8/render-scale-zero", "rgba8", BASE, dict(render_scale=0.0, out_width=0, out_height=0), 0))
    out.append(_case("rgba8/render-scale-1.5", "rgba8", BASE, dict(render_scale=1.5, out_width=0, out_height=0), 1))
    out.append(_case("rgba8/render-scale-1", "rgba8", BASE, dict(render_scale=1.0, out_width=0, out_height=0, use_nis=1), 0))
    out.append(_case("rgba8/render-scale-1-easu-only", "rgba8", BASE, dict(render_scale=1.0, out_width=0, out_height=0, stage_mask=1), 0))
    # batches: four images with alternating eyes per form; one shared side-by-side batch; pair_submit
    for src, p, nis, sm, fu, m in (("rgba8", 0, 0, 0, -1, 0), ("rgba8", 0, 0, 0, -1, 1), ("rgba8", 0, 0, 0, 0, 1), ("rgba8", 0, 0, 0, 1, 0),
                                   ("rgba8", 0, 0, 0, 1, 1), ("rgba8", 0, 0, 1, -1, 1), ("rgba8", 0, 0, 2, -1, 0), ("rgba8", 0, 1, 0, -1, 1),
                                   ("rgba16f", 0, 0, 0, -1, 1), ("rgba16f", 0, 1, 0, -1, 1), ("rgba16f", 0, 0, 0, -1, 0)):
        add(src, p, nis, sm, fu, 1, 0, m, dst={"rgba8": "rgba8", "rgba16f": "rgba16f"}[src], kind="batch4")
    add("rgba16f", 0, 0, 0, -1, 1, 1, 1, dst="rgba8", kind="batch4")
    add("rgba8", 0, 0, 0, -1, 1, 0, 1, dst="rgba8", kind="shared")
    add("rgba8", 0, 0, 0, -1, 1, 0, 1, kind="pair")
    add("rgba8", 0, 0, 0, -1, 1, 0, 1, dst="bgra8", kind="pair")
    ids = [c["id"] for c in out]
    assert len(set(ids)) == len(ids), "duplicate case ids"
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
_SRC_CACHE = {}


CONTENTS = ("structured", "random")   # tests/synth.structured_u8 (what the record was taken on), tests/synth.random_u8


def source_array(src, w, h, seed, content="structured"):
    """the numpy half of _source: the array that is uploaded (the content generator's uint8 image in the source's format) and its
    ovrfsr_format override.  tests/forms_model.decoded() reads the image the pipeline sees from this same array."""
    import numpy as np
    from tests import synth
    gen = {"structured": synth.structured_u8, "random": synth.random_u8}[content]
    u8 = gen(w, h, seed)
    fmt = None
    if src == "rgba8":
        a = u8
    elif src == "bgra8":
        a, fmt = np.ascontiguousarray(u8[..., [2, 1, 0, 3]]), BGRA8
    elif src in ("rgba16f", "rgba32f"):
        f = u8.astype(np.float32) / np.float32(255)
        a = f.astype(np.float16) if src == "rgba16f" else f
    elif src == "rgb10a2":
        v = u8.astype(np.uint32) * 4 + (u8.astype(np.uint32) >> 6)
        a = (v[..., 0] | v[..., 1] << 10 | v[..., 2] << 20 | np.uint32(3) << 30).view(np.int32)
    elif src == "r11g11b10f":
        v = u8.astype(np.uint32)  # finite words only: exponent fields stay below 31
        a, fmt = (v[..., 0] * 4 | (v[..., 1] * 4) << 11 | (v[..., 2] * 2) << 22).view(np.int32), R11G11B10F
    elif src == "ms4_rgba8":
        a = np.stack([gen(w, h, seed + 10 * s) for s in range(4)], axis=2)
    elif src == "ms2_rgba16f":
        a = np.stack([(gen(w, h, seed + 10 * s).astype(np.float32) / np.float32(255)).astype(np.float16) for s in range(2)], axis=2)
    else:
        raise ValueError(src)
    return a, fmt


def _source(src, w, h, seed, content="structured"):
    """the device tensor of an eye image (source_array, uploaded) and its ovrfsr_format override"""
    import torch
    key = (src, w, h, seed, content)
    if key in _SRC_CACHE:
        return _SRC_CACHE[key]
    a, fmt = source_array(src, w, h, seed, content)
    _SRC_CACHE[key] = (torch.from_numpy(a).to(torch.device("cuda")), fmt)
    return _SRC_CACHE[key]


def _dest(dst, ow, oh, n=None):
    import torch
    dev = torch.device("cuda")
    lead = () if n is None else (n,)
    if dst == "rgb10a2":
        return torch.zeros(lead + (oh, ow), dtype=torch.int32, device=dev), None
    dt = {"rgba8": torch.uint8, "bgra8": torch.uint8, "rgba16f": torch.float16, "rgba32f": torch.float32}[dst]
    return torch.zeros(lead + (oh, ow, 4), dtype=dt, device=dev), (BGRA8 if dst == "bgra8" else None)


def sha_of(arrays):
    """the SHA-256 the record holds, of the output arrays in the order run_case hands them back"""
    h = hashlib.sha256()
    for a in arrays:
        h.update(a.tobytes())
    return h.hexdigest()


def _host(*tensors):
    import torch
    torch.cuda.synchronize()
    return [t.contiguous().cpu().numpy() for t in tensors]


def run_case(case, content="structured", arrays=False):
    """-> {"calls": [[status, text], ...], "owned_format": format or None, "sha256": hex or None}; "create": status where ovrfsr_create refused.
    content: the generator of the eye images (CONTENTS; the record is taken on "structured").  arrays = True adds "arrays": the outputs
    that were hashed, as numpy arrays in the order they were hashed (None where nothing was)."""
    import torch
    import openvr_fsr_amd as A
    from openvr_fsr_amd.postprocessor import _wrap, image_of
    L = A.library()
    iw, ih, ow, oh = case["shape"]
    cfg = A.Config.default(**case["cfg"])
    try:
        pp = A.PostProcessor(cfg)
    except A.OvrFsrError as e:   # a configuration ovrfsr_create refuses never reaches the launch manager: no call to record
        return dict(create=int(e.status), calls=[], owned_format=None, sha256=None)
    calls = []

    def call(rc):
        calls.append([int(rc), (L.ovrfsr_last_error(pp._ctx) or b"").decode() if rc != 0 else ""])
        return rc

    rec = dict(calls=calls, owned_format=None, sha256=None)
    if arrays:
        rec["arrays"] = None

    def done(*tensors):
        host = _host(*tensors)
        rec["sha256"] = sha_of(host)
        if arrays:
            rec["arrays"] = host
    kind, src, dst = case["kind"], case["src"], case["dst"]
    try:
        if kind in ("batch4", "shared"):
            n = 4 if kind == "batch4" else 2
            t0, fmt = _source(src, iw, ih, 3, content)
            t1, _ = _source(src, iw, ih, 4, content)
            texs = torch.stack([t0, t1] * (n // 2))
            outs, ofmt = _dest(dst, ow, oh, n)
            i0, o0 = image_of(texs[0], fmt), image_of(outs[0], ofmt)
            args = (C.byref(i0), texs.stride(0) * texs.element_size(), C.byref(o0), outs.stride(0) * outs.element_size(), pp._stream())
            for _ in range(2):
                rc = call(L.ovrfsr_apply_batch(pp._ctx, n, 0, 1, *args) if kind == "batch4" else L.ovrfsr_apply_batch_shared(pp._ctx, n, *args))
                if rc == 0:
                    done(outs)
                    break
            return rec
        eyes = (0, 1) if kind == "pair" else (0,)
        if kind == "pair":
            cfg.pair_submit = 1
            pp.set_config(cfg)
        results = []
        for eye in eyes:
            tex, fmt = _source(src, iw, ih, 3 + eye, content)
            img = image_of(tex, fmt)
            out, ofmt = (None, None) if dst == "owned" else _dest(dst, ow, oh)
            oimg = image_of(out, ofmt) if out is not None else A.Image()
            for _ in range(2):
                rc = call(L.ovrfsr_apply(pp._ctx, eye, C.byref(img), None, C.byref(oimg), pp._stream()))
                if rc == 0:
                    break
            if rc != 0:
                return rec
            if out is None:
                rec["owned_format"] = int(oimg.format)
                out = tex if oimg.data == tex.data_ptr() else _wrap(oimg, tex.device)
            results.append(out)
        done(*results)
        return rec
    finally:
        torch.cuda.synchronize()
        pp.close()


def record():
    return {c["id"]: run_case(c) for c in cases()}


def main():
    out = sys.argv[1]
    rec = record()
    with open(out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    ok = sum(1 for r in rec.values() if r["calls"] and r["calls"][-1][0] == 0)
    print("%d cases recorded, %d end in OK, %d in a refusal -> %s" % (len(rec), ok, len(rec) - ok, out))


if __name__ == "__main__":
    main()
