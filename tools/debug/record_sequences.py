#!/usr/bin/env python3
"""tools/debug/record_sequences.py -- what cfg.pair_submit DOES for sequences of submissions, as a record two builds can be compared by.

Every case is a fresh ctx driven through the C ABI: 80x64 -> 160x128, RGBA8, pair_submit = 1, the mask of tools/debug/record_forms.py (the
eyes' centres differ, so a batch of two takes the split eye passes).  Recorded per call: status, error text, ovrfsr_pair_pending and WHICH
image came back in *out (the caller's output of that call, an earlier one, the input, or a ctx-owned image by its offset from the first
owned pointer seen for the current input size).  Recorded per case, after one synchronisation at the end: the SHA-256 of every output image
(a ctx-owned image whose eye is still only recorded was never written and is left out).
tests/golden/submit_sequences_parent.json is this record taken at the commit BEFORE the submission sequencer (csrc/submit_sequence.cpp);
tests/test_gpu_submit_sequences.py runs the same matrix on the tree under test and asserts equality, tests/test_submit_sequence.py holds
the sequencer to the record's pair_pending flags without a GPU.

    python tools/debug/record_sequences.py OUT.json        (GPU)

The matrix (cases()):
  * all 126 eye sequences of length 1 to 6, once with caller-owned outputs and once with ctx-owned ones ("plain/<LR...>/<caller|owned>");
  * scripted cases: an apply_batch between the eyes; an input-size change with a recorded eye (ctx-owned and caller-owned output); reset and
    set_config with a recorded eye; a first eye recorded with a caller-owned output followed by ctx-owned ones (the owned image would have
    to grow under it); an unpairable second eye (another pitch, the same texture, an output overlapping the first input); a shared
    side-by-side texture (bounds 0,0,.5,1 / .5,0,1,1) submitted as L,R with one pointer and with two; no stage selected (stage_mask = 1 at render_scale 1), and NVSharpen at render_scale 1.

A script is a list of events.  ("apply", eye, tex, out[, bounds]): `tex` names the input -- "t<seed>" an 80x64 image, "t<seed>@WxH" another
size, "t<seed>/p<W>" the 80x64 image in rows W texels long, "u<seed>" the 80x64 image at the start of the buffer "U" --, `out` the output:
"o<k>" a caller-owned 160x128 image, "U" the caller-owned 160x128 image that begins where "u<seed>" does, None a ctx-owned one.
("batch", tex0, tex1, out0): ovrfsr_apply_batch of the two, alternating eyes, into the images o<k>, o<k+1>.  ("reset",), ("set_config", {...}).
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

IW, IH, OW, OH = 80, 64, 160, 128
MASK_ON = dict(radius=0.5, proj_centre=(0.2, 0.3, 0.8, 0.7))   # tools/debug/record_forms.py
BASE_CFG = dict(fsr_enabled=1, sharpness=0.9, pair_submit=1, out_width=OW, out_height=OH, **MASK_ON)
LEFT_HALF, RIGHT_HALF = (0.0, 0.0, 0.5, 1.0), (0.5, 0.0, 1.0, 1.0)


def plain_sequences():
    return ["".join(p) for n in range(1, 7) for p in itertools.product("LR", repeat=n)]


def plain_script(seq, owned):
    return [("apply", "LR".index(e), "t%d" % (3 + k), None if owned else "o%d" % k) for k, e in enumerate(seq)]


def cases():
    out = []
    for seq in plain_sequences():
        for owned in (False, True):
            out.append(dict(id="plain/%s/%s" % (seq, "owned" if owned else "caller"), cfg={}, script=plain_script(seq, owned)))

    def add(cid, script, **cfg):
        out.append(dict(id="scripted/" + cid, cfg=cfg, script=script))

    L, R = 0, 1
    add("batch-between-the-eyes", [("apply", L, "t3", "o0"), ("batch", "t4", "t5", "o1"), ("apply", R, "t6", "o3"), ("apply", L, "t7", "o4"), ("apply", R, "t8", "o5")])
    add("size-change-recorded-owned", [("apply", L, "t3", None), ("apply", L, "t4@96x80", None), ("apply", R, "t5@96x80", None),
                                       ("apply", L, "t6@96x80", None), ("apply", R, "t7@96x80", None)])
    add("size-change-recorded-caller", [("apply", L, "t3", "o0"), ("apply", L, "t4@96x80", "o1"), ("apply", R, "t5@96x80", "o2"),
                                        ("apply", L, "t6@96x80", "o3"), ("apply", R, "t7@96x80", "o4")])
    add("size-change-second-eye-owned", [("apply", L, "t3", None), ("apply", R, "t4@96x80", None), ("apply", L, "t5@96x80", None), ("apply", R, "t6@96x80", None)])
    # ... after the order R,L has been learned: the implicit reset keeps it where it keeps the ctx-owned image of the flushed eye
    for dst in ("owned", "caller"):
        o = (lambda k: None) if dst == "owned" else (lambda k: "o%d" % k)
        add("size-change-learned-order-" + dst, [("apply", R, "t3", o(0)), ("apply", L, "t4", o(1)), ("apply", R, "t5", o(2)), ("apply", L, "t6@96x80", o(3)),
                                                 ("apply", R, "t7@96x80", o(4)), ("apply", L, "t8@96x80", o(5)), ("apply", R, "t9@96x80", o(6))])
    add("reset-recorded", [("apply", L, "t3", "o0"), ("reset",), ("apply", R, "t4", "o1"), ("apply", L, "t5", "o2"), ("apply", R, "t6", "o3")])
    add("reset-after-learning", [("apply", R, "t3", "o0"), ("apply", L, "t4", "o1"), ("apply", R, "t5", "o2"), ("reset",),
                                 ("apply", L, "t6", "o3"), ("apply", R, "t7", "o4")])
    add("set-config-recorded", [("apply", L, "t3", "o0"), ("set_config", dict(sharpness=0.5)), ("apply", R, "t4", "o1"), ("apply", L, "t5", "o2"),
                                ("apply", R, "t6", "o3")])
    add("owned-grows-under-recorded", [("apply", L, "t3", "o0"), ("apply", R, "t4", None), ("apply", L, "t5", None), ("apply", R, "t6", "o1")])
    add("unpairable-pitch", [("apply", L, "t3", "o0"), ("apply", R, "t4/p96", "o1"), ("apply", L, "t5", "o2"), ("apply", R, "t6/p96", "o3")])
    add("unpairable-same-texture", [("apply", L, "t3", "o0"), ("apply", R, "t3", "o1"), ("apply", L, "t3", "o2"), ("apply", R, "t3", "o3")])
    add("unpairable-output-over-first-input", [("apply", L, "u3", "o0"), ("apply", R, "t4", "U"), ("apply", L, "u3", "o1"), ("apply", R, "t5", "U")])
    add("shared-one-pointer", [("apply", L, "t3", "o0", LEFT_HALF), ("apply", R, "t3", "o1", RIGHT_HALF), ("apply", L, "t4", "o2", LEFT_HALF),
                               ("apply", R, "t4", "o3", RIGHT_HALF)])
    add("shared-two-pointers", [("apply", L, "t3", "o0", LEFT_HALF), ("apply", R, "t4", "o1", RIGHT_HALF), ("apply", L, "t3", "o2", LEFT_HALF),
                                ("apply", R, "t4", "o3", RIGHT_HALF)])
    add("shared-one-pointer-owned", [("apply", L, "t3", None, LEFT_HALF), ("apply", R, "t3", None, RIGHT_HALF)])
    add("no-stage-stage-mask", [("apply", L, "t3", None), ("apply", R, "t4", None), ("apply", L, "t3", "o0")], stage_mask=1, render_scale=1.0, out_width=0, out_height=0)
    add("render-scale-1-nis-sharpens", [("apply", L, "t3", None), ("apply", R, "t4", None)], use_nis=1, render_scale=1.0, out_width=0, out_height=0)
    ids = [c["id"] for c in out]
    assert len(set(ids)) == len(ids), "duplicate case ids"
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
_TEX_CACHE = {}


def _texture(name, scratch):
    """name -> device tensor [H, W, 4] uint8 (a view where the name asks for a pitch or a place)"""
    import torch
    from tests import synth
    dev = torch.device("cuda")
    if name[0] == "u":   # rewritten at every use: the case overwrites it
        t = scratch["U"].view(-1)[:IW * IH * 4].view(IH, IW, 4)
        t.copy_(torch.from_numpy(synth.structured_u8(IW, IH, int(name[1:]))).to(dev))
        return t
    if name in _TEX_CACHE:
        return _TEX_CACHE[name]
    seed, w, h, pitch = name[1:], IW, IH, None
    if "@" in seed:
        seed, size = seed.split("@")
        w, h = (int(x) for x in size.split("x"))
    elif "/p" in seed:
        seed, pitch = seed.split("/p")
    t = torch.from_numpy(synth.structured_u8(w, h, int(seed))).to(dev)
    if pitch:
        wide = torch.zeros((h, int(pitch), 4), dtype=torch.uint8, device=dev)
        wide[:, :w] = t
        t = wide[:, :w]
    _TEX_CACHE[name] = t
    return t


def run_case(case):
    """-> {"calls": [[status, text, pair_pending, image name or None], ...], "sha256": {image name: hex}}"""
    import torch
    import openvr_fsr_amd as A
    from openvr_fsr_amd.postprocessor import _wrap, image_of
    lib = A.library()
    dev = torch.device("cuda")
    cfg_kw = dict(BASE_CFG)
    cfg_kw.update(case["cfg"])
    pp = A.PostProcessor(A.Config.default(**cfg_kw))
    calls, outs, names, owned = [], {}, {}, {}   # names: device address -> image name; owned: name -> ovrfsr_image
    scratch = {"U": torch.zeros((OH, OW, 4), dtype=torch.uint8, device=dev)}
    owned_base, owned_size, generation = None, None, -1

    def output(name):
        if name == "U":
            return scratch["U"]
        if name not in outs:
            outs[name] = torch.zeros((OH, OW, 4), dtype=torch.uint8, device=dev)
        return outs[name]

    def done(rc, image=None):
        calls.append([int(rc), (lib.ovrfsr_last_error(pp._ctx) or b"").decode() if rc != 0 else "", int(lib.ovrfsr_pair_pending(pp._ctx)), image])

    try:
        for ev in case["script"]:
            if ev[0] == "reset":
                done(lib.ovrfsr_reset(pp._ctx))
            elif ev[0] == "set_config":
                cfg_kw.update(ev[1])
                cfg = A.Config.default(**cfg_kw)
                done(lib.ovrfsr_set_config(pp._ctx, C.byref(cfg)))
            elif ev[0] == "batch":
                texs = torch.stack([_texture(ev[1], scratch), _texture(ev[2], scratch)])
                k = int(ev[3][1:])
                pair = torch.zeros((2, OH, OW, 4), dtype=torch.uint8, device=dev)
                outs["o%d" % k], outs["o%d" % (k + 1)] = pair[0], pair[1]
                i0, o0 = image_of(texs[0]), image_of(pair[0])
                done(lib.ovrfsr_apply_batch(pp._ctx, 2, 0, 1, C.byref(i0), texs.stride(0), C.byref(o0), pair.stride(0), pp._stream()))
                scratch.setdefault("keep", []).append(texs)
            else:
                _, eye, tex_name, out_name = ev[:4]
                tex = _texture(tex_name, scratch)
                names[tex.data_ptr()] = tex_name
                img = image_of(tex)
                if out_name is None:
                    oimg = A.Image()
                else:
                    o = output(out_name)
                    names[o.data_ptr()] = out_name
                    oimg = image_of(o)
                bounds = A.Bounds(*ev[4]) if len(ev) > 4 else None
                rc = lib.ovrfsr_apply(pp._ctx, eye, C.byref(img), C.byref(bounds) if bounds is not None else None, C.byref(oimg), pp._stream())
                image = None
                if rc == 0:
                    image = names.get(oimg.data)
                    if image is None:   # a ctx-owned image: by its offset from the first one seen for this input size
                        if owned_size != (img.width, img.height):
                            owned_base, owned_size, generation = oimg.data, (img.width, img.height), generation + 1
                        image = "owned%d%+d" % (generation, oimg.data - owned_base)
                        owned[image] = A.Image(oimg.data, oimg.width, oimg.height, oimg.pitch_bytes, oimg.format)
                done(rc, image)
        torch.cuda.synchronize()
        unwritten = calls[-1][3] if calls and calls[-1][2] else None   # still only recorded: a ctx-owned image nothing was written to
        sha = {}
        for name, t in sorted(list(outs.items()) + ([("U", scratch["U"])] if "U" in names.values() else [])):
            sha[name] = hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()
        for name, im in sorted(owned.items()):
            if name != unwritten:
                sha[name] = hashlib.sha256(_wrap(im, dev).contiguous().cpu().numpy().tobytes()).hexdigest()
        return dict(calls=calls, sha256=sha)
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
    print("%d cases, %d calls recorded -> %s" % (len(rec), sum(len(r["calls"]) for r in rec.values()), out))


if __name__ == "__main__":
    main()
