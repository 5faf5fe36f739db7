"""The submission sequencer (csrc/submit_sequence.cpp) without a GPU: tests/debug/sequence_probe.cpp is compiled on the fly with the sequencer
unit -- no HIP, nothing else of the library -- under AddressSanitizer and UBSan, and run as a child process.  Checked: (a) the recorded flags and
launches of known eye sequences, (b) properties over every eye sequence up to length 10, (c) the can-these-two-go-as-one-batch predicate, one
case per condition, (d) the single-submission rule of shared textures, (e) every row of the error-path table (what a failing flush or launch
leaves behind), (f) the ovrfsr_pair_pending flags the library at the commit before the sequencer gave on an MI355X
(tests/golden/submit_sequences_parent.json), for every plain eye sequence of that record."""
import itertools
import json
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openvr_fsr_amd", "csrc")

L, R = 0, 1
IN_BYTES, OUT_BYTES = 80 * 64 * 4, 160 * 128 * 4
U64 = 1 << 64


@pytest.fixture(scope="module")
def probe():
    """the probe, built under the host sanitizers; -> run(script lines) -> one dict per reporting event"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    tmp = tempfile.mkdtemp(prefix="ovrfsr_sequence_probe_")
    exe = os.path.join(tmp, "sequence_probe")
    # (g++ links the sanitizer runtimes dynamically unless told otherwise; linked statically, the probe needs nothing of its environment)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static + [
                    os.path.join(ROOT, "tests", "debug", "sequence_probe.cpp"), os.path.join(CSRC, "submit_sequence.cpp"), "-o", exe], check=True)

    def run(lines):
        path = os.path.join(tmp, "script.txt")
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-4000:]
        return [json.loads(x) for x in r.stdout.splitlines()]

    yield run
    shutil.rmtree(tmp, ignore_errors=True)


def img(addr, w=80, h=64, pitch=None, fmt=0):
    return "%d %d %d %d %d" % (addr, w, h, pitch if pitch is not None else w * 4, fmt)


def out_img(addr, **kw):
    return img(addr, **dict(dict(w=160, h=128), **kw))


def tex_at(k):
    return 0x100000 + k * 0x10000      # 80x64 RGBA8 images, disjoint


def out_at(k):
    return 0x800000 + k * 0x20000      # 160x128 RGBA8 images, disjoint from each other and from the inputs


def apply(eye, tex, dst, pair=1, stages=1, one=1):
    """tex, dst: an address (80x64 / 160x128 RGBA8, tight pitch) or a descriptor string"""
    return "apply %d %s %s %d %d %d" % (eye, img(tex) if isinstance(tex, int) else tex, out_img(dst) if isinstance(dst, int) else dst, pair, stages, one)


def plain(seq, pairable=True):
    """one Apply per eye of seq ("LRL..."); pairable: every call its own texture -- or one texture for all of them, which never pairs"""
    return ["new"] + [apply("LR".index(e), tex_at(k if pairable else 0), out_at(k)) for k, e in enumerate(seq)]


def flags(events):
    return "".join(str(e["state"]["pair_pending"]) for e in events)


# ---- (a) known sequences --------------------------------------------------------------------------------------------------------------
KNOWN = [("LRLRLR", "101010"), ("RLRLRL", "101010"), ("LLLRLR", "100010"), ("LLRLRLRL", "10010101"), ("LRRLRL", "100101"), ("LRLLRLR", "1010010")]


def test_known_sequences(probe):
    for seq, want in KNOWN:
        ev = probe(plain(seq))
        assert flags(ev) == want, (seq, flags(ev))
        assert [e["state"]["recorded"] for e in ev] == [int(c) for c in want]
    ev = probe(plain("LLLRLR"))
    assert [e["launches"] for e in ev] == [[], [[0], [1]], [[2]], [[3]], [], [[4, 5]]]
    assert [e["steps"] for e in ev] == [["record"], ["flush", "single"], ["single"], ["single"], ["record"], ["pair"]]


# ---- (b) properties over every eye sequence up to length 10 ---------------------------------------------------------------------------
def _runs(probe, seqs, pairable):
    lines = []
    for s in seqs:
        lines += plain(s, pairable)
    ev = probe(lines)
    assert len(ev) == sum(len(s) for s in seqs)
    out, i = [], 0
    for s in seqs:
        out.append(ev[i:i + len(s)])
        i += len(s)
    return out


@pytest.mark.parametrize("pairable", [True, False], ids=["pairable", "unpairable"])
def test_every_submission_is_launched_once_in_order_and_soon(probe, pairable):
    seqs = ["".join(p) for n in range(1, 11) for p in itertools.product("LR", repeat=n)]
    assert len(seqs) == 2046   # (x 2 predicates = 4092 runs)
    for seq, ev in zip(seqs, _runs(probe, seqs, pairable)):
        launched = []
        for k, e in enumerate(ev):
            assert e["failed"] is None
            now = [c for batch in e["launches"] for c in batch]
            assert all(c in (k - 1, k) for c in now), (seq, k, e["launches"])           # no later than the end of the following call
            assert all(len(batch) == 1 for batch in e["launches"]) or pairable, (seq, k)  # an unpairable pair goes as two single launches
            launched += now
            assert e["state"]["pending"] == (k not in launched), (seq, k)
            assert e["state"]["pair_pending"] == e["state"]["recorded"] == (k not in launched), (seq, k)
            if k:
                assert not (e["state"]["recorded"] and ev[k - 1]["state"]["recorded"]), (seq, k)   # never two recorded calls in a row
        n = len(seq)
        assert launched == list(range(n if not ev[-1]["state"]["pending"] else n - 1)), (seq, launched)   # exactly once, in arrival order


def test_an_alternating_tail_pairs_again_within_one_call(probe):
    """after any prefix of up to six calls, eyes that alternate from the prefix's last eye on are recorded and paired, recorded and paired, ...
    from the tail's second call at the latest"""
    prefixes = [""] + ["".join(p) for n in range(1, 7) for p in itertools.product("LR", repeat=n)]
    seqs, cut = [], []
    for p in prefixes:
        for first in ("LR" if not p else "R" if p[-1] == "L" else "L"):
            tail = "".join("LR"[("LR".index(first) + i) & 1] for i in range(8))
            seqs.append(p + tail)
            cut.append(len(p))
    for seq, n, ev in zip(seqs, cut, _runs(probe, seqs, True)):
        steps = [e["steps"] for e in ev[n:]]
        start = 0 if steps[0] in (["record"], ["pair"]) and steps[1] in (["record"], ["pair"]) else 1
        want = [["record"], ["pair"]]
        k0 = want.index(steps[start]) if steps[start] in want else None
        assert k0 is not None, (seq, n, steps)
        assert steps[start:] == [want[(k0 + i) & 1] for i in range(len(steps) - start)], (seq, n, steps)


# ---- (c) the pairable predicate ---------------------------------------------------------------------------------------------------------
def _pairable(probe, fi, fo, si, so):
    return probe(["pairable %s %s %s %s" % (fi, fo, si, so)])[0]


def test_pairable_predicate(probe):
    A, B, OA, OB = tex_at(0), tex_at(1), out_at(0), out_at(1)
    ok = _pairable(probe, img(A), out_img(OA), img(B), out_img(OB))
    assert ok == dict(pairable=1, in_stride=B - A, out_stride=OB - OA)
    negative = {
        "another input pitch": (img(A), out_img(OA), img(B, pitch=384), out_img(OB)),
        "another output pitch": (img(A), out_img(OA), img(B), out_img(OB, pitch=768)),
        "another size": (img(A), out_img(OA), img(B, w=64), out_img(OB)),
        "another output size": (img(A), out_img(OA), img(B), out_img(OB, h=96)),
        "another format": (img(A, fmt=3), out_img(OA), img(B), out_img(OB)),
        "another output format": (img(A), out_img(OA), img(B), out_img(OB, fmt=3)),
        "one texture for both eyes": (img(A), out_img(OA), img(A), out_img(OB)),
        "the outputs overlap": (img(A), out_img(OA), img(B), out_img(OA + OUT_BYTES - 4)),
        "first input under second output": (img(A), out_img(OA), img(B), out_img(A - OUT_BYTES + 4)),
        "second input under first output": (img(A), out_img(B + IN_BYTES - 4), img(B), out_img(OB)),
        "first input under first output": (img(A), out_img(A + IN_BYTES - 4), img(B), out_img(OB)),
        "second input under second output": (img(A), out_img(OA), img(B), out_img(B - OUT_BYTES + 4)),
        "input stride no multiple of the texel": (img(A, fmt=1, pitch=640), out_img(OA), img(B + 4, fmt=1, pitch=640), out_img(OB)),
        "output stride no multiple of the texel": (img(A), out_img(OA, fmt=2, pitch=2560), img(B), out_img(OA + 0x100008, fmt=2, pitch=2560)),
    }
    for name, images in negative.items():
        assert _pairable(probe, *images)["pairable"] == 0, name
    # the images just touching are disjoint
    assert _pairable(probe, img(A), out_img(OA), img(B), out_img(OA + OUT_BYTES))["pairable"] == 1
    # the second image BELOW the first: the stride wraps modulo 2^64 -- inputs and outputs independently
    below_in = _pairable(probe, img(B), out_img(OA), img(A), out_img(OB))
    assert below_in == dict(pairable=1, in_stride=U64 - (B - A), out_stride=OB - OA)
    below_out = _pairable(probe, img(A), out_img(OB), img(B), out_img(OA))
    assert below_out == dict(pairable=1, in_stride=B - A, out_stride=U64 - (OB - OA))


def test_pair_launch_carries_the_recorded_eye_and_the_wrapped_strides(probe):
    ev = probe(["new", apply(R, tex_at(1), out_at(1)), apply(L, tex_at(0), out_at(0))])
    assert ev[1]["steps"] == ["pair"] and ev[1]["pair_eye"] == R
    assert (ev[1]["in_stride"], ev[1]["out_stride"]) == (U64 - 0x10000, U64 - 0x20000)
    assert ev[1]["returned"] == out_at(0) and ev[0]["returned"] == out_at(1)


# ---- (d) the single-submission rule -------------------------------------------------------------------------------------------------------
def test_shared_texture_is_processed_once(probe):
    shared = dict(pair=0, one=0)
    ev = probe(["new", apply(L, tex_at(0), out_at(0), **shared), apply(R, tex_at(0), out_at(1), **shared), apply(L, tex_at(0), out_at(2), **shared)])
    assert [e["steps"] for e in ev] == [["single"], ["reuse"], ["single"]]
    assert [e["returned"] for e in ev] == [out_at(0), out_at(0), out_at(2)]
    assert [e.get("single_eye") for e in ev] == [L, None, L]   # (a shared texture carries both eyes: the kernels get LEFT)
    ev = probe(["new", apply(L, tex_at(0), out_at(0), **shared), apply(R, tex_at(1), out_at(1), **shared)])
    assert [e["steps"] for e in ev] == [["single"], ["single"]] and [e["returned"] for e in ev] == [out_at(0), out_at(1)]
    # one texture per eye: the same pointer twice is processed twice, for the eye named
    ev = probe(["new", apply(L, tex_at(0), out_at(0), pair=0), apply(R, tex_at(0), out_at(1), pair=0)])
    assert [e["steps"] for e in ev] == [["single"], ["single"]] and [e["single_eye"] for e in ev] == [L, R]


def test_no_stage_selected_forwards_the_input(probe):
    for one in (0, 1):
        ev = probe(["new", apply(L, tex_at(0), out_at(0), pair=0, stages=0, one=one), apply(R, tex_at(1), out_at(1), pair=0, stages=0, one=one)])
        assert [e["steps"] for e in ev] == [["forward"], ["forward"]] and [e["launches"] for e in ev] == [[], []]
        assert [e["returned"] for e in ev] == [tex_at(0), tex_at(1)]
    ev = probe(["new", apply(L, tex_at(0), out_at(0), pair=0, stages=0, one=0), apply(R, tex_at(0), out_at(1), pair=0, stages=0, one=0)])
    assert [e["steps"] for e in ev] == [["forward"], ["reuse"]] and ev[1]["returned"] == tex_at(0)


# ---- (e) the error-path table ---------------------------------------------------------------------------------------------------------------
def _state(e, *keys):
    return tuple(e["state"][k] for k in keys)


COMMITTED = ("last_texture", "eye_count", "output")


def test_error_same_eye_again(probe):
    pre = ["new", apply(L, tex_at(0), out_at(0))]
    ok = probe(pre + [apply(L, tex_at(1), out_at(1))])
    assert ok[1]["steps"] == ["flush", "single"] and ok[1]["launches"] == [[0], [1]]
    assert _state(ok[1], "pending", "defer", "recorded", "last_eye") == (0, 0, 0, L) and _state(ok[1], *COMMITTED) == (tex_at(1), 0, out_at(1))
    bad = probe(pre + ["fail flush", apply(L, tex_at(1), out_at(1))])
    assert bad[1]["failed"] == "flush" and bad[1]["launches"] == []
    assert _state(bad[1], "pending", "defer", "recorded", "last_eye") == (0, 1, 0, L)      # pending cleared before its launch; defer unchanged
    assert _state(bad[1], *COMMITTED) == _state(bad[0], *COMMITTED)
    bad = probe(pre + ["fail main", apply(L, tex_at(1), out_at(1))])
    assert bad[1]["failed"] == "main" and bad[1]["launches"] == [[0]]
    assert _state(bad[1], "pending", "defer") == (0, 0) and _state(bad[1], *COMMITTED) == _state(bad[0], *COMMITTED)


def test_error_pair(probe):
    pre = ["new", apply(R, tex_at(0), out_at(0))]
    ok = probe(pre + [apply(L, tex_at(1), out_at(1))])
    assert ok[1]["launches"] == [[0, 1]] and _state(ok[1], "first_eye", "defer", "pending", "recorded") == (R, 1, 0, 0)
    assert _state(ok[1], *COMMITTED) == (tex_at(1), 0, out_at(1))
    bad = probe(pre + ["fail main", apply(L, tex_at(1), out_at(1))])
    assert bad[1]["failed"] == "main" and bad[1]["launches"] == []
    assert _state(bad[1], "first_eye", "defer", "pending", "recorded", "last_eye") == (R, 1, 0, 0, L)
    assert _state(bad[1], *COMMITTED) == _state(bad[0], *COMMITTED)


def test_error_unpairable_pair(probe):
    pre = ["new", apply(R, tex_at(0), out_at(0))]
    ok = probe(pre + [apply(L, tex_at(0), out_at(1))])
    assert ok[1]["steps"] == ["flush", "single"] and ok[1]["launches"] == [[0], [1]]
    assert _state(ok[1], "first_eye", "defer", "pending") == (R, 1, 0) and _state(ok[1], *COMMITTED) == (tex_at(0), 0, out_at(1))
    bad = probe(pre + ["fail flush", apply(L, tex_at(0), out_at(1))])
    assert bad[1]["failed"] == "flush" and bad[1]["launches"] == []
    assert _state(bad[1], "first_eye", "defer", "pending") == (R, 1, 0) and _state(bad[1], *COMMITTED) == _state(bad[0], *COMMITTED)
    bad = probe(pre + ["fail main", apply(L, tex_at(0), out_at(1))])
    assert bad[1]["failed"] == "main" and bad[1]["launches"] == [[0]] and _state(bad[1], *COMMITTED) == _state(bad[0], *COMMITTED)


def test_nothing_recorded_rows(probe):
    # !defer: the other eye turns deferring on again, from the next call on; the call itself is a single launch
    ev = probe(plain("LLLR") + [apply(L, tex_at(4), out_at(4))])
    assert [_state(e, "defer") for e in ev] == [(1,), (0,), (0,), (1,), (1,)]
    assert [e["steps"] for e in ev[2:]] == [["single"], ["single"], ["record"]]
    # defer, the frame's first eye unknown or this one: recorded -- pending set, everything committed, nothing launched
    ev = probe(["new", apply(R, tex_at(0), out_at(0))])
    assert ev[0]["steps"] == ["record"] and ev[0]["launches"] == [] and ev[0]["returned"] == out_at(0)
    assert _state(ev[0], "pending", "pending_eye", "pending_in", "pending_out", "recorded") == (1, R, tex_at(0), out_at(0), 1)
    assert _state(ev[0], *COMMITTED) == (tex_at(0), 1, out_at(0))
    # otherwise (a frame's second eye whose partner went alone): single
    ev = probe(plain("LR") + ["batch", apply(R, tex_at(2), out_at(2))])
    assert ev[3]["steps"] == ["single"] and _state(ev[3], "first_eye", "defer", "recorded") == (L, 1, 0)
    # a failing single launch commits nothing
    bad = probe(plain("LR") + ["fail main", apply(R, tex_at(2), out_at(2))])
    assert bad[2]["failed"] == "main" and _state(bad[2], *COMMITTED) == _state(bad[1], *COMMITTED) and _state(bad[2], "last_eye", "recorded") == (R, 0)
    # without pair mode the eye is not tracked
    ev = probe(["new", apply(R, tex_at(0), out_at(0), pair=0)])
    assert _state(ev[0], "last_eye", "recorded") == (-1, 0)


def test_events_from_outside_apply(probe):
    # a batch call: the recorded submission goes first, on its own
    ev = probe(plain("L") + ["batch", "batch"])
    assert ev[1]["steps"] == ["flush"] and ev[1]["launches"] == [[0]] and _state(ev[1], "pending", "pair_pending", "recorded") == (0, 0, 1)
    assert ev[2]["steps"] == [] and ev[2]["launches"] == []
    bad = probe(plain("L") + ["fail flush", "batch"])
    assert bad[1]["failed"] == "flush" and bad[1]["launches"] == [] and _state(bad[1], "pending") == (0,)
    # an explicit reset drops the recorded eye and forgets the learned order
    ev = probe(plain("RLR") + ["reset"])
    assert _state(ev[2], "first_eye", "pending") == (R, 1)
    assert _state(ev[3], "first_eye", "defer", "last_eye", "pending", "recorded", "last_texture", "eye_count", "output") == (-1, 1, -1, 0, 0, 0, 0, 0)
    # the implicit reset of a size change keeps the order where it keeps the flushed eye's ctx-owned image
    ev = probe(plain("RLR") + ["size 1", apply(L, tex_at(3), out_at(3))])
    assert ev[3]["launches"] == [[2]] and _state(ev[3], "first_eye", "last_eye", "pending", "eye_count") == (R, R, 0, 0)
    assert ev[4]["steps"] == ["single"]
    ev = probe(plain("RLR") + ["size 0", apply(L, tex_at(3), out_at(3))])
    assert _state(ev[3], "first_eye", "last_eye") == (-1, -1) and ev[4]["steps"] == ["record"]


# ---- (f) the GPU record of the parent commit ----------------------------------------------------------------------------------------------
def test_recorded_flags_agree_with_the_gpu_record(probe):
    record = json.load(open(os.path.join(ROOT, "tests", "golden", "submit_sequences_parent.json")))
    seqs = sorted({k.split("/")[1] for k in record if k.startswith("plain/")})
    assert len(seqs) == 126
    owned_base = 0x4000000   # two ctx-owned images, left first
    lines = []
    for s in seqs:
        lines += plain(s)
        lines += ["new"] + [apply("LR".index(e), tex_at(k), owned_base + "LR".index(e) * OUT_BYTES) for k, e in enumerate(s)]
    ev = probe(lines)
    i = 0
    for s in seqs:
        for owner in ("caller", "owned"):
            calls = record["plain/%s/%s" % (s, owner)]["calls"]
            got = ev[i:i + len(s)]
            i += len(s)
            assert [c[0] for c in calls] == [0] * len(s)
            assert [e["state"]["pair_pending"] for e in got] == [c[2] for c in calls], (s, owner)
            if owner == "owned":   # ... and the image handed back, by its offset from the first one
                assert ["owned0%+d" % (e["returned"] - got[0]["returned"]) for e in got] == [c[3] for c in calls], s
