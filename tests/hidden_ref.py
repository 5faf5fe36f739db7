"""What tests/test_hidden_area.py and tests/test_gpu_hidden_area.py share: a numpy brute-force restatement of the hidden-area rule
(include/openvr_fsr_amd.h, "hidden-area mesh"), the test meshes, and the planner probe (tests/debug/hidden_probe.cpp) built under the host
sanitizers as a stand-alone program."""
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openvr_fsr_amd", "csrc")


def _fixed(c, n):
    """u or v (float32) -> 1/256-pixel fixed point: clamped to [-4, 4] in double, floor(c * n * 256 + 0.5)"""
    d = np.clip(np.asarray(c, np.float32).astype(np.float64), -4.0, 4.0)
    return np.floor(d * float(n) * 256.0 + 0.5).astype(np.int64)


def hidden_pixels(uv, W, H, x0=0, x1=None):
    """[H, W] bool: the pixels some triangle of the mesh covers; the mesh maps onto columns [x0, x1) and covers nothing outside them"""
    x1 = W if x1 is None else x1
    cover = np.zeros((H, W), bool)
    tris = np.asarray(uv if uv is not None else [], np.float32).reshape(-1, 3, 2)
    if x1 <= x0:
        return cover
    px = (256 * np.arange(W, dtype=np.int64) + 128)[None, :]
    py = (256 * np.arange(H, dtype=np.int64) + 128)[:, None]
    for t in tris:
        X = _fixed(t[:, 0], x1 - x0) + 256 * x0
        Y = _fixed(t[:, 1], H)
        e = []
        for k in range(3):
            k1 = (k + 1) % 3
            e.append((X[k1] - X[k]) * (py - Y[k]) - (Y[k1] - Y[k]) * (px - X[k]))
        area = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
        if area == 0:
            continue
        c = ((e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)) | ((e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0))
        c[:, :x0] = False
        c[:, x1:] = False
        cover |= c
    return cover


def tiles_of(cover, tw, th):
    """[tilesY, tilesX] uint8: 1 where every pixel of (tile & image) is set"""
    H, W = cover.shape
    tx, ty = (W + tw - 1) // tw, (H + th - 1) // th
    out = np.zeros((ty, tx), np.uint8)
    for j in range(ty):
        for i in range(tx):
            out[j, i] = cover[j * th:(j + 1) * th, i * tw:(i + 1) * tw].all()
    return out


def hidden_tiles(uv, W, H, tw=32, th=32):
    return tiles_of(hidden_pixels(uv, W, H), tw, th)


def hidden_tiles_shared(left, right, W, H, tw=32, th=32):
    """a shared side-by-side texture: the left mesh on columns [0, W // 2), the right mesh on [W // 2, W)"""
    return tiles_of(hidden_pixels(left, W, H, 0, W // 2) | hidden_pixels(right, W, H, W // 2, W), tw, th)


def partly_covered(uv, W, H, tw=32, th=32):
    """[tilesY, tilesX] bool: tiles with some but not all pixels hidden"""
    c = hidden_pixels(uv, W, H)
    some = tiles_of(~c, tw, th) == 0
    return some & (tiles_of(c, tw, th) == 0)


# ---- the meshes of the GPU tests ------------------------------------------------------------------------------------------------------
# SYNTHETIC (no headset mesh exists here): per eye a band along the top edge, the two bottom corners and a wedge, different per eye.  Against
# the launch-form matrix's mask (radius 0.5, centres (0.2, 0.3, 0.8, 0.7)) each eye gets hidden tiles next to tiles RCAS processes, hidden
# tiles outside the radius, partly covered tiles and visible outside tiles: tests/test_gpu_hidden_area.py asserts that, case by case.
def rect(u0, v0, u1, v1):
    return [[(u0, v0), (u1, v0), (u1, v1)], [(u0, v0), (u1, v1), (u0, v1)]]


MESH = {
    0: np.asarray(rect(-0.1, -0.1, 1.1, 0.26) + rect(0.79, 0.7, 1.2, 1.2) + [[(0.0, 1.0), (0.0, 0.55), (0.5, 1.0)]], np.float32),
    1: np.asarray(rect(-0.1, 0.74, 1.1, 1.1) + rect(-0.2, -0.2, 0.21, 0.3) + [[(1.0, 0.0), (1.0, 0.45), (0.5, 0.0)]], np.float32),
}
EVERYTHING = np.asarray(rect(-1.0, -1.0, 2.0, 2.0), np.float32)


# ---- the planner probe -----------------------------------------------------------------------------------------------------------------
def build_probe():
    """-> run(lines) -> one dict per case line; run.tmp: its directory (the caller removes it)"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    tmp = tempfile.mkdtemp(prefix="ovrfsr_hidden_probe_")
    exe = os.path.join(tmp, "hidden_probe")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static + [
                    os.path.join(ROOT, "tests", "debug", "hidden_probe.cpp"), os.path.join(CSRC, "pipeline_plan.cpp"),
                    os.path.join(CSRC, "constants.cpp"), os.path.join(CSRC, "nis_config.cpp"), "-o", exe], check=True)

    def run(lines):
        path = os.path.join(tmp, "cases.txt")
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-4000:]
        out = [json.loads(x) for x in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out

    run.tmp = tmp
    return run


def with_mesh(line, left=None, right=None):
    """a case line of tests/debug/plan_probe.cpp + the two meshes, as tests/debug/hidden_probe.cpp reads it"""
    ms = [np.asarray(m if m is not None else [], np.float32).reshape(-1) for m in (left, right)]
    return " ".join([line, str(ms[0].size // 6), str(ms[1].size // 6)] + [repr(float(x)) for m in ms for x in m])
