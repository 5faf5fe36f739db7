#!/usr/bin/env python3
"""Why ovrfsr_set_hdr_domain exists, as a picture, from the CPU oracle alone (no GPU, no library): a 1-texel highlight of 4096 on a 0.25
field, 32x32 -> 64x64 at sharpness 0.9, filtered as submitted -- oracle.rcas(oracle.easu(x)) -- and in FSR 1's reversible tone-mapped
domain -- the numpy mapping of tests/hdrmap.py around the same two calls.  Prints the output rows through the highlight.  Recorded in
profiles/hdr_domain.txt; nothing is asserted.

    python tests/debug/hdr_picture.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    import numpy as np
    from oracle import oracle as O
    from tests import hdrmap
    w = h = 32
    x = np.full((h, w, 4), 0.25, np.float32)
    x[..., 3] = 1.0
    x[16, 16, :3] = 4096.0
    con, rcon = O.easu_con(w, h, 2 * w, 2 * h), O.rcas_con(0.9, 0)
    centre, rad = O.mask_constants(2 * w, 2 * h)
    linear = O.rcas(O.easu(x, 2 * w, 2 * h, con, centre, rad), rcon, centre, rad)
    mapped = hdrmap.back(O.rcas(O.easu(hdrmap.forward(x), 2 * w, 2 * h, con, centre, rad), rcon, centre, rad))
    np.set_printoptions(linewidth=200, suppress=True, precision=3)
    print("1-texel highlight of 4096 on a 0.25 field, 32x32 -> 64x64, sharpness 0.9: red channel, output rows 30..35, columns 26..39")
    for name, img in (("filtered as submitted", linear), ("filtered in the mapped domain", mapped)):
        win = img[30:36, 26:40, 0]
        print(name)
        print(win)
        field = np.abs(img[..., 0] - 0.25) > 0.0025
        print("  pixels more than 1 %% off the field: %d; smallest value %.4g, largest %.4g, sum over the image %.1f" %
              (int(field.sum()), float(img[..., 0].min()), float(img[..., 0].max()), float(img[..., 0].astype(np.float64).sum())))


if __name__ == "__main__":
    main()
