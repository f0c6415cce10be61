"""Frames for the tests of the group loads in the lane-private walks (rdoq<0>, and the bit counter that follows it): small pictures whose
transform units meet the edge cases of those walks.  Shared by tests/test_walk_prefetch_emu.py (emulator) and
tests/test_gpu_walk_prefetch.py (device); not a test module itself.

  flat      every sample 128: all residuals are zero (all-zero TUs, the walks return before their first load)
  impulse   flat with one bright sample per CTU: a few low-frequency levels (the only non-zero level in group 0)
  checker   flat with a one-sample checkerboard of small amplitude in a 32x32 block and three 8x8 blocks: the energy sits in
            the highest frequencies (the only non-zero level in the last coefficient group of a TU)
  stripes   a 32x32 block of horizontal stripes whose rows carry a weak ramp, next to flat blocks: levels at both ends of a
            32x32 TU's scan with empty runs between them
  textured  synth.textured: dense levels, 4x4 PUs with 17-20 candidate variants
"""
import numpy as np

SIZES = [(64, 64), (128, 64)]
QPS = [22, 37]
SOURCES = ["flat", "impulse", "checker", "stripes", "textured"]
CASES = [(s, w, h, qp) for s in SOURCES for (w, h) in SIZES for qp in QPS]


def frame(pkg, source, w, h):
    if source == "textured":
        return pkg.synth.textured(w, h, seed=13)
    Y = np.full((h, w), 128, np.uint8)
    U = np.full((h // 2, w // 2), 128, np.uint8)
    V = np.full((h // 2, w // 2), 128, np.uint8)
    for x0 in range(0, w, 64):
        if source == "impulse":
            Y[21, x0 + 37] = 250
        elif source == "checker":
            yy, xx = np.mgrid[0:32, 0:32]
            Y[0:32, x0:x0 + 32] = 128 + 6 * (((xx + yy) & 1) * 2 - 1)
            Y[40:48, x0 + 40:x0 + 48] = 128 + 9 * (((xx[:8, :8] + yy[:8, :8]) & 1) * 2 - 1)
            for bx, amp in ((8, 1), (24, 5)):       # an 8x8 TU keeps one level, at its highest frequency: amplitude 1 at QP 22, 5 at QP 37
                Y[48:56, x0 + bx:x0 + bx + 8] = 128 + amp * (((xx[:8, :8] + yy[:8, :8]) & 1) * 2 - 1)
        elif source == "stripes":
            yy, xx = np.mgrid[0:32, 0:32]
            Y[32:64, x0:x0 + 32] = np.clip(128 + 20 * ((yy & 1) * 2 - 1) + (xx - 16), 0, 255)
    return Y, U, V
