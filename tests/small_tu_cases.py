"""Frames for the tests of the 4x4 / 8x8 trials (register path of pu_first_pass_batched): shared by
tests/test_small_tu_emu.py (emulator) and tests/test_gpu_small_tu.py (device); not a test module itself.

  textured 64x64, QP 22 / QP 37   one CTU: many / few non-zero 4x4 and 8x8 blocks, trials whose levels are all zero,
                                  4x4 PUs with 17-20 candidate variants, chroma 4x4 trials
  textured 72x80, QP 32           partial right and bottom CTUs: 8x8 CUs at the picture edges, missing neighbours
  noise    64x64, QP 32           flat with sparse single-sample noise: transform skip wins for some 4x4 PU
"""
import numpy as np

CASES = [("textured", 64, 64, 22), ("textured", 64, 64, 37), ("textured", 72, 80, 32), ("noise", 64, 64, 32)]
COUNTERS = ["ts_winner", "all_zero", "batch_over_16", "chroma_4x4"]       # fcu_emu_small_cnt, csrc/fcu_engine.h


def frame(pkg, source, w, h):
    if source == "textured":
        return pkg.synth.textured(w, h, seed=13)
    rng = np.random.RandomState(5)
    Y = np.full((h, w), 100, np.uint8)
    hit = rng.rand(h, w) < 0.06                       # isolated samples far from the flat level: a 4x4 block with one spike
    Y[hit] = rng.choice([20, 230], size=int(hit.sum()))
    U = np.full((h // 2, w // 2), 128, np.uint8)
    V = np.full((h // 2, w // 2), 128, np.uint8)
    return Y, U, V
