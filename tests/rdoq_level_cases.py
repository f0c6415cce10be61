"""Frames for the tests of level_choice() (the level choice of RDOQ's first loop and the rates of its record in one pass,
DESIGN.md 3): shared by tests/test_rdoq_level_emu.py (emulator) and tests/test_gpu_rdoq_level.py (device); not a test module
itself.

  mixed    64x64,  QP 22     one CTU, sharp edges at a low QP: large levels, Rice parameter up to 4, remainders in the escape branch
  textured 64x64,  QP 37     few levels: uiMaxAbsLevel 1 and 2, levels RDOQ lowers or zeroes
  textured 128x64, QP 22     two CTUs, many levels: groups with eight and more levels (c1Idx >= 8), c2Idx >= 1
  mixed    128x64, QP 37     two CTUs, smooth and textured regions
  lowdelay_P clip            two 128x64 pictures: the inter RQT's rdoq_wave calls, luma and chroma
"""
import numpy as np

INTRA_CASES = [("mixed", 64, 64, 22), ("textured", 64, 64, 37), ("textured", 128, 64, 22), ("mixed", 128, 64, 37)]
LDP_CLIP = ("textured", 128, 64, 27, 3, 2, 8)                  # generator, width, height, base QP, seed, pictures, search range
# fcu_emu_level_cnt, csrc/fcu_engine.h
COUNTERS = ["max1", "max2", "max3up", "chose_lower", "chose_zero", "last", "c1idx_8up", "c2idx_1up", "rice0", "rice4",
            "escape_at", "escape_above", "symbol_32768up"]
MUST_BE_ZERO = "symbol_32768up"                                # levels are clipped to 32767: no remainder reaches 32768


def frame(pkg, source, w, h):
    return getattr(pkg.synth, source)(w, h, seed=13)


def ldp_pictures(pkg):
    """the clip's pictures: from the second on, the right half is content the reference picture does not hold"""
    import search_trace as st
    gen, w, h, _, seed, n_pic, _ = LDP_CLIP
    pics = []
    for poc in range(n_pic):
        f = st.moving_frame(pkg.synth, gen, w, h, seed, poc)
        if poc:
            n = st.moving_frame(pkg.synth, "mixed", w, h, seed + 7 * poc, poc)
            f = tuple(np.ascontiguousarray(np.concatenate([a[:, :a.shape[1] // 2], b[:, b.shape[1] // 2:]], axis=1)) for a, b in zip(f, n))
        pics.append(f)
    return pics
