"""Frames for the tests of rdoq_wave's passes after the walk (last position, signs, sign hiding on lane registers):
shared by tests/test_rdoq_tail_emu.py (emulator) and tests/test_gpu_rdoq_tail.py (device); not a test module itself.

  textured 64x64, QP 22      one CTU, many levels: sign hiding changes levels in 4x4 blocks, in lower groups of 8x8 blocks and in
                             larger blocks, clears last levels, meets equal costs
  textured 64x64, QP 37      few levels: blocks the last-position search zeroes, 8x8 groups zeroed by costZeroCG, 8x8 blocks
                             whose top candidate level is in group 0
  mixed    128x64, QP 32     two CTUs, smooth and textured regions
  textured 128x128, QP 27    four CTUs
  lowdelay_P clip            two 128x64 pictures: the inter RQT's calls, luma and chroma (8x8 and larger)
"""
import numpy as np

INTRA_CASES = [("textured", 64, 64, 22), ("textured", 64, 64, 37), ("mixed", 128, 64, 32), ("textured", 128, 128, 27)]
LDP_CLIP = ("textured", 128, 64, 27, 3, 2, 8)                  # generator, width, height, base QP, seed, pictures, search range
# fcu_emu_tail_cnt, csrc/fcu_engine.h
COUNTERS = ["sh_4x4", "sh_8x8_low", "sh_big", "sh_tie", "sh_cleared_last", "last_zero", "cg_zeroed_8x8", "top_in_group0_8x8",
            "chroma", "inter", "sh_no_finite"]
MUST_BE_ZERO = "sh_no_finite"                                  # a group in which no position has a finite sign-hiding cost


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
