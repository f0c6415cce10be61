"""The engine source's WaveFrontSynchro row chains of P pictures on the CPU wave emulator (tests/emu/wpp_emu.cpp) against the
P-slice WPP reference (tests/wpp_oracle.py): every fcu_ctu_out field, the reconstruction, each row's final coder state and
the search state (m_integerMv2Nx2N) each row ends with, in all four slots; the emulator's read-before-write count of the TZ
start vectors stays zero."""
import numpy as np
import pytest

import hmo_py
import search_trace as st
from test_wpp_p_oracle import split_motion_clip
from wpp_oracle import wpp_p_clip
from wpp_testlib import assert_ctus_equal, emulate, p_picture_args, wpp_emu  # noqa: F401 (wpp_emu: the fixture)


# gen, w, h, base_qp, n_pic, search range, TZ, references (rps), TMVP, AMP, cabac_b_table
CASES = [
    ("shear_mixed", 256, 112, 30, 3, 16, 1, (2, "recent"), 1, 1, 0),     # partial bottom row (48 high), two references
    ("mixed", 192, 176, 32, 4, 16, 1, (4, "hm"), 0, 0, 1),              # the cfg's reference sets, B tables, partial bottom row
    ("textured", 192, 128, 27, 3, 8, 0, (1, "hm"), 1, 0, 0),            # full search: no slot is ever written
    ("mixed", 192, 48, 30, 4, 16, 1, (1, "hm"), 1, 1, 0),               # one partial row: the search state crosses pictures only
    ("shear_textured", 56, 136, 30, 3, 16, 1, (2, "recent"), 0, 1, 0),  # 56 wide: every row begins on a boundary CTU
]


def _run_case(pkg, wpp_emu, gen, w, h, base_qp, n_pic, sr, fast, nref_rps, tmvp, amp, btab, decision=None, frames=None):
    nref, rps = nref_rps
    if frames is None:
        frames = [st.moving_frame(pkg.synth, gen, w, h, 7, poc) for poc in range(n_pic)]
    res = wpp_p_clip(frames, base_qp, ref_pocs=lambda poc, n: pkg.lowdelay.ref_pocs(poc, n, rps), n_refs=nref, search_range=sr,
                     fast_search=fast, tmvp=tmvp, amp=amp, cabac_b_table=btab, decision=decision)
    int_mv = [(0, 0)] * 4
    n_inter = 0
    for poc in range(1, n_pic):
        R = res[poc]
        o = R["o"]
        qp, p = p_picture_args(res, poc, base_qp, nref, sr, fast, tmvp, amp, btab)
        e = emulate(wpp_emu, frames[poc], qp, p=p, decision=decision, int_mv=int_mv)
        assert e["rbw"] == 0, (poc, "a TZ search read a start vector the row had neither written nor inherited")
        n_inter += assert_ctus_equal(o.enc, e["out"], (poc,))
        for a, b in zip(R["rec_unfiltered"], e["rec"]):
            assert np.array_equal(a, b), (poc, "reconstruction")
        for r in range(o.H):
            assert np.array_equal(e["states"][r][0][st.O_SORTED], o.row_state[r][0][st.O_SORTED]) and e["states"][r][1] == o.row_state[r][1], (poc, r, "coder state")
            assert e["mvs"][r] == o.row_int_mv[r], (poc, r, "search state after the row")
        int_mv = e["mvs"][-1]                                       # the last row's state: the next picture's row 0
        assert int_mv == R["int_mv"]
    assert n_inter > 0
    return res


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}_{c[1]}x{c[2]}_ref{c[7][0]}_tz{c[6]}" for c in CASES])
def test_emulated_wpp_p_rows_are_bit_exact(wpp_emu, pkg, case):
    _run_case(pkg, wpp_emu, *case)


@pytest.mark.parametrize("w,h,still,nref", [(256, 112, (0, 0, 128, 64), 2), (192, 48, None, 1)])
def test_emulated_wpp_p_rows_on_the_hand_off_fixtures(wpp_emu, pkg, w, h, still, nref):
    """the clips of tests/test_wpp_p_oracle.py whose decisions depend on the search state carried into the bottom row / into
    a picture"""
    frames = split_motion_clip(w, h, 3, 5 if still else 3, still=still)
    _run_case(pkg, wpp_emu, "split", w, h, 30, 3, 64, 1, (nref, "recent"), 0, 1 if still else 0, 0, frames=frames)


def test_emulated_wpp_p_rows_in_the_testing_state(wpp_emu, pkg):
    """the fork's Testing state with every switch on (Skip2Nx2N drops intra only, so the depth-0 searches still run)"""
    gen, w, h = "shear_mixed", 192, 112
    obf, _ = hmo_py.obf_prepass(st.moving_frame(pkg.synth, gen, w, h, 7, 1)[0])
    decision = (hmo_py.TESTING, obf, (1, 1, 1, 1), (1, 1, 1, 1), 1)
    _run_case(pkg, wpp_emu, gen, w, h, 32, 2, 16, 1, (1, "hm"), 0, 0, 0, decision=decision)


def test_read_before_write_count_fires(wpp_emu, pkg):
    """the count is live: a 48-high picture has no full CTU, so its TZ searches read start vectors they did not write, and a
    row 0 whose start state is declared unknown shows them"""
    gen, w, h, base_qp = "mixed", 128, 48, 30
    frames = [st.moving_frame(pkg.synth, gen, w, h, 7, poc) for poc in range(2)]
    res = wpp_p_clip(frames, base_qp, search_range=16)
    _, qp, lam = hmo_py.ldp_slice(1, base_qp)
    p = dict(lam=lam, sr=16, fast=1, amp=0, btab=0, refs=[res[0]["rec"]], ref_pocs=[0], poc=1, col_ref_pocs=[-1], col=None)
    assert emulate(wpp_emu, frames[1], qp, p=p, int_mv=[(0, 0)] * 4)["rbw"] == 0
    assert emulate(wpp_emu, frames[1], qp, p=p, int_mv=[(0, 0)] * 4, start_known=0)["rbw"] > 0
