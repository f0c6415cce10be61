"""WaveFrontSynchro on pictures cut into slices of whole CTU rows (fcu_wpp_begin_slices): the engine source's row chains on the
CPU wave emulator (tests/emu/wpp_emu.cpp, bound with the rules libfcu.so's binder uses) against the reference of
tests/wpp_oracle.py -- every fcu_ctu_out field, the reconstruction, the coder state after every row, the Verifying
counters, and for P pictures the search state after every row (so after every slice's last row) with the emulator's
read-before-write count of the TZ start vectors at zero.

Inputs on which the composition is not vacuous, i.e. the sliced-WPP decisions differ from the slices-only AND from the WPP-only
decisions of the oracle (found on the CPU with the reference; test_sliced_wpp_differs_from_*): I picture mixed 320x256 QP 22
with R = 2; P picture shear_mixed 192x240 base QP 30 (picture 1) with R = 2."""
import ctypes as C
import functools

import numpy as np
import pytest

import hmo_py
import search_trace as st
from wpp_oracle import WppOracle, wpp_oracle, wpp_p_clip
from wpp_testlib import I_PICTURE, TOOLS, assert_ctus_equal, emulate, flags_of, p_picture_args, wpp_emu  # noqa: F401 (wpp_emu: the fixture)

# gen, w, h, qp, tools, state, slice_rows                   (contents and QPs of tests/test_wpp_emu.py's cases)
I_CASES = [
    ("mixed", 256, 192, 22, -1, None, 2),                   # W = 4, H = 3: the last slice is a single row
    ("mixed", 320, 256, 22, -1, None, 2),                   # W = 5, H = 4
    ("mixed", 320, 256, 22, -1, None, 1),                   # every row is a slice: nothing may wait
    ("smooth", 136, 200, 37, -1, None, 2),                  # H = 4, partial bottom row: the second row of its slice
    ("smooth", 136, 200, 37, -1, None, 3),                  # ... and the row that starts its slice
    ("textured", 64, 192, 37, -1, None, 2),                 # W = 1: no context load
    ("textured", 200, 136, 22, TOOLS, None, 2),
    ("mixed", 256, 192, 32, -1, "testing", 2),
    ("mixed", 200, 136, 37, -1, "verifying", 2),
]


def _i_decision(Y, state):
    if state is None:
        return None
    obf, _ = hmo_py.obf_prepass(Y)
    return (hmo_py.TESTING if state == "testing" else hmo_py.VERIFYING, obf, (1, 1, 0, 1), (1, 0, 1, 1), 0)


def _check_i(lib, frame, qp, tools, state, R, o):
    e = emulate(lib, frame, qp, R, tools=tools, decision=_i_decision(frame[0], state))
    assert_ctus_equal(o.enc, e["out"])
    for p, q in zip(o.enc.rec, e["rec"]):
        assert np.array_equal(p, q)
    for r in range(o.H):
        assert np.array_equal(e["states"][r][0], o.row_state[r][0]) and e["states"][r][1] == o.row_state[r][1], r
    return e


@pytest.mark.parametrize("gen,w,h,qp,tools,state,R", I_CASES)
def test_emulated_sliced_wpp_rows_of_an_i_picture_are_bit_exact(wpp_emu, pkg, gen, w, h, qp, tools, state, R):
    frame = getattr(pkg.synth, gen)(w, h, seed=9)
    o = wpp_oracle(*frame, qp, R, decision=_i_decision(frame[0], state), **flags_of(tools))
    e = _check_i(wpp_emu, frame, qp, tools, state, R, o)
    if state == "verifying":
        assert np.array_equal(e["verify"], o.verify)
        assert e["verify"][:, :4].sum() > 0


@pytest.mark.parametrize("R", [3, 5])
def test_one_slice_of_all_rows_equals_one_slice_wpp(wpp_emu, pkg, R):
    """slice_rows >= H: bit for bit what fcu_wpp_begin decides (tests/wpp_oracle.py), and the new reference agrees"""
    frame = pkg.synth.mixed(256, 192, seed=9)
    o1 = wpp_oracle(*frame, 22)
    o = wpp_oracle(*frame, 22, R)
    assert o.enc.p.slice_ctus == R * 4 and o1.enc.p.slice_ctus == 0             # two runs of the reference, bound differently
    assert o.enc.all_ctus_bytes() == o1.enc.all_ctus_bytes()
    for r in range(o.H):
        assert np.array_equal(o.row_state[r][0], o1.row_state[r][0]) and o.row_state[r][1] == o1.row_state[r][1]
    e, e1 = emulate(wpp_emu, frame, 22, R), emulate(wpp_emu, frame, 22, 0)     # ... and two of the emulator
    assert e["above"] == [-1, 0, 1] and e1["above"] == [-1, 0, 1]
    for got in (e, e1):
        assert_ctus_equal(o1.enc, got["out"])
        for p, q in zip(o1.enc.rec, got["rec"]):
            assert np.array_equal(p, q)
        for r in range(o1.H):
            assert np.array_equal(got["states"][r][0], o1.row_state[r][0]) and got["states"][r][1] == o1.row_state[r][1]


def test_sliced_wpp_differs_from_slices_alone_and_from_wpp_alone_on_an_i_picture(pkg):
    """the composition is not vacuous: mixed 320x256, QP 22, R = 2"""
    frame = pkg.synth.mixed(320, 256, seed=9)
    both = wpp_oracle(*frame, 22, 2).enc.all_ctus_bytes()
    slices = hmo_py.Encoder(*frame, 22, slice_ctus=10)
    slices.compress_frame()
    assert both != slices.all_ctus_bytes()
    assert both != wpp_oracle(*frame, 22).enc.all_ctus_bytes()


# gen, w, h, base_qp, n_pic, search range, TZ, references (rps), TMVP, AMP, cabac_b_table, slice_rows
P_CASES = [
    ("shear_mixed", 192, 240, 30, 3, 16, 1, (2, "recent"), 1, 1, 0, 2),   # H = 4, partial bottom row (48 high) second in its slice; two references, AMP + TMVP
    ("shear_mixed", 192, 240, 30, 2, 16, 1, (1, "hm"), 0, 0, 0, 3),       # ... the partial row starts its slice
    ("mixed", 192, 176, 32, 4, 16, 1, (4, "hm"), 0, 0, 1, 2),             # the cfg's reference sets, B tables; the partial row (48) is a slice of its own
    ("textured", 192, 128, 27, 3, 8, 0, (1, "hm"), 1, 0, 0, 1),           # full search, every row a slice
    ("shear_textured", 56, 136, 30, 3, 16, 1, (2, "recent"), 0, 1, 0, 2),  # 56 wide: every row begins on a boundary CTU, W = 1
]


@functools.lru_cache(maxsize=None)
def _p_reference(pkg, gen, w, h, base_qp, n_pic, sr, fast, nref_rps, tmvp, amp, btab, R):
    nref, rps = nref_rps
    frames = [st.moving_frame(pkg.synth, gen, w, h, 7, poc) for poc in range(n_pic)]
    return frames, wpp_p_clip(frames, base_qp, R, ref_pocs=lambda poc, n: pkg.lowdelay.ref_pocs(poc, n, rps), n_refs=nref, search_range=sr,
                                     fast_search=fast, tmvp=tmvp, amp=amp, cabac_b_table=btab)


@pytest.mark.parametrize("case", P_CASES, ids=[f"{c[0]}_{c[1]}x{c[2]}_ref{c[7][0]}_tz{c[6]}_R{c[11]}" for c in P_CASES])
def test_emulated_sliced_wpp_rows_of_p_pictures_are_bit_exact(wpp_emu, pkg, case):
    gen, w, h, base_qp, n_pic, sr, fast, (nref, rps), tmvp, amp, btab, R = case
    frames, res = _p_reference(pkg, *case)
    n_inter = 0
    for poc in range(1, n_pic):
        o = res[poc]["o"]
        qp, p = p_picture_args(res, poc, base_qp, nref, sr, fast, tmvp, amp, btab)
        e = emulate(wpp_emu, frames[poc], qp, R, p=p)
        assert e["rbw"] == 0, (poc, "a TZ search read a start vector the row had neither written nor inherited")
        n_inter += assert_ctus_equal(o.enc, e["out"], (poc,))
        for a, b in zip(res[poc]["rec_unfiltered"], e["rec"]):
            assert np.array_equal(a, b), (poc, "reconstruction")
        for r in range(o.H):
            assert np.array_equal(e["states"][r][0][st.O_SORTED], o.row_state[r][0][st.O_SORTED]) and e["states"][r][1] == o.row_state[r][1], (poc, r, "coder state")
            assert e["mvs"][r] == o.row_int_mv[r], (poc, r, "search state after the row")
        last_rows = [min(s * R + R, o.H) - 1 for s in range((o.H + R - 1) // R)]
        assert [e["mvs"][r] for r in last_rows] == o.slice_int_mv, (poc, "search state after every slice")
    assert n_inter > 0


def test_sliced_wpp_differs_from_slices_alone_and_from_wpp_alone_on_a_p_picture(pkg):
    """the composition is not vacuous: picture 1 of P_CASES[0]'s clip (shear_mixed 192x240, base QP 30, TZ), R = 2, decided
    from the same reference picture by the three references"""
    case = P_CASES[0]
    gen, w, h, base_qp, n_pic, sr, fast, (nref, rps), tmvp, amp, btab, R = case
    frames, res = _p_reference(pkg, *case)
    _, qp, lam = hmo_py.ldp_slice(1, base_qp)
    kw = dict(ref=res[0]["rec"], col=res[0]["ctus"], lambda_override=lam, search_range=sr, fast_search=fast, amp=amp)
    both = res[1]["ctus"]
    slices = hmo_py.Encoder(*frames[1], qp, slice_ctus=R * 3, search_state_per_slice=1, **kw)
    slices.compress_frame()
    assert both != slices.all_ctus_bytes()
    assert both != WppOracle(*frames[1], qp, **kw).run().enc.all_ctus_bytes()


def test_binder_refuses_slices_that_start_mid_row_and_slice_rows_below_one(wpp_emu, pkg):
    """the rule fcu_wpp_begin_slices answers FCU_ERR_ARG by (fcu_host.h: wpp_slice_ctus), through the emulator's binder"""
    frame = [np.ascontiguousarray(a) for a in pkg.synth.mixed(256, 192, seed=9)]        # W = 4
    rec = [np.zeros_like(a) for a in frame]
    out = (hmo_py.Ctu * 12)()

    def create(slice_rows, fp_slice_ctus):
        hd = wpp_emu.wpp_emu_create(256, 192, 32, slice_rows, fp_slice_ctus, -1, *[a.ctypes.data for a in frame], *[a.ctypes.data for a in rec],
                                    C.addressof(out), *I_PICTURE, None, 1)
        if hd:
            sl = wpp_emu.wpp_emu_slice_ctus(hd)
            wpp_emu.wpp_emu_destroy(hd)
            return sl
        return None

    assert create(2, 0) == 8 and create(2, 8) == 8 and create(1, 4) == 4 and create(7, 0) == 28
    for slice_rows, fp_slice_ctus in [(2, 6), (2, 4), (2, 9), (1, 3), (0, 0), (0, 4), (-1, 0)]:
        assert wpp_emu.wpp_emu_slice_rule(4, slice_rows, fp_slice_ctus) == -1, (slice_rows, fp_slice_ctus)
        if (slice_rows, fp_slice_ctus) != (0, 0):             # (the driver's slice_rows 0 with slice_ctus 0 is the one-slice binding of fcu_wpp_begin)
            assert create(slice_rows, fp_slice_ctus) is None, (slice_rows, fp_slice_ctus)
    assert create(0, 0) == 0


def test_drivers_refuse_slice_rows_without_wpp(pkg):
    for make in (lambda **kw: pkg.sequence.SequenceDecider(256, 192, 32, **kw), lambda **kw: pkg.lowdelay.LowDelayPDecider(256, 192, 32, **kw)):
        with pytest.raises(ValueError, match="slice_rows"):
            make(slice_rows=2)
        with pytest.raises(ValueError, match="slice_rows"):
            make(slice_rows=2, slice_ctus=8)
        with pytest.raises(ValueError, match="slice_rows"):
            make(wpp=True, slice_rows=0)
        with pytest.raises(ValueError):                           # unchanged: wpp with slice_ctus
            make(wpp=True, slice_ctus=8)
