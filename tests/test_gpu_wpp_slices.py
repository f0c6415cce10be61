"""WaveFrontSynchro on pictures cut into slices of whole CTU rows, on the MI355X: fcu_wpp_begin_slices / fcu_compress_wpp -- the
first row of every slice waits for nothing, the other rows for the row above in their slice -- against the test-side reference
(tests/wpp_oracle.py): every fcu_ctu_out field, the reconstruction, the rows' coder states, for P pictures the search
state after every row; SequenceDecider and LowDelayPDecider end to end with the loop filters; and the argument and state checks
of the entry point and of the launch.  Every GPU step is one bounded launch; nothing provokes the give-up path."""
import ctypes as C

import numpy as np
import pytest

import hmo_py
import search_trace as st
from wpp_oracle import WppOracle, wpp_oracle, wpp_p_clip
from wpp_testlib import CTU_DT, _compare, _compare_ctus, _poisoned

pytestmark = pytest.mark.gpu


# gen, w, h, qp, slice_rows: a subset of tests/test_wpp_slices_emu.py's I cases
@pytest.mark.parametrize("gen,w,h,qp,R", [("mixed", 256, 192, 22, 2), ("mixed", 320, 256, 22, 2), ("mixed", 320, 256, 22, 1), ("smooth", 136, 200, 37, 2),
                                          ("smooth", 136, 200, 37, 3), ("textured", 64, 192, 37, 2)])
def test_small_i_pictures_match_the_reference(pkg, gen, w, h, qp, R):
    Y, U, V = getattr(pkg.synth, gen)(w, h, seed=9)
    o = wpp_oracle(Y, U, V, qp, R)
    eng = pkg.CuEngine(w, h, max_chains=o.H)
    rec, out = _poisoned(eng, (Y, U, V))
    n, _, _ = eng.init_wpp_picture(0, (Y, U, V), qp, rec=rec, out=out, slice_rows=R)
    assert n == o.H
    eng.compress_wpp(0, n)
    _compare(o, rec, out, f"{gen} {w}x{h} qp{qp} R{R}", eng, 0)
    eng.destroy()


def test_one_slice_of_all_rows_equals_fcu_wpp_begin(pkg):
    w, h, qp = 256, 192, 22
    Y, U, V = pkg.synth.mixed(w, h, seed=9)
    o = wpp_oracle(Y, U, V, qp)
    eng = pkg.CuEngine(w, h, max_chains=3)
    for R in (3, 7):
        rec, out = _poisoned(eng, (Y, U, V))
        eng.init_wpp_picture(0, (Y, U, V), qp, rec=rec, out=out, slice_rows=R)
        eng.compress_wpp(0, 3)
        _compare(o, rec, out, f"R{R}", eng, 0)
    eng.destroy()


def test_decision_states_match_the_reference(pkg):
    eng_mod = pkg.engine
    w, h, qp, R = 384, 256, 32, 2
    Y, U, V = pkg.synth.mixed(w, h, seed=5)
    obf_o, _ = hmo_py.obf_prepass(Y)
    rows = (h + 63) // 64
    eng = pkg.CuEngine(w, h, max_chains=rows)
    obf_dev = eng.obf_prepass(Y)[0][0].contiguous()

    def check(state, sw):
        o = wpp_oracle(Y, U, V, qp, R, decision=(state, obf_o, sw[0], sw[1], 0))
        rec, out = _poisoned(eng, (Y, U, V))
        eng.init_wpp_picture(0, (Y, U, V), qp, rec=rec, out=out, slice_rows=R)
        for r in range(rows):
            eng.set_decision(r, state, obf_dev, *sw)         # rewrites the descriptor tail from the host copy: the row's binding survives
        eng.compress_wpp(0, rows)
        _compare(o, rec, out, f"state {state}", eng, 0)
        return o

    o = check(eng_mod.VERIFYING, ((0, 0, 0, 0), (0, 0, 0, 0)))
    ver = eng.verify_counts(0, rows)
    assert np.array_equal(ver, o.verify) and ver[:, :4].sum() > 0
    check(eng_mod.TESTING, ((1, 1, 0, 1), (1, 0, 1, 1)))
    eng.destroy()


def test_several_sliced_pictures_in_one_launch_beyond_residency(pkg):
    """256 pictures of 128x1088 (2 x 17 CTUs) with R = 2: 4352 row chains in one launch, more than the GPU keeps resident; a
    row that waits always waits on a lower chain index, so ticket order still guarantees progress"""
    w, h, n_pics, seeds, R = 128, 1088, 256, 4, 2
    srcs = [pkg.synth.mixed(w, h, seed=s) for s in range(seeds)]
    refs = [wpp_oracle(*s, 32, R) for s in srcs]
    rows = (h + 63) // 64
    eng = pkg.CuEngine(w, h, max_chains=n_pics * rows)
    assert n_pics * rows > 256 * max(1, eng.lib.fcu_chains_per_cu())
    pics = []
    for i in range(n_pics):
        rec, out = _poisoned(eng, srcs[i % seeds])
        eng.init_wpp_picture(i * rows, srcs[i % seeds], 32, rec=rec, out=out, slice_rows=R)
        pics.append((rec, out))
    assert eng.lib.fcu_compress_wpp(eng.h, 0, n_pics * rows, None) == 0, eng.lib.fcu_last_error().decode()
    for i, (rec, out) in enumerate(pics):
        _compare(refs[i % seeds], rec, out, f"picture {i}")
    eng.destroy()


def test_4k_rows_with_two_row_slices(pkg):
    """3840x2160 with R = 2 (the bench's slicing): the whole picture is decided in one launch; the reference's cost is bounded the
    way tests/test_gpu_parity.py bounds it for its 4K rows -- the first six CTU rows (three slices, 360 CTUs) are compared"""
    w, h, qp, R, rows = 3840, 2160, 32, 2, 6
    Y, U, V = pkg.synth.textured(w, h, seed=8)
    eng = pkg.CuEngine(w, h, max_chains=34)
    rec, out = _poisoned(eng, (Y, U, V))
    n, _, _ = eng.init_wpp_picture(0, (Y, U, V), qp, rec=rec, out=out, slice_rows=R)
    assert n == 34
    eng.compress_wpp(0, n)
    o = WppOracle(Y, U, V, qp, R, rows=rows).run()
    nb = C.sizeof(hmo_py.Ctu)
    _compare_ctus(out.cpu().numpy().tobytes()[:rows * 60 * nb], o.enc.all_ctus_bytes()[:rows * 60 * nb], "4K R2")
    for p, q in zip([t.cpu().numpy() for t in rec], o.enc.rec):
        k = rows * 64 >> (0 if p.shape[1] == w else 1)
        assert np.array_equal(p[:k], q[:k])
    for r in range(rows):
        ctx, frac = eng.ctx_state(r, full=True)
        assert np.array_equal(ctx, o.row_state[r][0]) and frac == o.row_state[r][1], r
    assert all(eng.position(r) == (r + 1) * 60 for r in range(34))
    eng.destroy()


def test_sequence_decider_with_sliced_wpp(pkg):
    w, h, qp, R = 256, 192, 32, 2
    srcs = [pkg.synth.mixed(w, h, seed=s) for s in (1, 2, 3)]
    dec = pkg.sequence.SequenceDecider(w, h, qp, fast=False, in_flight=3, wpp=True, slice_rows=R)
    assert "SliceArgument 8" in dec.slice_mode and "WaveFrontSynchro" in dec.slice_mode
    res = dec.decide_group(srcs)
    for (Y, U, V), r in zip(srcs, res):
        o = wpp_oracle(Y, U, V, qp, R)
        o.enc.deblock()                                      # LFCrossSliceBoundaryFlag 1: across the slice boundaries
        _compare(o, r["rec"], r["out"], f"POC {r['poc']} deblocked")
    dec.close()


# gen, w, h, base_qp, n_pic, search range, TZ, references (rps), TMVP, AMP, cabac_b_table, slice_rows, SAO
P_CASES = [
    ("shear_mixed", 192, 240, 30, 3, 16, 1, (2, "recent"), 1, 1, 0, 2, True),
    ("shear_mixed", 192, 240, 30, 2, 16, 1, (1, "hm"), 0, 0, 0, 3, False),
    ("mixed", 192, 176, 32, 4, 16, 1, (4, "hm"), 0, 0, 1, 2, False),
    ("textured", 192, 128, 27, 3, 8, 0, (1, "hm"), 1, 0, 0, 1, True),
]


@pytest.mark.parametrize("case", P_CASES, ids=[f"{c[0]}_{c[1]}x{c[2]}_ref{c[7][0]}_tz{c[6]}_R{c[11]}" for c in P_CASES])
def test_lowdelay_clips_with_sliced_wpp_match_the_reference(pkg, case):
    """LowDelayPDecider(wpp=True, slice_rows=R): several pictures, deblocked (and SAO told the slice length where on)"""
    gen, w, h, base_qp, n_pic, sr, fast, (nref, rps), tmvp, amp, btab, R, sao = case
    frames = [st.moving_frame(pkg.synth, gen, w, h, 7, poc) for poc in range(n_pic)]
    want = wpp_p_clip(frames, base_qp, R, ref_pocs=lambda poc, n: pkg.lowdelay.ref_pocs(poc, n, rps), n_refs=nref, search_range=sr,
                      fast_search=fast, tmvp=tmvp, amp=amp, cabac_b_table=btab, sao=sao)
    dec = pkg.lowdelay.LowDelayPDecider(w, h, base_qp, n_clips=1, search_range=sr, fast_search=fast, tmvp=bool(tmvp), amp=bool(amp),
                                        n_refs=nref, rps=rps, sao=sao, wpp=True, slice_rows=R)
    n_inter = 0
    for poc, f in enumerate(frames):
        r = dec.decide_picture([f], cabac_b_table=btab)[0]
        W_, what = want[poc], f"{gen} {w}x{h} R{R} poc{poc}"
        o = W_["o"]
        _compare_ctus(r["out"].cpu().numpy().tobytes(), W_["ctus"], what)
        for p, q in zip(r["rec_unfiltered"], W_["rec_unfiltered"]):
            assert np.array_equal(p.cpu().numpy(), q), f"{what}: reconstruction"
        for p, q in zip(r["rec"], W_["rec"]):
            assert np.array_equal(p.cpu().numpy(), q), f"{what}: picture after the loop filters"
        for k in range(o.H):
            ctx, frac = dec.eng.ctx_state(r["first"] + k, full=True)
            assert np.array_equal(ctx[st.O_SORTED], o.row_state[k][0][st.O_SORTED]) and frac == o.row_state[k][1], f"{what}: row {k} coder state"
            if poc > 0:
                assert dec.eng.search_state(r["first"] + k) == o.row_int_mv[k], f"{what}: row {k} search state"
        if poc > 0:
            assert r["search_state"] == o.slice_int_mv[-1], f"{what}: search state after the last slice"
        n_inter += int((np.frombuffer(W_["ctus"], CTU_DT)["pred_mode"] == 0).sum())
    dec.close()
    assert n_inter > 0


def test_argument_and_state_checks(pkg):
    eng_mod = pkg.engine
    w, h = 192, 192                                          # W = 3, H = 3
    Y, U, V = pkg.synth.mixed(w, h, seed=2)
    eng = pkg.CuEngine(w, h, max_chains=7)
    lib, torch = eng.lib, eng.torch
    assert lib.fcu_wpp_rows(eng.h) == 3
    planes = [torch.as_tensor(a).cuda() for a in (Y, U, V)]
    rec = [p.clone() for p in planes]
    out = torch.zeros(eng.n_ctu * eng_mod.CTU_OUT_BYTES, dtype=torch.uint8, device="cuda")
    ptrs = [p.data_ptr() for p in planes] + [p.data_ptr() for p in rec] + [out.data_ptr()]

    rec2, out2 = [p.clone() for p in planes], torch.zeros_like(out)
    ptrs2 = ptrs[:3] + [p.data_ptr() for p in rec2] + [out2.data_ptr()]

    def begin(first, fp, slice_rows, ptrs=ptrs):
        return lib.fcu_wpp_begin_slices(eng.h, first, C.byref(fp), slice_rows, *ptrs)

    fp = eng_mod.FrameParams()
    lib.fcu_default_frame_params(C.byref(fp), 32)
    for fp.slice_ctus in (4, 3, 7):
        assert begin(0, fp, 2) == -2, fp.slice_ctus          # a slice that starts mid-row / a length that is not slice_rows x W
    fp.slice_ctus = 0
    assert begin(0, fp, 0) == -2 and begin(0, fp, -1) == -2  # slice_rows below one
    assert begin(5, fp, 2) == -2 and begin(-1, fp, 2) == -2  # too few chains left for three rows
    fp.slice_ctus = 6
    assert lib.fcu_wpp_begin(eng.h, 0, C.byref(fp), *ptrs) == -2     # the one-slice entry points keep rejecting slice_ctus
    assert begin(0, fp, 2) == 0                              # slice_ctus exactly slice_rows x W
    fp.slice_ctus = 0
    assert begin(0, fp, 2) == 0 and begin(3, fp, 1, ptrs2) == 0      # two pictures: chains 0..2 (slices {0,1},{2}) and 3..5 (every row a slice)

    # state checks of the launch
    assert lib.fcu_compress_chains(eng.h, 0, 3, 3, None) == -4       # row chains belong to fcu_compress_wpp
    assert lib.fcu_chain_set_range(eng.h, 2, 6, 3) == -4
    assert lib.fcu_compress_wpp(eng.h, 0, 2, None) == -4     # a partial picture: ends before the last row
    assert lib.fcu_compress_wpp(eng.h, 2, 1, None) == -4     # ... starts at the first row of a later slice, not of the picture
    assert lib.fcu_compress_wpp(eng.h, 1, 2, None) == -4
    assert lib.fcu_compress_wpp(eng.h, 4, 2, None) == -4     # (R = 1: every row starts a slice, still not a picture start)
    eng.init_chain(6, (Y, U, V), 32)
    assert lib.fcu_compress_wpp(eng.h, 3, 4, None) == -4     # a plain chain in the range
    assert lib.fcu_compress_wpp(eng.h, 0, 6, None) == 0      # both pictures
    assert lib.fcu_compress_wpp(eng.h, 0, 3, None) == -4     # already decided
    _compare_ctus(out.cpu().numpy().tobytes(), wpp_oracle(Y, U, V, 32, 2).enc.all_ctus_bytes(), "R2 of two pictures")
    _compare_ctus(out2.cpu().numpy().tobytes(), wpp_oracle(Y, U, V, 32, 1).enc.all_ctus_bytes(), "R1 of two pictures")

    # a P row without a reference picture
    fpp = eng_mod.ldp_slice(32, 1)
    fpp.tmvp = 0
    assert begin(0, fpp, 2) == 0
    pad = eng.pad_reference(planes)
    for r in (0, 1):
        assert lib.fcu_chain_set_reference(eng.h, r, *[p.data_ptr() for p in pad]) == 0
    assert lib.fcu_compress_wpp(eng.h, 0, 3, None) == -4     # row 2 (a slice of its own) still without one
    assert lib.fcu_chain_set_reference(eng.h, 2, *[p.data_ptr() for p in pad]) == 0
    assert lib.fcu_compress_wpp(eng.h, 0, 3, None) == 0
    eng.destroy()
