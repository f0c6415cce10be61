"""WaveFrontSynchro for P pictures on the MI355X: LowDelayPDecider(wpp=True) -- the rows of every clip's picture in one
fcu_compress_wpp launch, the TZ search state handed from row to row and from picture to picture -- against the test-side
P-slice WPP reference (tests/wpp_oracle.py) with the oracle's loop filters: every fcu_ctu_out field, the reconstruction
before and after the loop filters, each row's coder state and the search state after every picture; plus the argument and
state checks of fcu_wpp_begin_p / fcu_compress_wpp."""
import ctypes as C

import numpy as np
import pytest

import hmo_py
import search_trace as st
from test_wpp_p_oracle import split_motion_clip
from wpp_oracle import WppOracle, wpp_p_clip
from wpp_testlib import CTU_DT, _compare_ctus

pytestmark = pytest.mark.gpu


def _check_picture(dec, r, R, what, rows=True):
    """one picture of LowDelayPDecider(wpp=True) (r) against one picture of wpp_p_clip (R)"""
    _compare_ctus(r["out"].cpu().numpy().tobytes(), R["ctus"], what)
    for p, q in zip(r["rec_unfiltered"], R["rec_unfiltered"]):
        assert np.array_equal(p.cpu().numpy(), q), f"{what}: reconstruction"
    for p, q in zip(r["rec"], R["rec"]):
        assert np.array_equal(p.cpu().numpy(), q), f"{what}: picture after the loop filters"
    assert r["search_state"] == R["int_mv"], f"{what}: search state after the picture"
    if rows and r["poc"] > 0:
        o = R["o"]
        for k in range(o.H):
            ctx, frac = dec.eng.ctx_state(r["first"] + k, full=True)
            assert np.array_equal(ctx[st.O_SORTED], o.row_state[k][0][st.O_SORTED]) and frac == o.row_state[k][1], f"{what}: row {k} coder state"
            assert dec.eng.search_state(r["first"] + k) == o.row_int_mv[k], f"{what}: row {k} search state"


def _clip(pkg, gen, w, h, base_qp, n_pic, sr, fast, nref_rps, tmvp, amp, btab, sao=False, seed=7, frames=None):
    nref, rps = nref_rps
    if frames is None:
        frames = [st.moving_frame(pkg.synth, gen, w, h, seed, poc) for poc in range(n_pic)]
    want = wpp_p_clip(frames, base_qp, ref_pocs=lambda poc, n: pkg.lowdelay.ref_pocs(poc, n, rps), n_refs=nref, search_range=sr,
                      fast_search=fast, tmvp=tmvp, amp=amp, cabac_b_table=btab, sao=sao)
    dec = pkg.lowdelay.LowDelayPDecider(w, h, base_qp, n_clips=1, search_range=sr, fast_search=fast, tmvp=bool(tmvp), amp=bool(amp),
                                        n_refs=nref, rps=rps, sao=sao, wpp=True)
    n_inter = 0
    for poc, f in enumerate(frames):
        r = dec.decide_picture([f], cabac_b_table=btab)[0]
        R = want[poc]
        _check_picture(dec, r, R, f"{gen} {w}x{h} poc{poc}")
        if sao:
            assert r["sao"] is not None and R["sao"] is not None              # the pictures after the loop filters above include SAO
        n_inter += int((np.frombuffer(R["ctus"], CTU_DT)["pred_mode"] == 0).sum())
    dec.close()
    assert n_inter > 0
    return want


# gen, w, h, base_qp, n_pic, search range, TZ, references (rps), TMVP, AMP, cabac_b_table -- the emulator test's mix
CASES = [
    ("shear_mixed", 256, 112, 30, 3, 16, 1, (2, "recent"), 1, 1, 0),
    ("mixed", 192, 176, 32, 4, 16, 1, (4, "hm"), 0, 0, 1),
    ("textured", 192, 128, 27, 3, 8, 0, (1, "hm"), 1, 0, 0),
    ("mixed", 192, 48, 30, 4, 16, 1, (1, "hm"), 1, 1, 0),
    ("shear_textured", 56, 136, 30, 3, 16, 1, (2, "recent"), 0, 1, 0),
]


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}_{c[1]}x{c[2]}_ref{c[7][0]}_tz{c[6]}" for c in CASES])
def test_lowdelay_wpp_clips_match_the_oracle(pkg, case):
    _clip(pkg, *case)


@pytest.mark.parametrize("w,h,still,nref", [(256, 112, (0, 0, 128, 64), 2), (192, 176, (0, 0, 128, 128), 2), (192, 48, None, 1)])
def test_lowdelay_wpp_hand_off_fixtures(pkg, w, h, still, nref):
    """the clips of tests/test_wpp_p_oracle.py whose decisions depend on the search state carried into the bottom row / into
    a picture"""
    frames = split_motion_clip(w, h, 3, 5 if still else 3, still=still)
    _clip(pkg, "split", w, h, 30, 3, 64, 1, (nref, "recent"), 0, 1 if still else 0, 0, frames=frames)


def test_lowdelay_wpp_clip_with_sao(pkg):
    """SAO 1: every picture's reference is the deblocked and SAO-filtered predecessor"""
    _clip(pkg, "mixed", 192, 112, 30, 4, 16, 1, (2, "hm"), 1, 0, 0, sao=True)


def test_1080p_pair_at_search_range_64(pkg):
    """BASELINE configs[4] at full size: an I + P pair of 1920x1080 at SearchRange 64 with TZ search (17 rows, the bottom one
    56 samples high: it waits for the whole row above and starts from its search state)"""
    _clip(pkg, "mixed", 1920, 1080, 32, 2, 64, 1, (1, "hm"), 0, 0, 0, seed=21)


def test_dependency_stress(pkg):
    """textured top rows, flat bottom rows, a partial bottom row: the bottom rows decide a CTU in a fraction of the time of the
    top ones and would overtake the rows above if a wait were missing"""
    w, h = 768, 624
    frames = []
    for poc in range(3):
        Y, U, V = [a.copy() for a in st.moving_frame(pkg.synth, "textured", w, h, 4, poc)]
        Y[192:] = 128
        U[96:] = 128
        V[96:] = 128
        frames.append((Y, U, V))
    _clip(pkg, "stress", w, h, 27, 3, 16, 1, (1, "hm"), 1, 0, 0, frames=frames)


def test_many_clips_in_one_launch(pkg):
    """256 clips of 128x1088 (2 x 17 CTUs): 4352 row chains per launch, more than the GPU keeps resident; every clip equals
    the same clip decided alone"""
    w, h, n_clips, seeds, n_pic = 128, 1088, 256, 4, 2
    clips = [[st.moving_frame(pkg.synth, "mixed", w, h, s, poc) for poc in range(n_pic)] for s in range(seeds)]
    alone = []
    for s in range(seeds):
        dec = pkg.lowdelay.LowDelayPDecider(w, h, 32, n_clips=1, search_range=16, fast_search=1, wpp=True)
        alone.append([(bytes(r["out"].cpu().numpy()), [p.cpu().numpy() for p in r["rec"]], r["search_state"])
                      for r in (dec.decide_picture([f])[0] for f in clips[s])])
        dec.close()
    dec = pkg.lowdelay.LowDelayPDecider(w, h, 32, n_clips=n_clips, search_range=16, fast_search=1, wpp=True)
    assert n_clips * 17 > 256 * max(1, dec.eng.lib.fcu_chains_per_cu())
    for poc in range(n_pic):
        res = dec.decide_picture([clips[i % seeds][poc] for i in range(n_clips)])
        for i, r in enumerate(res):
            out, rec, state = alone[i % seeds][poc]
            assert bytes(r["out"].cpu().numpy()) == out, f"clip {i} poc{poc}"
            assert all(np.array_equal(p.cpu().numpy(), q) for p, q in zip(r["rec"], rec)), f"clip {i} poc{poc}"
            assert r["search_state"] == state, f"clip {i} poc{poc}"
    dec.close()


def test_testing_state_set_before_the_search_state(pkg):
    """the fork's Testing state with every switch on, set on every row with set_decision BEFORE the row-0 search state
    (set_decision rewrites the descriptor tail, which holds the search state)"""
    eng_mod = pkg.engine
    w, h, base_qp, sr = 192, 112, 32, 16
    f0, f1 = [st.moving_frame(pkg.synth, "shear_mixed", w, h, 7, poc) for poc in range(2)]
    want = wpp_p_clip([f0], base_qp, search_range=sr)
    state_in = [(5, -3), (0, 2), (-7, 1), (2, 2)]
    obf_o, _ = hmo_py.obf_prepass(f1[0])
    sw = ((1, 1, 1, 1), (1, 1, 1, 1))
    _, qp, lam = hmo_py.ldp_slice(1, base_qp)
    o = WppOracle(*f1, qp, int_mv=state_in, decision=(hmo_py.TESTING, obf_o, sw[0], sw[1], 1), ref=want[0]["rec"], lambda_override=lam,
                  search_range=sr, fast_search=1).run()
    rows = (h + 63) // 64
    eng = pkg.CuEngine(w, h, max_chains=rows)
    fp = eng_mod.ldp_slice(base_qp, 1)
    fp.search_range, fp.fast_search = sr, 1
    pad = eng.pad_reference([eng.torch.as_tensor(p).cuda() for p in want[0]["rec"]])
    obf_dev = eng.obf_prepass(f1[0])[0][0].contiguous()
    _, rec, out = eng.init_wpp_picture(0, f1, fp.qp, params=fp, ref=pad)
    for r in range(rows):
        eng.set_decision(r, eng_mod.TESTING, obf_dev, *sw, depth_exception=1)
    eng.set_search_state(0, state_in)
    eng.compress_wpp(0, rows)
    _compare_ctus(out.cpu().numpy().tobytes(), o.enc.all_ctus_bytes(), "Testing state")
    for p, q in zip(rec, o.enc.rec):
        assert np.array_equal(p.cpu().numpy(), q), "Testing state: reconstruction"
    assert eng.search_state(rows - 1) == o.int_mv
    eng.destroy()


def test_argument_and_state_checks(pkg):
    eng_mod = pkg.engine
    w, h = 192, 128
    Y, U, V = pkg.synth.mixed(w, h, seed=2)
    eng = pkg.CuEngine(w, h, max_chains=5)
    lib = eng.lib
    torch = eng.torch
    planes = [torch.as_tensor(a).cuda() for a in (Y, U, V)]
    rec = [p.clone() for p in planes]
    out = torch.zeros(eng.n_ctu * eng_mod.CTU_OUT_BYTES, dtype=torch.uint8, device="cuda")
    ptrs = [p.data_ptr() for p in planes] + [p.data_ptr() for p in rec] + [out.data_ptr()]
    pad_a, pad_b = eng.pad_reference(planes), eng.pad_reference([torch.flip(p, [0]).contiguous() for p in planes])

    def begin_p(first, fp):
        return lib.fcu_wpp_begin_p(eng.h, first, C.byref(fp), *ptrs)

    fi = eng_mod.FrameParams()
    lib.fcu_default_frame_params(C.byref(fi), 32)
    assert begin_p(0, fi) == -2                              # an I slice
    fp = eng_mod.ldp_slice(32, 1)
    fp.tmvp = 0
    fp.slice_ctus = 3
    assert begin_p(0, fp) == -2                              # WPP with SliceMode 1
    fp.slice_ctus = 0
    assert begin_p(4, fp) == -2                              # too few chains left for two rows
    assert lib.fcu_wpp_begin(eng.h, 0, C.byref(fp), *ptrs) == -2     # fcu_wpp_begin keeps rejecting P

    assert begin_p(0, fp) == 0
    assert lib.fcu_compress_wpp(eng.h, 0, 2, None) == -4     # a P row without a reference picture
    assert lib.fcu_chain_set_reference(eng.h, 0, *[p.data_ptr() for p in pad_a]) == 0
    assert lib.fcu_compress_wpp(eng.h, 0, 2, None) == -4     # row 1 still without one
    assert lib.fcu_chain_set_reference(eng.h, 1, *[p.data_ptr() for p in pad_b]) == 0
    assert lib.fcu_compress_wpp(eng.h, 0, 2, None) == -4     # row 1 names another picture
    assert lib.fcu_chain_set_reference(eng.h, 1, *[p.data_ptr() for p in pad_a]) == 0
    ptr2 = (C.c_void_p * 6)(*[p.data_ptr() for p in pad_a + pad_b])
    pocs = (C.c_int * 2)(0, -1)
    assert lib.fcu_chain_set_references(eng.h, 1, 2, ptr2, pocs, 1) == 0
    assert lib.fcu_compress_wpp(eng.h, 0, 2, None) == -4     # row 1 has two references, row 0 one
    assert lib.fcu_chain_set_references(eng.h, 0, 2, ptr2, pocs, 1) == 0
    col = torch.zeros_like(out)
    assert lib.fcu_chain_set_collocated(eng.h, 0, col.data_ptr()) == 0
    assert lib.fcu_compress_wpp(eng.h, 0, 2, None) == -4     # a collocated field on row 0 only
    assert lib.fcu_chain_set_collocated(eng.h, 1, col.data_ptr()) == 0
    assert lib.fcu_compress_chains(eng.h, 0, 2, 3, None) == -4       # row chains belong to fcu_compress_wpp
    assert lib.fcu_compress_wpp(eng.h, 0, 2, None) == 0
    eng.destroy()
