"""Tiles on the MI355X, through the C ABI: fcu_tiles_begin / fcu_compress_chains (one chain per tile) and fcu_wpp_begin_tiles /
fcu_compress_wpp (WaveFrontSynchro inside every tile) against the reference of tests/tile_oracle.py -- every fcu_ctu_out field of
every CTU, the reconstruction, the coder state after every chain (the Q15 counter left out after the last CTU of every tile but
the last), for P pictures the search state after every chain -- on the cases tests/test_tiles_emu.py decides on the emulator;
the 1 x 1 grid against the one-slice paths; the deciders end to end; and the argument checks of the entry points.  Every GPU step
is one bounded launch; nothing provokes the give-up path."""
import numpy as np
import pytest

import search_trace as st
from tile_oracle import assert_picture_equal
from tiles_testlib import (I_QPS, I_TILES, P_CASES, WIDE_QP, WIDE_TILES, expected_chains, i_decision, i_frame, i_reference, p_inputs, p_reference,
                           wide_frame, wide_reference)
from wpp_testlib import CTU_DT, _poisoned

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -2, -4


def _decide(pkg, f, qp, tiles, wpp, ref, p=None, decision=None):
    """one picture through the tile chains of the engine, compared with `ref`; returns the engine's out bytes"""
    h, w = f[0].shape
    W, H = (w + 63) // 64, (h + 63) // 64
    n = tiles[0] * (H if wpp else tiles[1])
    eng = pkg.CuEngine(w, h, max_chains=n)
    try:
        assert eng.tile_chains(*tiles, wpp) == n
        rec, out = _poisoned(eng, f)
        kw = {}
        if p is not None:
            fp = pkg.engine.ldp_slice(30, 1)
            assert fp.qp == qp
            fp.lambda_, fp.search_range, fp.fast_search, fp.amp = p["lam"], p["sr"], p["fast"], p["amp"]
            kw = dict(params=fp, ref=eng.pad_reference(p["ref"]))
            if p.get("col") is not None:                     # TMVP (tile rows only): the reference picture's fcu_ctu_out array
                fp.tmvp = 1
                kw["col"] = eng.torch.as_tensor(np.frombuffer(p["col"], np.uint8).copy()).to(rec[0].device)
        got_n, _, _ = eng.init_tile_picture(0, f, qp, *tiles, wpp=wpp, rec=rec, out=out, **kw)
        assert got_n == n
        if decision is not None:
            obf = None if decision[1] is None else eng.torch.as_tensor(np.ascontiguousarray(decision[1], np.int16)).to(rec[0].device)
            for k in range(n):
                eng.set_decision(k, decision[0], obf, decision[2], decision[3], decision[4])      # rewrites the descriptor tail: the tile survives
        if wpp:
            eng.compress_wpp(0, n)
        else:
            eng.compress_chains(0, n, eng.n_ctu)
        eng.sync()
        states = [eng.ctx_state(k, full=True) for k in range(n)]
        mvs = [eng.search_state(k) for k in range(n)] if p is not None else None
        out_bytes = out.cpu().numpy().tobytes()
        skipped = assert_picture_equal(ref, out_bytes, [t.cpu().numpy() for t in rec], states, mvs, sorted_ctx=st.O_SORTED if p is not None else None)
        assert skipped == tiles[0] * tiles[1] - 1
        assert [eng.position(k) for k in range(n)] == [c[5] for c in expected_chains(W, H, tiles, wpp)]      # CTUs decided inside the tile
        eng.deblock(0)
        eng.sync()
        for a, b in zip(eng.rec_planes(0), ref.deblocked()):
            assert np.array_equal(a, b), "deblocked picture"
        return out_bytes
    finally:
        eng.destroy()


@pytest.mark.parametrize("wpp", [False, True], ids=["tile_chains", "wpp_in_tiles"])
@pytest.mark.parametrize("qp", I_QPS)
def test_tiles_of_an_i_picture_match_the_reference(pkg, qp, wpp):
    _decide(pkg, i_frame(pkg), qp, I_TILES, wpp, i_reference(pkg, qp, wpp))


@pytest.mark.parametrize("wpp", [False, True], ids=["tile_chains", "wpp_in_tiles"])
def test_tiles_in_the_testing_state_match_the_reference(pkg, wpp):
    f = i_frame(pkg)
    _decide(pkg, f, 37, I_TILES, wpp, i_reference(pkg, 37, wpp, True), decision=i_decision(f))


@pytest.mark.parametrize("wpp", [False, True], ids=["tile_chains", "wpp_in_tiles"])
def test_set_decision_after_binding_keeps_the_tiles_on_the_device(pkg, wpp):
    """fcu_chain_set_decision copies the descriptor tail -- the tile rectangle sits in it -- from the host descriptor to the
    device (ADVICE.md finding 4).  Training state on every chain after binding: nothing about the decisions changes, so the
    picture must still be the tiled reference, which it is only if every chain's rectangle on the device survived the copy."""
    _decide(pkg, i_frame(pkg), 27, I_TILES, wpp, i_reference(pkg, 27, wpp), decision=(pkg.engine.TRAINING, None, (0, 0, 0, 0), (0, 0, 0, 0), 0))


@pytest.mark.parametrize("wpp", [False, True], ids=["tile_chains", "wpp_in_tiles"])
def test_four_wide_tiles_match_the_reference(pkg, wpp):
    """512 x 128 as 2 x 1 tiles of 4 x 2 CTUs: with WaveFrontSynchro the second row of the tile at tile_x0 = 4 really waits, for
    min(x + 2, 4) CTUs of the row above counted inside the tile"""
    _decide(pkg, wide_frame(pkg), WIDE_QP, WIDE_TILES, wpp, wide_reference(pkg, wpp))


@pytest.mark.parametrize("wpp", [False, True], ids=["tile_chains", "wpp_in_tiles"])
@pytest.mark.parametrize("name", list(P_CASES))
def test_tiles_of_a_p_picture_match_the_reference(pkg, name, wpp):
    f, qp, p = p_inputs(pkg, name)
    _decide(pkg, f, qp, P_CASES[name][2], wpp, p_reference(pkg, name, wpp), p=p)


def test_a_1x1_grid_equals_the_one_slice_paths(pkg):
    f = i_frame(pkg)
    h, w = f[0].shape
    eng = pkg.CuEngine(w, h, max_chains=6)
    rec0, out0 = _poisoned(eng, f)
    eng.init_chain(0, f, 27, rec=rec0, out=out0)
    eng.compress_chains(0, 1, eng.n_ctu)
    rec1, out1 = _poisoned(eng, f)
    assert eng.init_tile_picture(1, f, 27, 1, 1, rec=rec1, out=out1)[0] == 1
    eng.compress_chains(1, 1, eng.n_ctu)
    eng.sync()
    dt = CTU_DT

    def same(a, b):
        x, y = np.frombuffer(a.cpu().numpy().tobytes(), dt), np.frombuffer(b.cpu().numpy().tobytes(), dt)
        return all(np.array_equal(x[n], y[n]) for n in dt.names)
    assert same(out0, out1) and all(np.array_equal(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(rec0, rec1))
    s0, s1 = eng.ctx_state(0, full=True), eng.ctx_state(1, full=True)
    assert np.array_equal(s0[0], s1[0]) and s0[1] == s1[1]
    rows = eng.lib.fcu_wpp_rows(eng.h)
    rec2, out2 = _poisoned(eng, f)
    eng.init_wpp_picture(0, f, 27, rec=rec2, out=out2)
    eng.compress_wpp(0, rows)
    st2 = [eng.ctx_state(k, full=True) for k in range(rows)]
    rec3, out3 = _poisoned(eng, f)
    assert eng.init_tile_picture(3, f, 27, 1, 1, wpp=True, rec=rec3, out=out3)[0] == rows
    eng.compress_wpp(3, rows)
    assert same(out2, out3) and all(np.array_equal(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(rec2, rec3))
    for k in range(rows):
        s = eng.ctx_state(3 + k, full=True)
        assert np.array_equal(s[0], st2[k][0]) and s[1] == st2[k][1]
    eng.destroy()


def test_deciders_with_tiles(pkg):
    f = i_frame(pkg)
    for wpp in (False, True):
        ref = i_reference(pkg, 27, wpp)
        dec = pkg.sequence.SequenceDecider(192, 136, 27, fast=False, in_flight=2, tiles=I_TILES, wpp=wpp)
        assert "2 x 2 uniform tiles" in dec.slice_mode
        for r in dec.decide_group([f, f]):
            got, want = np.frombuffer(r["out"].cpu().numpy().tobytes(), CTU_DT), np.frombuffer(ref.ctus, CTU_DT)
            assert all(np.array_equal(got[n], want[n]) for n in CTU_DT.names)
            for a, b in zip(r["rec"], ref.deblocked()):
                assert np.array_equal(a.cpu().numpy(), b)
        dec.close()
    name = "cols_tz"
    w, h, tiles, mode, sr, fast, amp, M = P_CASES[name]
    ld = pkg.lowdelay.LowDelayPDecider(w, h, 30, search_range=sr, tiles=tiles, wpp=True, fast_search=fast)
    frames = [st.moving_frame(pkg.synth, "mixed", w, h, 7, poc) for poc in range(2)]
    r0 = ld.decide_picture([frames[0]])[0]
    r1 = ld.decide_picture([frames[1]])[0]
    assert r0["slice_type"] == 0 and r1["slice_type"] == 1
    pm = np.frombuffer(r1["out"].cpu().numpy().tobytes(), CTU_DT)["pred_mode"]
    assert (pm == 0).sum() > 0                                 # the P picture found inter CUs through the tile chains
    ld.close()


def test_argument_and_state_checks(pkg):
    f = i_frame(pkg)
    eng = pkg.CuEngine(192, 136, max_chains=6)
    lib = eng.lib
    rec, out = _poisoned(eng, f)
    planes = [eng.torch.as_tensor(a).to(rec[0].device).contiguous() for a in f]
    ptrs = [p.data_ptr() for p in planes] + [p.data_ptr() for p in rec] + [out.data_ptr()]
    import ctypes as C
    fp = pkg.engine.FrameParams()
    lib.fcu_default_frame_params(C.byref(fp), 32)
    for begin in (lib.fcu_tiles_begin, lib.fcu_wpp_begin_tiles):
        assert begin(eng.h, 0, C.byref(fp), 4, 1, *ptrs) == ERR_ARG and begin(eng.h, 0, C.byref(fp), 1, 4, *ptrs) == ERR_ARG      # an empty tile
        assert begin(eng.h, 0, C.byref(fp), 0, 1, *ptrs) == ERR_ARG
        fp.slice_ctus = 3
        assert begin(eng.h, 0, C.byref(fp), 2, 2, *ptrs) == ERR_ARG           # tiles together with SliceMode 1
        fp.slice_ctus = 0
        fp.slice_type, fp.lambda_, fp.tmvp = 1, 30.0, 1
        assert begin(eng.h, 0, C.byref(fp), 2, 1, *ptrs) == ERR_ARG           # TMVP across tile columns
        assert begin(eng.h, 0, C.byref(fp), 1, 2, *ptrs) == 0                 # ... tile rows only: allowed
        fp.slice_type, fp.lambda_, fp.tmvp = 0, 0.0, 0
    assert lib.fcu_tiles_begin(eng.h, 3, C.byref(fp), 2, 2, *ptrs) == ERR_ARG         # 4 chains from 3: too few
    assert lib.fcu_wpp_begin_tiles(eng.h, 1, C.byref(fp), 2, 2, *ptrs) == ERR_ARG     # 6 chains from 1: too few
    assert lib.fcu_tile_chains(eng.h, 2, 2, 0) == 4 and lib.fcu_tile_chains(eng.h, 2, 2, 1) == 6 and lib.fcu_tile_chains(eng.h, 4, 1, 0) == -1
    assert lib.fcu_tiles_begin(eng.h, 0, C.byref(fp), 2, 2, *ptrs) == 0
    assert lib.fcu_chain_set_range(eng.h, 1, 0, 9) == ERR_STATE               # a tile chain keeps its tile
    assert lib.fcu_compress_wpp(eng.h, 0, 4, None) == ERR_STATE               # tile chains are advanced by fcu_compress_chains
    assert lib.fcu_wpp_begin_tiles(eng.h, 0, C.byref(fp), 2, 2, *ptrs) == 0
    assert lib.fcu_compress_chains(eng.h, 0, 6, 9, None) == ERR_STATE         # row chains are decided by fcu_compress_wpp
    assert lib.fcu_compress_wpp(eng.h, 0, 5, None) == ERR_STATE               # the range must end with the picture's last tile
    assert lib.fcu_compress_wpp(eng.h, 1, 5, None) == ERR_STATE               # ... and start with its first
    assert lib.fcu_compress_wpp(eng.h, 0, 6, None) == 0
    assert lib.fcu_compress_wpp(eng.h, 0, 6, None) == ERR_STATE               # already decided
    eng.destroy()
