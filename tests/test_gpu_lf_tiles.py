"""Loop filters of a picture with tiles on the MI355X, through the C ABI: fcu_deblock_tiles and fcu_sao_tiles against the tile
reference of tests/lf_tile_oracle.py for the grids x LFCrossTileBoundaryFlag x slice type that tests/test_lf_tiles.py runs on the
emulator; a 1 x 1 grid byte for byte against fcu_deblock / fcu_sao; a batch of two pictures with their own parameters; the argument
checks; and a lowdelay_P clip with tiles, SAO and the flag 0 whose every picture is tile reference -> deblock -> SAO reference.
Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import hmo_py
import lf_tile_oracle as L
import search_trace as st
import test_sao as T
from tile_oracle import tile_reference
from wpp_testlib import CTU_DT

pytestmark = pytest.mark.gpu
ERR_ARG = -2
CASES = [(g, c) for g in L.GRIDS for c in (0, 1)]
IDS = ["%dx%d_cross%d" % (g[0], g[1], c) for g, c in CASES]
dev = lambda planes: [torch.as_tensor(np.ascontiguousarray(p)).cuda() for p in planes]
ctus_dev = lambda b: torch.as_tensor(np.frombuffer(b, np.uint8).copy()).cuda()


@pytest.fixture(scope="module")
def eng(pkg):
    e = pkg.CuEngine(L.W, L.H, max_chains=4)
    yield e
    e.destroy()


def _assert_sao(pkg, coded, off, rec, r, tag=()):
    assert np.array_equal(T.M.canon(pkg.engine.sao_coded_to_array(coded)), T.M.canon(r["params"])), tag + ("signalled parameters",)
    for k, (p, q) in enumerate(zip(rec, r["rec"])):
        assert np.array_equal(p.cpu().numpy(), q), tag + ("filtered plane", k)
    assert list(off) == r["off"], tag + ("off_count",)


@pytest.mark.parametrize("tiles,cross", CASES, ids=IDS)
def test_deblock_and_sao_of_a_tile_picture_match_the_reference(pkg, eng, tiles, cross):
    """the picture is decided through the engine's tile chains, then deblocked and SAO-filtered on the device (I and P: the slice
    type SAO is told)"""
    ref = L.decided(pkg, tiles)
    n, rec, out = eng.init_tile_picture(0, L.frame(pkg), L.QP, *tiles)
    eng.compress_chains(0, n, eng.n_ctu)
    eng.sync()
    got, want = np.frombuffer(out.cpu().numpy().tobytes(), CTU_DT), np.frombuffer(ref.ctus, CTU_DT)
    assert all(np.array_equal(got[k], want[k]) for k in CTU_DT.names)
    ms = eng.deblock(0, tiles=tiles, lf_cross_tiles=cross, timed=True)
    assert len(ms) == 2
    want_dbk = L.deblocked(ref, tiles, cross)
    for k, (p, q) in enumerate(zip(rec, want_dbk)):
        assert np.array_equal(p.cpu().numpy(), q), ("deblocked plane", k)
    org = eng._keep[0][0]
    for slice_type in L.SLICE_TYPES:
        r = L.filtered(pkg, tiles, cross, slice_type)
        d_rec = dev(want_dbk)
        coded, off, ms4 = eng.sao([{"org": org, "rec": d_rec, "qp": L.QP, "lambda_": L.LAMBDA, "slice_type": slice_type}], tiles=tiles, lf_cross_tiles=cross, timed=True)
        assert len(ms4) == 4
        _assert_sao(pkg, coded[0], off[0], d_rec, r, (slice_type,))


def test_one_tile_is_byte_identical_to_the_calls_without_tiles(pkg, eng):
    ref = L.decided(pkg, (1, 1))
    out, org = ctus_dev(ref.ctus), dev(L.frame(pkg))
    for cross in (0, 1):
        a, b = dev(ref.rec), dev(ref.rec)
        eng.deblock(out=out, rec=a)
        eng.deblock(out=out, rec=b, tiles=(1, 1), lf_cross_tiles=cross)
        eng.sync()
        assert all(torch.equal(p, q) for p, q in zip(a, b))
        assert any(not np.array_equal(p.cpu().numpy(), q) for p, q in zip(a, ref.rec))
        pic = lambda rec: [{"org": org, "rec": rec, "qp": L.QP, "lambda_": L.LAMBDA, "slice_type": 1, "enabled": (1, 1, 1)}]
        c0, o0, _ = eng.sao(pic(a))
        c1, o1, _ = eng.sao(pic(b), tiles=(1, 1), lf_cross_tiles=cross)
        assert torch.equal(c0, c1) and np.array_equal(o0, o1) and all(torch.equal(p, q) for p, q in zip(a, b))


def test_a_batch_of_two_pictures_with_their_own_parameters(pkg, eng):
    """one fcu_sao_tiles call: QP 32 / I / all components next to QP 37 / P / Cb off, other content -- each as the reference alone"""
    tiles, cross = (2, 2), 0
    f1 = [np.ascontiguousarray(a) for a in pkg.synth.mixed(L.W, L.H, seed=5)]
    ref1 = tile_reference(f1, 37, tiles)
    lam1 = 0.6 * 2.0 ** ((37 - 12) / 3.0)
    dbk1 = L.deblocked(ref1, tiles, cross)
    rec1 = [p.copy() for p in dbk1]
    p1, off1, _ = L.sao_tiles(f1, rec1, 37, hmo_py.SLICE_P, lam1, tiles, cross, enabled=(1, 0, 1))
    r0 = L.filtered(pkg, tiles, cross, hmo_py.SLICE_I)
    d0, d1 = dev(r0["dbk"]), dev(dbk1)
    coded, off, _ = eng.sao([{"org": dev(L.frame(pkg)), "rec": d0, "qp": L.QP, "lambda_": L.LAMBDA, "slice_type": hmo_py.SLICE_I},
                             {"org": dev(f1), "rec": d1, "qp": 37, "lambda_": lam1, "slice_type": hmo_py.SLICE_P, "enabled": (1, 0, 1)}], tiles=tiles, lf_cross_tiles=cross)
    _assert_sao(pkg, coded[0], off[0], d0, r0, (0,))
    _assert_sao(pkg, coded[1], off[1], d1, dict(params=p1, off=off1, rec=rec1), (1,))


def test_argument_checks(pkg, eng):
    lib = eng.lib
    ref = L.decided(pkg, (1, 1))
    out, org, rec = ctus_dev(ref.ctus), dev(L.frame(pkg)), dev(ref.deblocked())
    before = [p.clone() for p in rec]
    dbk = lambda cols, rows, cross: lib.fcu_deblock_tiles(eng.h, out.data_ptr(), *[p.data_ptr() for p in rec], 0, 0, cols, rows, cross, None, None)
    prm = (pkg.engine.SaoParams * 1)()
    prm[0].slice_type, prm[0].qp, prm[0].slice_ctus = 0, L.QP, 0
    prm[0].lambda_[0] = L.LAMBDA
    for k in range(3):
        prm[0].enabled[k] = 1
    po, pr = (C.c_void_p * 3)(*[p.data_ptr() for p in org]), (C.c_void_p * 3)(*[p.data_ptr() for p in rec])
    coded = torch.zeros((eng.n_ctu, pkg.engine.SAO_CTU_BYTES), dtype=torch.uint8, device="cuda")
    sao = lambda cols, rows, cross: lib.fcu_sao_tiles(eng.h, 1, prm, cols, rows, cross, po, pr, coded.data_ptr(), None, None, None)
    for call in (dbk, sao):
        for cols, rows, cross in ((5, 1, 0), (1, 4, 1), (0, 1, 1), (1, 0, 0), (2, 2, 2), (2, 2, -1)):      # 4 x 3 CTUs: an empty tile; the flag
            assert call(cols, rows, cross) == ERR_ARG, (cols, rows, cross)
    prm[0].slice_ctus = 4
    assert sao(2, 2, 1) == ERR_ARG and b"slice" in lib.fcu_last_error()      # tiles together with SliceMode 1
    assert lib.fcu_sao(eng.h, 1, prm, po, pr, coded.data_ptr(), None, None, None) == 0      # ... which fcu_sao itself takes
    eng.sync()
    rec2 = dev(ref.deblocked())
    pr2 = (C.c_void_p * 3)(*[p.data_ptr() for p in rec2])
    prm[0].slice_ctus = 0
    assert lib.fcu_deblock_tiles(eng.h, None, *[p.data_ptr() for p in rec2], 0, 0, 2, 2, 0, None, None) == ERR_ARG
    assert lib.fcu_deblock_tiles(eng.h, out.data_ptr(), *[p.data_ptr() for p in rec2], 7, 0, 2, 2, 0, None, None) == ERR_ARG
    assert lib.fcu_sao_tiles(eng.h, 0, prm, 2, 2, 0, po, pr2, coded.data_ptr(), None, None, None) == ERR_ARG
    eng.sync()
    assert all(torch.equal(p, q) for p, q in zip(rec2, dev(ref.deblocked()))), "a refused call touched the planes"
    assert len(before) == 3


@pytest.mark.parametrize("wpp", [False, True], ids=["tile_chains", "wpp_in_tiles"])
def test_lowdelay_clip_with_tiles_sao_and_no_crossing(pkg, wpp):
    """LowDelayPDecider(256, 192, tiles=(2, 2), sao=True, lf_cross_tiles=0), four pictures: every picture's CTU records, SAO
    parameters and filtered planes == tile reference -> stitched deblocking -> SAO tile reference, the filtered picture being the
    next one's reference picture.  The P pictures go through the crop reference, which holds when the reference picture equals
    its edge replication wherever a tile's search can read across the tile edge; the clip does not move and the search range is
    small, and the reach of every decided picture is asserted below the plateau half-width."""
    from tile_oracle import grid, plateau_planes, reach_of
    w, h, base_qp, sr, n_pic, tiles, M = 256, 192, 30, 4, 4, (2, 2), 32
    cb, rb = grid(4, 3, *tiles)
    dec = pkg.lowdelay.LowDelayPDecider(w, h, base_qp, n_clips=1, search_range=sr, sao=True, tiles=tiles, lf_cross_tiles=0, wpp=wpp)
    state, prev = hmo_py.SaoState(), None
    base = plateau_planes(st.moving_frame(pkg.synth, "mixed", w, h, 9, 0), cb, rb, M)
    for poc in range(n_pic):
        noise = np.random.default_rng(100 + poc).integers(-3, 4, (h, w))
        f = [np.clip(base[0].astype(np.int16) + noise, 0, 255).astype(np.uint8), base[1].copy(), base[2].copy()]
        stype, qp, lam = hmo_py.ldp_slice(poc, base_qp)
        r = dec.decide_picture([f])[0]
        kw = dict(lambda_override=lam) if poc == 0 else dict(ref=prev, lambda_override=lam, search_range=sr, fast_search=1)
        ref = tile_reference(f, qp, tiles, wpp=wpp, **kw)
        got, want = np.frombuffer(r["out"].cpu().numpy().tobytes(), CTU_DT), np.frombuffer(ref.ctus, CTU_DT)
        for k in CTU_DT.names:
            assert np.array_equal(got[k], want[k]), (poc, k)
        if poc:
            assert reach_of(ref.ctus, sr)[0] <= M, poc
        dbk = L.deblocked(ref, tiles, 0)
        layer = hmo_py.ldp_layer(poc)
        en = state.enabled(layer)
        assert en == r["sao_enabled"], poc
        rec = [p.copy() for p in dbk]
        params, off, _ = L.sao_tiles(f, rec, qp, stype, lam, tiles, 0, enabled=en)
        state.update(layer, off, ref.W * ref.H)
        assert np.array_equal(T.M.canon(pkg.engine.sao_coded_to_array(r["sao"])), T.M.canon(params)), poc
        for a, b in zip(r["rec"], rec):
            assert np.array_equal(a.cpu().numpy(), b), poc
        prev = rec
    dec.close()
