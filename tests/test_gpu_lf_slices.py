"""Loop filters of a picture of slices on the MI355X, through the C ABI: fcu_deblock_slices and fcu_sao_slices against the slice
reference of tests/lf_slice_oracle.py for the slice lengths x LFCrossSliceBoundaryFlag x slice type that tests/test_lf_slices.py
runs on the emulator; the flag 1, or one slice, byte for byte against fcu_deblock / fcu_sao; a P picture; slice independence on
the device; a batch of two pictures with their own slices; the argument checks; and a lowdelay_P clip with slices, SAO and the
flag 0 whose every picture is oracle decision -> reference deblocking -> reference SAO.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import hmo_py
import lf_slice_oracle as L
import search_trace as st
import test_sao as T
from wpp_testlib import CTU_DT

pytestmark = pytest.mark.gpu
ERR_ARG = -2
ALL = L.CUTS + L.ONE
CASES = [(s, c) for s in ALL for c in (0, 1)]
IDS = ["slice%d_cross%d" % (s, c) for s, c in CASES]
dev = lambda planes: [torch.as_tensor(np.ascontiguousarray(p)).cuda() for p in planes]
host = lambda planes: [p.cpu().numpy() for p in planes]
ctus_dev = lambda b: torch.as_tensor(np.frombuffer(b, np.uint8).copy()).cuda()
same = lambda a, b: all(np.array_equal(p, q) for p, q in zip(a, b))


@pytest.fixture(scope="module")
def eng(pkg):
    e = pkg.CuEngine(L.W, L.H, max_chains=12)
    yield e
    e.destroy()


def _assert_sao(pkg, coded, off, rec, r, tag=()):
    assert np.array_equal(T.M.canon(pkg.engine.sao_coded_to_array(coded)), T.M.canon(r["params"])), tag + ("signalled parameters",)
    for k, (p, q) in enumerate(zip(rec, r["rec"])):
        assert np.array_equal(p.cpu().numpy(), q), tag + ("filtered plane", k)
    assert list(off) == r["off"], tag + ("off_count",)


def _pic(org, rec, slice_type, slice_ctus, **kw):
    return dict({"org": org, "rec": rec, "qp": L.QP, "lambda_": L.LAMBDA, "slice_type": slice_type, "slice_ctus": slice_ctus}, **kw)


@pytest.mark.parametrize("slice_ctus,cross", CASES, ids=IDS)
def test_deblock_and_sao_of_a_slice_picture_match_the_reference(pkg, eng, slice_ctus, cross):
    """the oracle's decision of the sliced I picture, deblocked and SAO-filtered on the device (I and P: the slice type SAO is told)"""
    d = L.decided(pkg, slice_ctus)
    out, org, rec = ctus_dev(d.ctus), dev(d.frame), dev(d.rec)
    ms = eng.deblock(out=out, rec=rec, slice_ctus=slice_ctus, lf_cross_slices=cross, timed=True)
    assert len(ms) == 2
    want_dbk = L.filtered(pkg, slice_ctus, cross, hmo_py.SLICE_I)["dbk"]
    for k, (p, q) in enumerate(zip(rec, want_dbk)):
        assert np.array_equal(p.cpu().numpy(), q), ("deblocked plane", k)
    lib = eng.lib
    for slice_type in L.SLICE_TYPES:
        r = L.filtered(pkg, slice_ctus, cross, slice_type)
        d_rec = dev(want_dbk)
        if cross == 0:
            coded, off, ms4 = eng.sao([_pic(org, d_rec, slice_type, slice_ctus)], lf_cross_slices=0, timed=True)
            assert len(ms4) == 4
            coded, off = coded[0], off[0]
        else:                                                       # CuEngine.sao hands the flag 1 to fcu_sao: the entry point itself
            prm = (pkg.engine.SaoParams * 1)()
            prm[0].slice_type, prm[0].qp, prm[0].slice_ctus, prm[0].lambda_[0] = slice_type, L.QP, slice_ctus, L.LAMBDA
            for k in range(3):
                prm[0].enabled[k] = 1
            po, pr = (C.c_void_p * 3)(*[p.data_ptr() for p in org]), (C.c_void_p * 3)(*[p.data_ptr() for p in d_rec])
            coded, off = torch.zeros((eng.n_ctu, pkg.engine.SAO_CTU_BYTES), dtype=torch.uint8, device="cuda"), np.zeros(3, np.int32)
            assert lib.fcu_sao_slices(eng.h, 1, prm, 1, po, pr, coded.data_ptr(), off.ctypes.data, None, None) == 0
        _assert_sao(pkg, coded, off, d_rec, r, (slice_type,))


@pytest.mark.parametrize("slice_ctus,cross", [(s, 1) for s in ALL] + [(s, 0) for s in L.ONE], ids=lambda v: str(v))
def test_crossing_or_one_slice_is_byte_identical_to_the_plain_calls(pkg, eng, slice_ctus, cross):
    d = L.decided(pkg, slice_ctus)
    out, org = ctus_dev(d.ctus), dev(d.frame)
    a, b = dev(d.rec), dev(d.rec)
    eng.deblock(out=out, rec=a)
    eng.deblock(out=out, rec=b, slice_ctus=slice_ctus, lf_cross_slices=cross)
    eng.sync()
    assert all(torch.equal(p, q) for p, q in zip(a, b)) and not same(host(a), d.rec)
    prm = (pkg.engine.SaoParams * 1)()
    prm[0].slice_type, prm[0].qp, prm[0].slice_ctus, prm[0].lambda_[0] = 1, L.QP, slice_ctus, L.LAMBDA
    for k in range(3):
        prm[0].enabled[k] = 1
    po = (C.c_void_p * 3)(*[p.data_ptr() for p in org])
    res = []
    for rec, call in ((a, lambda *x: eng.lib.fcu_sao(eng.h, 1, prm, *x)), (b, lambda *x: eng.lib.fcu_sao_slices(eng.h, 1, prm, cross, *x))):
        pr = (C.c_void_p * 3)(*[p.data_ptr() for p in rec])
        coded, off = torch.zeros((eng.n_ctu, pkg.engine.SAO_CTU_BYTES), dtype=torch.uint8, device="cuda"), np.zeros(3, np.int32)
        assert call(po, pr, coded.data_ptr(), off.ctypes.data, None, None) == 0
        res.append((coded, off))
    assert torch.equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("cross", (0, 1))
@pytest.mark.parametrize("slice_ctus", L.P_CUTS)
def test_deblocking_of_a_p_picture_matches_the_reference(pkg, eng, slice_ctus, cross):
    d = L.decided_p(pkg, slice_ctus)
    rec = dev(d.rec)
    eng.deblock(out=ctus_dev(d.ctus), rec=rec, slice_ctus=slice_ctus, lf_cross_slices=cross)
    eng.sync()
    assert same(host(rec), L.deblock_slices(d.ctus, L.W, L.H, d.rec, slice_ctus, cross))


@pytest.mark.parametrize("slice_ctus", L.CUTS)
def test_slices_are_independent_without_crossing(pkg, eng, slice_ctus):
    """samples outside slice s replaced by seeded random bytes: the deblocked samples inside the slice stay what the reference
    gives for the clean picture (statistics and the offset pass with fixed parameters: on the emulator, tests/test_lf_slices.py)"""
    d, r = L.decided(pkg, slice_ctus), L.filtered(pkg, slice_ctus, 0, hmo_py.SLICE_I)
    out = ctus_dev(d.ctus)
    for s in range(len(L.slice_ranges(L.W, L.H, slice_ctus))):
        m = [L.slice_map(L.W, L.H, slice_ctus, comp) == s for comp in range(3)]
        rec = dev(L.randomised_outside(d.rec, L.W, L.H, slice_ctus, s, 1000 + s))
        eng.deblock(out=out, rec=rec, slice_ctus=slice_ctus, lf_cross_slices=0)
        eng.sync()
        for comp, (p, q) in enumerate(zip(host(rec), r["dbk"])):
            assert np.array_equal(p[m[comp]], q[m[comp]]), ("deblocking", s, comp)


def test_a_batch_of_two_pictures_with_their_own_slices(pkg, eng):
    """one fcu_sao_slices call: slices of 5 / I / all components next to slices of 3 / P / Cb off -- each as the reference alone"""
    r0, r1 = L.filtered(pkg, 5, 0, hmo_py.SLICE_I), L.filtered(pkg, 3, 0, hmo_py.SLICE_P, (1, 0, 1))
    org, d0, d1 = dev(L.frame(pkg)), dev(r0["dbk"]), dev(r1["dbk"])
    coded, off, _ = eng.sao([_pic(org, d0, hmo_py.SLICE_I, 5), _pic(org, d1, hmo_py.SLICE_P, 3, enabled=(1, 0, 1))], lf_cross_slices=0)
    _assert_sao(pkg, coded[0], off[0], d0, r0, (0,))
    _assert_sao(pkg, coded[1], off[1], d1, r1, (1,))


def test_argument_checks(pkg, eng):
    lib = eng.lib
    d = L.decided(pkg, 5)
    clean = L.filtered(pkg, 5, 0, hmo_py.SLICE_I)["dbk"]
    out, org, rec = ctus_dev(d.ctus), dev(d.frame), dev(clean)
    dbk = lambda s, c, o=out, beta=0: lib.fcu_deblock_slices(eng.h, o.data_ptr() if o is not None else None, *[p.data_ptr() for p in rec], beta, 0, s, c, None, None)
    prm = (pkg.engine.SaoParams * 1)()
    prm[0].slice_type, prm[0].qp, prm[0].slice_ctus, prm[0].lambda_[0] = 0, L.QP, 5, L.LAMBDA
    for k in range(3):
        prm[0].enabled[k] = 1
    po, pr = (C.c_void_p * 3)(*[p.data_ptr() for p in org]), (C.c_void_p * 3)(*[p.data_ptr() for p in rec])
    coded = torch.zeros((eng.n_ctu, pkg.engine.SAO_CTU_BYTES), dtype=torch.uint8, device="cuda")
    sao = lambda c, n=1: lib.fcu_sao_slices(eng.h, n, prm, c, po, pr, coded.data_ptr(), None, None, None)
    for c in (2, -1):
        assert dbk(5, c) == ERR_ARG and b"lf_cross_slices" in lib.fcu_last_error()
        assert sao(c) == ERR_ARG and b"lf_cross_slices" in lib.fcu_last_error()
    assert dbk(-1, 0) == ERR_ARG and b"slice_ctus" in lib.fcu_last_error()
    assert dbk(-1, 1) == ERR_ARG and b"slice_ctus" in lib.fcu_last_error()
    prm[0].slice_ctus = -1
    assert sao(0) == ERR_ARG and b"slice_ctus" in lib.fcu_last_error()
    prm[0].slice_ctus = 5
    assert dbk(5, 0, None) == ERR_ARG and dbk(5, 0, out, 7) == ERR_ARG and sao(0, 0) == ERR_ARG      # what the plain calls refuse
    prm[0].qp = 52
    assert sao(0) == ERR_ARG
    eng.sync()
    assert same(host(rec), clean), "a refused call touched the planes"
    with pytest.raises(ValueError, match="tiles need one slice"):
        eng.deblock(out=out, rec=rec, tiles=(2, 2), slice_ctus=5, lf_cross_slices=0)
    # slices far beyond the picture, and slices on a layout: one slice / the layout's slice length
    lo = pkg.layout.PictureLayout(L.W, L.H, slice_ctus=5, lf_cross_slices=0)
    a, b = dev(d.rec), dev(d.rec)
    eng.deblock(out=out, rec=a, layout=lo)
    eng.deblock(out=out, rec=b, slice_ctus=1 << 30, lf_cross_slices=0)
    eng.sync()
    assert same(host(a), clean) and same(host(b), L.deblock_slices(d.ctus, L.W, L.H, d.rec, 0, 1))


@pytest.mark.parametrize("kw", [dict(slice_ctus=5), dict(wpp=True, slice_rows=1)], ids=["staircase_chains", "wpp_row_slices"])
def test_lowdelay_clip_with_slices_sao_and_no_crossing(pkg, kw):
    """LowDelayPDecider(256, 192, slice_ctus=5 | wpp + slice_rows=1, sao=True, lf_cross_slices=0), four pictures: every picture's
    CTU records, SAO parameters and filtered planes == oracle decision -> reference deblocking -> reference SAO, the filtered
    picture being the next one's reference picture."""
    w, h, base_qp, sr, n_pic = 256, 192, 30, 8, 4
    dec = pkg.lowdelay.LowDelayPDecider(w, h, base_qp, n_clips=1, search_range=sr, sao=True, lf_cross_slices=0, **kw)
    sl = dec.sao_slice_ctus
    assert sl == (5 if "slice_ctus" in kw else 4) and dec.lf_cross_slices == 0
    state, prev = hmo_py.SaoState(), None
    for poc in range(n_pic):
        f = st.moving_frame(pkg.synth, "mixed", w, h, 9, poc)
        stype, qp, lam = hmo_py.ldp_slice(poc, base_qp)
        r = dec.decide_picture([f])[0]
        # (the slices are decided side by side: every slice starts the TZ search state from zero, search_state_per_slice)
        okw = dict(lambda_override=lam) if poc == 0 else dict(ref=prev, lambda_override=lam, search_range=sr, fast_search=1, search_state_per_slice=1)
        o = hmo_py.Encoder(*f, qp, slice_ctus=sl, **okw)
        o.compress_frame()
        ctus, rec0 = o.all_ctus_bytes(), [p.copy() for p in o.rec]
        o.close()
        got, want = np.frombuffer(r["out"].cpu().numpy().tobytes(), CTU_DT), np.frombuffer(ctus, CTU_DT)
        for k in CTU_DT.names:
            assert np.array_equal(got[k], want[k]), (poc, k)
        rec = L.deblock_slices(ctus, w, h, rec0, sl, 0)
        layer = hmo_py.ldp_layer(poc)
        en = state.enabled(layer)
        assert en == r["sao_enabled"], poc
        params, off, _, _ = L.sao_slices([np.ascontiguousarray(p) for p in f], rec, qp, stype, lam, sl, 0, enabled=en)
        state.update(layer, off, 12)
        assert np.array_equal(T.M.canon(pkg.engine.sao_coded_to_array(r["sao"])), T.M.canon(params)), poc
        for a, b in zip(r["rec"], rec):
            assert np.array_equal(a.cpu().numpy(), b), poc
        prev = rec
    dec.close()
