"""The picture-level kernels past their loop and grid thresholds through the C ABI on the GPU: the cases of tests/big_cases.py (one
CTU row of 128, 129 and 130 CTUs, and 16 such pictures for the risk-table model) that tests/test_big_pictures.py runs on the
emulators, against the same numpy references, byte for byte.  Every output buffer is poisoned with 0xA5 before the first call, and
every entry point is called twice: these kernels promise identical bytes on a repeated call.  The tests live here and not in
test_gpu_report.py, test_gpu_maps.py, test_gpu_cu_trace.py and test_gpu_risk.py, whose helpers they use, so that those modules stay
as they are."""
import ctypes as C

import numpy as np
import pytest
import torch

import big_cases as BC
import cu_trace_ref as ref
import maps_cases as MC
import maps_ref
import report_ref
import risk_ref
from test_gpu_maps import lib_maps, stale, up
from test_gpu_report import picture
from test_gpu_risk import _dev

pytestmark = pytest.mark.gpu


def filled(nbytes):
    return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")


def twice(call, outputs):
    """runs `call` twice and returns the bytes of `outputs` (a function), which the second call must leave as they were"""
    call()
    first = outputs()
    call()
    assert outputs() == first
    return first


# ---- fcu_picture_report
def abi_report(pkg, eng, pics, reports, d_ctu):
    n = len(pics)
    org = (C.c_void_p * (3 * n))(*[t.data_ptr() for p in pics for t in p["org"]])
    rec = (C.c_void_p * (3 * n))(*[t.data_ptr() for p in pics for t in p["rec"]])
    out = (C.c_void_p * n)(*[p["out"].data_ptr() for p in pics])
    assert eng.lib.fcu_picture_report(eng.h, n, org, rec, out, reports.ctypes.data, d_ctu.data_ptr(), None, None) == 0, eng.lib.fcu_last_error()


@pytest.mark.parametrize("n_ctu,offset", [(128, 0), (129, 0), (129, 1), (130, 0)])
def test_big_report_at_and_past_one_trip_of_the_record_walk(n_ctu, offset, pkg):
    """report_pic walks 128 records per trip.  One picture and a batch of three of different content, on the wide loads (128 and
    129 CTUs, aligned planes), the byte-exact ones for planes one byte off, and for the width that is no multiple of 16 (130)"""
    e = pkg.engine
    cases = [BC.report_case(n_ctu, s) for s in (5, 8, 9)]
    eng = pkg.CuEngine(*BC.size(n_ctu), max_chains=1)
    try:
        assert eng.n_ctu == n_ctu
        pics = [picture(c, offset) for c in cases]
        for batch in (pics[:1], pics):
            n = len(batch)
            reports = np.frombuffer(b"\xa5" * (n * e.PIC_REPORT_DTYPE.itemsize), e.PIC_REPORT_DTYPE).copy()
            d_ctu = filled(n * n_ctu * e.CTU_REPORT_DTYPE.itemsize)
            twice(lambda: abi_report(pkg, eng, batch, reports, d_ctu), lambda: (reports.tobytes(), d_ctu.cpu().numpy().tobytes()))
            ctu = d_ctu.cpu().numpy().view(e.CTU_REPORT_DTYPE).reshape(n, n_ctu)
            for i in range(n):
                report_ref.assert_equal(e.pic_report_to_dict(reports[i]), ctu[i], cases[i][3], cases[i][4], (n_ctu, offset, i))
    finally:
        eng.destroy()


# ---- fcu_split_match, fcu_decision_maps
@pytest.mark.parametrize("n_ctu", sorted(BC.WIDTHS))
def test_big_split_match_at_and_past_one_trip_of_the_record_walk(n_ctu, pkg):
    """match_pic walks 128 records per trip.  A against B (a seeded third of the CTUs differs: the first, the last and the first of
    the second trip among them), A against itself and B against A in one call"""
    e = pkg.engine
    w, h = BC.size(n_ctu)
    a, b, want, third = BC.match_case(n_ctu, 21)
    eng = pkg.CuEngine(w, h, max_chains=1)
    try:
        da, db = up(a), up(b)
        pa, pb = (C.c_void_p * 3)(da.data_ptr(), da.data_ptr(), db.data_ptr()), (C.c_void_p * 3)(db.data_ptr(), da.data_ptr(), da.data_ptr())
        rec = np.frombuffer(b"\xa5" * (3 * e.PIC_MATCH_DTYPE.itemsize), e.PIC_MATCH_DTYPE).copy()
        d_ctu = filled(3 * n_ctu * e.CTU_MATCH_DTYPE.itemsize)

        def call():
            assert eng.lib.fcu_split_match(eng.h, 3, pa, pb, rec.ctypes.data, d_ctu.data_ptr(), None, None) == 0, eng.lib.fcu_last_error()
        twice(call, lambda: (rec.tobytes(), d_ctu.cpu().numpy().tobytes()))
        got = [e.pic_match_to_dict(rec[i]) for i in range(3)]
        maps_ref.assert_match_equal(got[0], want, n_ctu)
        maps_ref.assert_match_equal(got[1], maps_ref.split_match(pkg, a, a, w, h), (n_ctu, "self"))
        swapped = dict(want, node=want["node"].transpose(0, 2, 1), only_a=want["only_b"], only_b=want["only_a"])
        maps_ref.assert_match_equal(got[2], swapped, (n_ctu, "swapped"))
        ctu = d_ctu.cpu().numpy().view(e.CTU_MATCH_DTYPE).reshape(3, n_ctu)
        for k in maps_ref.MATCH_KEYS:                          # the per-CTU records add up to the picture's
            assert np.array_equal(ctu[0][k].astype(np.int64).sum(axis=0), np.asarray(got[0][k]).astype(np.int64)), k
        same = ctu[0]["part_equal"] == ctu[0]["part_total"]
        assert not ctu["pad"].any() and same[[i for i in range(n_ctu) if i not in third]].all() and not same[third].all()
    finally:
        eng.destroy()


def test_big_decision_maps_of_130_ctus(pkg):
    w, h = BC.size(BC.MANY)
    r, obf, want = BC.maps_case()
    NL = sum(p * q for p, q in maps_ref.level_shapes(w, h))
    eng = pkg.CuEngine(w, h, max_chains=1)
    try:
        d_r, d_obf = up(r), up(obf)
        bufs = {"bytes": stale(len(MC.ALL_FIELDS) * (h // 4) * (w // 4), fill=0xA5), "mv": stale((h // 4) * (w // 4) * 4, fill=0xA5),
                "labels": stale(NL, fill=0xA5), "n_obf": stale(NL * 2, fill=0xA5)}
        got = []
        twice(lambda: got.append(lib_maps(eng, w, h, [d_r], MC.ALL_FIELDS, True, True, [d_obf], bufs=bufs)[0]),
              lambda: {k: v.cpu().numpy().tobytes() for k, v in bufs.items()})
        maps_ref.assert_maps_equal(got[0][0], MC.select(want, MC.ALL_FIELDS), "strip")
    finally:
        eng.destroy()


# ---- fcu_label_score, fcu_trace_maps
def test_big_label_score_and_trace_maps_of_130_ctus(pkg):
    """two pictures against two label arrays: the per-CTU and per-picture score records byte for byte the reference's -- score_pic
    adds 130 records in raster order, which the case tells from the reversed order -- and the label / J0 / J1 maps"""
    w, h = BC.size(BC.MANY)
    traces, labels, want_ctu, want_pic, want_maps = BC.score_case()
    eng = pkg.CuEngine(w, h, max_chains=1)
    try:
        NL = eng.label_count()
        tr, lb = [_dev(torch, t) for t in traces], [_dev(torch, q) for q in labels]
        tp, lp = (C.c_void_p * 2)(*[t.data_ptr() for t in tr]), (C.c_void_p * 2)(*[t.data_ptr() for t in lb])
        rec = np.frombuffer(b"\xa5" * (2 * 224), ref.PIC_SCORE).copy()
        d_ctu = filled(2 * BC.MANY * 128)

        def score():
            assert eng.lib.fcu_label_score(eng.h, 2, tp, lp, rec.ctypes.data, d_ctu.data_ptr(), None, None) == 0, eng.lib.fcu_last_error()
        twice(score, lambda: (rec.tobytes(), d_ctu.cpu().numpy().tobytes()))
        ctu = d_ctu.cpu().numpy().view(ref.CTU_SCORE).reshape(2, BC.MANY)
        for i in range(2):
            assert ctu[i].tobytes() == want_ctu[i].tobytes(), i
            assert rec[i]["v"][:, 4:].tobytes() == want_pic[i]["v"][:, 4:].tobytes(), (i, rec[i]["v"][:, 4:], want_pic[i]["v"][:, 4:])
            assert rec[i].tobytes() == want_pic[i].tobytes(), i
            assert (BC.reversed_sums(ctu[i])[3] != rec[i]["v"][3, 4:]).any()
        out = [filled(2 * NL * k) for k in (1, 8, 8)]

        def maps():
            assert eng.lib.fcu_trace_maps(eng.h, 2, tp, *[t.data_ptr() for t in out], None, None) == 0, eng.lib.fcu_last_error()
        twice(maps, lambda: [t.cpu().numpy().tobytes() for t in out])
        for i in range(2):
            for k, (got, want) in enumerate(zip(out, want_maps[i])):
                assert got.cpu().numpy().reshape(2, -1)[i].tobytes() == want.tobytes(), (i, k)
    finally:
        eng.destroy()


# ---- the risk-table model
def test_big_training_where_the_cap_on_the_slots_binds(pkg):
    """16 pictures = 2080 units on 128 workgroups: waves of two and of three units, risk_add over every slot.  In one context, so
    that the slot buffer holds what other batches left: 3 pictures, then all 16 into a model poisoned with 0xA5; 3 + 13 accumulated
    in two calls; all 16 again over the slots of the 13; and 3 accumulated on top of the 16"""
    w, h = BC.size(BC.MANY)
    traces, keys, model, dropped, _, _ = BC.risk_case()
    k = BC.RISK_SPLIT
    eng = pkg.CuEngine(w, h, max_chains=1)
    try:
        tr, ky = [_dev(torch, t) for t in traces], [_dev(torch, q, torch.uint16) for q in keys]
        part, d1 = eng.risk_train(tr[:k], ky[:k])
        assert part.cpu().numpy().tobytes() == risk_ref.train(traces[:k], keys[:k], w, h)[0].tobytes()
        m = filled(24672)
        got, d = eng.risk_train(tr, ky, model=m)
        assert got.cpu().numpy().tobytes() == model.tobytes() and d == dropped
        _, d2 = eng.risk_train(tr[k:], ky[k:], model=part, accumulate=True)
        assert part.cpu().numpy().tobytes() == model.tobytes() and d1 + d2 == dropped
        again, d3 = eng.risk_train(tr, ky, model=m)
        assert again.cpu().numpy().tobytes() == model.tobytes() and d3 == dropped
        want, d4 = risk_ref.train(traces[:k], keys[:k], w, h, model=model)
        _, d5 = eng.risk_train(tr[:k], ky[:k], model=m, accumulate=True)
        assert m.cpu().numpy().tobytes() == want.tobytes() and d5 == d4 == d1
    finally:
        eng.destroy()


def test_big_predict_and_nobf_maps_of_130_ctus(pkg):
    """the level plans of risk_predict / nobf_blocks with five workgroups at level 3: labels of four pictures for min_count 1 and 3
    and the N_OBF maps of two"""
    w, h = BC.size(BC.MANY)
    _, keys, model, _, labels, _ = BC.risk_case()
    pick = (0, 1, 2, BC.RISK_PICS - 1)
    eng = pkg.CuEngine(w, h, max_chains=1)
    try:
        NL = eng.label_count()
        ky = [_dev(torch, keys[j], torch.uint16) for j in pick]
        kp = (C.c_void_p * 4)(*[t.data_ptr() for t in ky])
        m = torch.as_tensor(np.frombuffer(model.tobytes(), np.uint8).copy()).cuda()
        for min_count in (1, 3):
            out = filled(4 * NL)

            def predict():
                assert eng.lib.fcu_risk_predict(eng.h, 4, kp, m.data_ptr(), min_count, out.data_ptr(), None, None) == 0, eng.lib.fcu_last_error()
            assert twice(predict, lambda: out.cpu().numpy().tobytes()) == b"".join(labels[min_count][j].tobytes() for j in pick), min_count
        cases = [BC.maps_case(s) for s in (11, 12)]
        obf = [torch.as_tensor(np.array(c[1])).cuda() for c in cases]
        op = (C.c_void_p * 2)(*[t.data_ptr() for t in obf])
        nobf = filled(2 * NL * 2)

        def call():
            assert eng.lib.fcu_nobf_maps(eng.h, 2, op, nobf.data_ptr(), None) == 0, eng.lib.fcu_last_error()
        want = b"".join(np.concatenate([q.reshape(-1) for q in c[2]["n_obf"]]).astype(np.uint16).tobytes() for c in cases)
        assert twice(call, lambda: nobf.cpu().numpy().tobytes()) == want
    finally:
        eng.destroy()
