"""The risk-table model through the C ABI on the GPU: the synthetic cases of tests/risk_cases.py against the numpy reference
(tests/risk_ref.py), byte for byte, and SequenceDecider(risk=True) against the reference applied to its own Training traces."""
import ctypes as C

import numpy as np
import pytest

import maps_cases
import risk_cases
import risk_ref

pytestmark = pytest.mark.gpu


def _dev(torch, a, dtype=None):
    t = torch.as_tensor(np.array(a).view(np.uint8).reshape(-1)).cuda()                 # (a writable copy: the cases are read-only)
    return t if dtype is None else t.view(dtype)


@pytest.mark.parametrize("size", risk_cases.SIZES, ids=lambda s: "%dx%d" % s)
def test_cases_through_the_abi(pkg, size):
    """model bytes and `dropped` for one picture and a batch of three (over stale bytes), the accumulate identity, the repeat
    identity, the labels for min_count 0 / 1 / 3, fcu_risk_table on the model copied back, fcu_nobf_maps on the cases of maps_cases"""
    import torch
    w, h = size
    eng = pkg.CuEngine(w, h, max_chains=1)
    try:
        NL = eng.label_count()
        for n_pics in (1, 3):
            traces, keys, model, dropped, _ = risk_cases.case(w, h, n_pics)
            tr, ky = [_dev(torch, t) for t in traces], [_dev(torch, k, torch.uint16) for k in keys]
            m = torch.full((24672,), 0x5C, dtype=torch.uint8, device="cuda")
            got, d = eng.risk_train(tr, ky, model=m)
            assert got.cpu().numpy().tobytes() == model.tobytes() and d == dropped, n_pics
            again, d2 = eng.risk_train(tr, ky)
            assert again.cpu().numpy().tobytes() == model.tobytes() and d2 == dropped
        a, d1 = eng.risk_train(tr[:1], ky[:1])
        _, d2 = eng.risk_train(tr[1:], ky[1:], model=a, accumulate=True)
        assert a.cpu().numpy().tobytes() == model.tobytes() and d1 + d2 == dropped
        _, _, model, _, labels = risk_cases.case(w, h, 3)
        for min_count in risk_cases.MIN_COUNTS:
            lab = eng.risk_predict(ky, got, min_count=min_count).cpu().numpy()
            assert lab.tobytes() == np.stack(labels[min_count]).tobytes(), min_count
            assert pkg.engine.risk_table(got.cpu().numpy(), min_count).tobytes() == risk_ref.table(model, min_count).tobytes()
        obf = [torch.as_tensor(np.array(maps_cases.case(w, h, s)[1])).cuda() for s in (3, 4)]
        nobf = eng.nobf_maps(obf).cpu().numpy()
        for i, s in enumerate((3, 4)):
            assert nobf[i].tobytes() == np.concatenate([q.reshape(-1) for q in maps_cases.case(w, h, s)[2]["n_obf"]]).astype(np.uint16).tobytes(), i
        assert nobf.shape == (2, NL)
    finally:
        eng.destroy()


def test_guards_through_the_abi(pkg):
    import torch
    eng = pkg.CuEngine(64, 64, max_chains=1)
    try:
        traces, keys, _, _, _ = risk_cases.case(64, 64, 1)
        tr, ky = _dev(torch, traces[0]), _dev(torch, keys[0], torch.uint16)
        m = torch.zeros(24672 + 8, dtype=torch.uint8, device="cuda")
        lab = torch.zeros(eng.label_count(), dtype=torch.int8, device="cuda")
        one, k1, none = (C.c_void_p * 1)(tr.data_ptr()), (C.c_void_p * 1)(ky.data_ptr()), (C.c_void_p * 1)(None)
        L, h, mp = eng.lib, eng.h, m.data_ptr()
        for args, word in (((0, one, k1, mp, 0), b"n_pics"), ((1, None, k1, mp, 0), b"dev_trace is null"), ((1, one, None, mp, 0), b"dev_keys is null"), ((1, none, k1, mp, 0), b"dev_trace[0]"),
                           ((1, one, none, mp, 0), b"dev_keys[0]"), ((1, one, k1, None, 0), b"dev_model is null"), ((1, one, k1, mp + 4, 0), b"multiple of 8")):
            assert L.fcu_risk_train(h, *args, None, None, None) == -2 and word in L.fcu_last_error(), word
        many = (1 << 22) // eng.label_count() + 1
        big = (C.c_void_p * many)(*([tr.data_ptr()] * many))
        assert L.fcu_risk_train(h, many, big, big, mp, 0, None, None, None) == -2 and b"2^22" in L.fcu_last_error()
        for args, word in (((0, k1, mp, 1, lab.data_ptr()), b"n_pics"), ((1, None, mp, 1, lab.data_ptr()), b"dev_keys is null"), ((1, none, mp, 1, lab.data_ptr()), b"dev_keys[0]"),
                           ((1, k1, None, 1, lab.data_ptr()), b"dev_model is null"), ((1, k1, mp + 4, 1, lab.data_ptr()), b"multiple of 8"), ((1, k1, mp, -1, lab.data_ptr()), b"min_count"),
                           ((1, k1, mp, 1, None), b"dev_labels is null")):
            assert L.fcu_risk_predict(h, *args, None, None) == -2 and word in L.fcu_last_error(), word
        for args, word in (((0, k1, ky.data_ptr()), b"n_pics"), ((1, None, ky.data_ptr()), b"dev_obf is null"), ((1, none, ky.data_ptr()), b"dev_obf[0]"), ((1, k1, None), b"dev_nobf is null")):
            assert L.fcu_nobf_maps(h, *args, None) == -2 and word in L.fcu_last_error(), word
        for kw in (dict(risk=True, fast=False), dict(risk=True, labels=lambda *a: None), dict(risk={"min_count": -1}), dict(risk={"bins": 3}), dict(risk={"key": 5})):
            with pytest.raises(ValueError, match="risk"):
                pkg.sequence.SequenceDecider(64, 64, 32, **kw)
    finally:
        eng.destroy()


def test_sequence_decider_runs_the_schedule_on_the_model(pkg):
    """128x64, four pictures, period 4 = 2 Training + 1 Verifying + 1 Testing.  The Verifying and Testing pictures' `labels` equal
    risk_ref applied to the two Training traces copied to the host (keys: the pictures' own N_OBF maps); their decisions equal
    those of a second decider that is given the same arrays through labels=callable"""
    import torch
    w, h, qp = 128, 64, 32
    frames = [pkg.synth.mixed(w, h, seed=s) for s in (9, 10, 11, 12)]

    def run(**kw):
        sched = pkg.sequence.FastDecisionSchedule(period=4, n_training=2, n_verifying=1)
        dec = pkg.sequence.SequenceDecider(w, h, qp, fast=True, schedule=sched, **kw)
        try:
            res = [dec.decide(f) for f in frames]
            host = [dict(r, out=r["out"].cpu().numpy().copy(), labels=r["labels"].cpu().numpy().copy() if "labels" in r else None,
                         trace=dec.eng.cu_trace_array(r["cu_trace"]).copy() if "cu_trace" in r else None) for r in res]
            model = dec.risk_model.cpu().numpy().copy() if kw.get("risk") else None
            keys = [dec.eng.nobf_maps(dec.eng.obf_prepass(torch.as_tensor(f[0]).cuda())[0]).cpu().numpy()[0] for f in frames]
            return host, model, keys
        finally:
            dec.close()
    a, model, keys = run(risk=True)
    assert [r["state"] for r in a] == [pkg.sequence.TRAINING] * 2 + [pkg.sequence.VERIFYING, pkg.sequence.TESTING]
    assert all(r["trace"] is not None for r in a[:2]) and all(r["labels"] is None for r in a[:2]) and all(r["labels"] is not None for r in a[2:])
    want, dropped = risk_ref.train([r["trace"] for r in a[:2]], keys[:2], w, h)
    assert dropped == 0 and model.tobytes() == want.tobytes() and want["count"].sum() > 0
    for i in (2, 3):
        assert a[i]["labels"].tobytes() == risk_ref.predict(keys[i], want, 1, w, h).tobytes(), i
    assert a[2]["verify"][:, :4].sum() > 0
    given = {r["poc"]: torch.as_tensor(r["labels"]).cuda() for r in a[2:]}
    b, _, _ = run(labels=lambda poc, planes, obf: given[poc])
    assert all(np.array_equal(x["out"], y["out"]) for x, y in zip(a, b)) and np.array_equal(a[2]["verify"], b[2]["verify"])
    assert all(np.array_equal(x["sw_skip"], y["sw_skip"]) and np.array_equal(x["sw_term"], y["sw_term"]) for x, y in zip(a, b))
