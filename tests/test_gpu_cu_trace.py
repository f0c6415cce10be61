"""The CU trace, fcu_label_score and fcu_trace_maps through the C ABI on the GPU: the pins of tests/test_cu_trace.py against the
unchanged oracle (its Verifying counters on OBF maps that single out one CU; total_cost of pruned decisions), the two kernels
against the numpy reference (tests/cu_trace_ref.py), and the trace of the HIP engine against the emulator's, byte for byte."""
import ctypes as C

import numpy as np
import pytest

import cu_trace_ref as ref
import hmo_py
import labels_ref
from cu_trace_testlib import ALL_OFF, PICS, P_BASE_QP, assert_cu_pinned, emu_trace, inputs, n_ctus, oracle, score_labels, single_cu_obf, trace_emu, whole_cus  # noqa: F401

pytestmark = pytest.mark.gpu


class Picture:
    """one picture bound on the device as the chains of a layout, all sharing one trace"""

    def __init__(self, pkg, pic, **layout):
        import torch
        self.pkg, self.pic, self.torch = pkg, pic, torch
        self.w, self.h, self.qp, is_p = PICS[pic]
        self.lo = pkg.layout.PictureLayout(self.w, self.h, **layout)
        self.eng = pkg.CuEngine(self.w, self.h, max_chains=self.lo.chains)
        self.f, p = inputs(pkg, pic)
        self.kw = {}
        if p is not None:
            fp = pkg.engine.ldp_slice(P_BASE_QP, 1)
            fp.search_range, fp.fast_search = p["sr"], p["fast"]
            assert fp.qp == self.qp
            self.kw = dict(params=fp, ref=self.eng.pad_reference([torch.as_tensor(q).cuda() for q in p["ref"]]))

    def decide(self, trace=True, state=hmo_py.TRAINING, labels=None):
        """returns dict out (bytes), rec, states, verify, trace (device tensor, or None) -- the trace array starts as 0x5C bytes"""
        eng, torch = self.eng, self.torch
        n, rec, out = eng.init_picture(0, self.f, self.qp, self.lo, **self.kw)
        tr = None
        if trace:
            tr = torch.full((eng.n_ctu * 85 * 24,), 0x5C, dtype=torch.uint8, device="cuda")
            for k in range(n):
                eng.enable_cu_trace(k, tr)
        if labels is not None:
            eng.set_labels(range(n), torch.as_tensor(np.ascontiguousarray(labels, np.int8)).cuda())
            for k in range(n):
                eng.set_decision(k, state)
        eng.compress_pictures(0, 1, self.lo)
        eng.sync()
        return dict(out=out.cpu().numpy().tobytes(), rec=[q.cpu().numpy() for q in rec], states=[eng.ctx_state(k, full=True) for k in range(n)],
                    verify=eng.verify_counts(0, n), trace=tr)

    def close(self):
        self.eng.destroy()


def _host(p, tr):
    return p.eng.cu_trace_array(tr)


def test_every_cu_of_a_ctu_one_at_a_time_against_the_oracle(pkg):
    """64x64 I picture: all 85 records of the HIP engine pinned, one at a time, through the oracle's Verifying counters"""
    p = Picture(pkg, "one")
    try:
        tr = _host(p, p.decide()["trace"])
        assert tr["valid"].all() and tr["split_tried"].all() and not tr["pad"].any()
        for a, t, d, x, y, idx in whole_cus("one"):
            r = tr[a, t]
            v = oracle(pkg, "one", hmo_py.VERIFYING, single_cu_obf("one", d, x, y, not r["split_won"]))["verify"]
            assert_cu_pinned(v, r, d, (a, t, d, x, y))
    finally:
        p.close()


def test_absolute_costs_at_depth_0(pkg):
    """128x64 as slices of one CTU: J0 / J1 of the depth-0 records are the oracle's total_cost with the CTU terminated / with the
    whole-CU check skipped; the exhaustive total_cost is the winner's"""
    pic = "i128"
    w, h = PICS[pic][:2]
    p = Picture(pkg, pic, slice_ctus=1)
    try:
        tr = _host(p, p.decide()["trace"])
        zero, pos = np.zeros((h // 4, w // 4), np.int16), np.full((h // 4, w // 4), 3, np.int16)
        j0 = oracle(pkg, pic, hmo_py.TESTING, zero, ALL_OFF, (1, 0, 0, 0), slice_ctus=1)["total_cost"]
        j1 = oracle(pkg, pic, hmo_py.TESTING, pos, (1, 0, 0, 0), ALL_OFF, slice_ctus=1)["total_cost"]
        ex = oracle(pkg, pic, slice_ctus=1)["total_cost"]
        for a in range(n_ctus(pic)):
            r = tr[a, 0]
            assert r["valid"] and r["j0"] == j0[a] and r["j1"] == j1[a] and ex[a] == (r["j1"] if r["split_won"] else r["j0"]), (a, r)
    finally:
        p.close()


CASES = {"cut": ("cut", {}), "p": ("p", {}), "wpp": ("p", dict(wpp=True)), "tiles": ("cut", dict(tiles=(2, 1)))}


@pytest.mark.parametrize("case", list(CASES))
def test_trace_score_and_maps(pkg, trace_emu, case):
    """One picture per layout -- one chain, a P picture, WaveFrontSynchro rows, 2 x 1 tiles, all chains sharing one trace: the records
    without a trace are unchanged; the trace equals the emulator's byte for byte (one chain; rows and tiles: a cleared array with
    every whole CU visited); score and maps equal the numpy reference byte for byte, two pictures in one call, again on a repeated
    call into other stale bytes, the labels at an odd base address"""
    import torch
    pic, layout = CASES[case]
    w, h = PICS[pic][:2]
    p = Picture(pkg, pic, **layout)
    try:
        plain, e = p.decide(trace=False), p.decide()
        assert plain["out"] == e["out"] and all(np.array_equal(a, b) for a, b in zip(plain["rec"], e["rec"]))
        assert all(np.array_equal(s[0], t[0]) and s[1] == t[1] for s, t in zip(plain["states"], e["states"]))
        tr = _host(p, e["trace"])
        whole = {(a, t) for a, t, *_ in whole_cus(pic)}
        assert all(bool(tr[a, t]["valid"]) == ((a, t) in whole) for a in range(tr.shape[0]) for t in range(85)) and not tr["pad"].any()
        assert tr[tr["valid"] == 0].tobytes() == bytes(24 * int((tr["valid"] == 0).sum()))
        if not layout:
            assert tr.tobytes() == emu_trace(pkg, pic)["trace"].tobytes()
        # a second picture: the first one's records with the CTUs in reverse order
        tr2 = torch.as_tensor(np.ascontiguousarray(tr[::-1]).view(np.uint8).reshape(-1)).cuda()
        lab0 = score_labels(pic, "random")
        lab1 = lab0.copy()
        hit = np.random.default_rng(5).random(lab1.size)
        lab1[hit < 0.15], lab1[(hit >= 0.15) & (hit < 0.3)], lab1[(hit >= 0.3) & (hit < 0.45)] = labels_ref.ABSENT, labels_ref.FORCED, 7
        labs = torch.as_tensor(np.stack([lab0, lab1])).cuda()
        rec, ctu = p.eng.label_score([e["trace"], tr2], labs, ctu=True)
        for i, (t, q) in enumerate(((tr, lab0), (tr[::-1], lab1))):
            rc, rp = ref.score(t, q, w, h)
            assert ctu[i].tobytes() == rc.tobytes() and rec[i].tobytes() == rp.tobytes(), (case, i)
        assert rec["scored"][0].sum() > 0 and rec["open"][1].sum() > 0
        again = p.eng.label_score([e["trace"], tr2], labs)
        assert again.tobytes() == rec.tobytes()
        if not layout and not PICS[pic][3]:                  # an I picture as one chain: the engine's own Verifying counters
            own = p.decide(trace=False, state=hmo_py.VERIFYING, labels=lab0)["verify"]
            assert np.array_equal(rec["v"][0][:, :4], own[:, :4]) and np.all(np.abs(rec["v"][0][:, 4:] - own[:, 4:]) <= 1e-9 * np.abs(own[:, 4:]))
        m = p.eng.trace_maps([e["trace"], tr2], labels=True, costs=True)
        for i, t in enumerate((tr, tr[::-1])):
            for got, want in zip((m["labels"][i], m["j0"][i], m["j1"][i]), ref.maps(t, w, h)):
                assert got.cpu().numpy().tobytes() == want.tobytes(), (case, i)
        # the label output at an odd address, over other stale bytes, through the C ABI
        NL = p.eng.label_count()
        buf = torch.full((NL + 9,), 0xC4, dtype=torch.uint8, device="cuda")
        ptrs = (C.c_void_p * 1)(e["trace"].data_ptr())
        assert p.eng.lib.fcu_trace_maps(p.eng.h, 1, ptrs, buf.data_ptr() + 1, None, None, None, None) == 0
        o = buf.cpu().numpy()
        assert o[0] == 0xC4 and np.all(o[NL + 1:] == 0xC4) and o[1:NL + 1].tobytes() == ref.maps(tr, w, h)[0].tobytes()
    finally:
        p.close()


def test_guards_through_the_abi(pkg):
    import torch
    eng = pkg.CuEngine(128, 64, max_chains=1)
    try:
        tr = torch.zeros(eng.n_ctu * 85 * 24 + 8, dtype=torch.uint8, device="cuda")
        with pytest.raises(pkg.FcuError, match="not bound"):
            eng.enable_cu_trace(0, tr)
        eng.init_chain(0, pkg.synth.mixed(128, 64, seed=9), qp=32)
        assert eng.lib.fcu_chain_set_cu_trace(eng.h, 0, tr.data_ptr() + 4) == -2 and b"multiple of 8" in eng.lib.fcu_last_error()
        assert eng.lib.fcu_chain_set_cu_trace(eng.h, 1, tr.data_ptr()) == -2
        eng.enable_cu_trace(0, tr)
        eng.disable_cu_trace(0)
        lab = torch.zeros(eng.label_count(), dtype=torch.int8, device="cuda")
        one, none, labs = (C.c_void_p * 1)(tr.data_ptr()), (C.c_void_p * 1)(None), (C.c_void_p * 1)(lab.data_ptr())
        rec = np.zeros(1, ref.PIC_SCORE)
        L, h = eng.lib, eng.h
        for args, word in (((0, one, labs, rec.ctypes.data), b"n_pics"), ((1, None, labs, rec.ctypes.data), b"dev_trace is null"), ((1, one, None, rec.ctypes.data), b"dev_labels is null"),
                           ((1, none, labs, rec.ctypes.data), b"dev_trace[0]"), ((1, one, none, rec.ctypes.data), b"dev_labels[0]"), ((1, one, labs, None), b"host_scores")):
            assert L.fcu_label_score(h, *args, None, None, None) == -2 and word in L.fcu_last_error(), word
        for args, word in (((0, one, lab.data_ptr(), None, None), b"n_pics"), ((1, None, lab.data_ptr(), None, None), b"dev_trace is null"), ((1, none, lab.data_ptr(), None, None), b"dev_trace[0]"),
                           ((1, one, None, None, None), b"no output"), ((1, one, None, tr.data_ptr() + 4, None), b"multiples of 8")):
            assert L.fcu_trace_maps(h, *args, None, None) == -2 and word in L.fcu_last_error(), word
    finally:
        eng.destroy()


def test_sequence_decider_returns_the_trace_of_its_training_pictures(pkg):
    """SequenceDecider(cu_trace=True): the Training picture's result carries its trace, the others none; the decision is the one
    without the option; score and maps take the result dict as it is"""
    w, h, qp = 128, 128, 32
    frames = [pkg.synth.mixed(w, h, seed=s) for s in (9, 10)]

    def run(cu_trace):
        sched = pkg.sequence.FastDecisionSchedule(period=2, n_training=1, n_verifying=1)
        dec = pkg.sequence.SequenceDecider(w, h, qp, slice_ctus=2, fast=True, schedule=sched, cu_trace=cu_trace)
        try:
            res = [dec.decide(f) for f in frames]
            extra = None
            if cu_trace:
                m = dec.eng.trace_maps([res[0]], labels=True, costs=True)
                extra = (dec.eng.cu_trace_array(res[0]["cu_trace"]), {k: v.cpu().numpy() for k, v in m.items()})
            return [dict(r, out=r["out"].cpu().numpy().copy()) for r in res], extra
        finally:
            dec.close()
    (a, _), (b, (tr, m)) = run(False), run(True)
    assert "cu_trace" in b[0] and "cu_trace" not in b[1] and "cu_trace" not in a[0]
    assert all(np.array_equal(x["out"], y["out"]) for x, y in zip(a, b)) and np.array_equal(a[1]["verify"], b[1]["verify"])
    assert tr["valid"].all()
    for got, want in zip((m["labels"][0], m["j0"][0], m["j1"][0]), ref.maps(tr, w, h)):
        assert got.tobytes() == want.tobytes()
