"""The picture-level kernels past their loop and grid thresholds, on the emulators (tests/big_cases.py: one CTU row of 128, 129 and
130 CTUs, and 16 such pictures for the risk-table model): the second trip of report_pic and match_pic with a partial tail, the
long ordered walk of score_pic, the capped grid of risk_train with waves of two and of three units and the slot walk of risk_add
over all its slots, and the level plans of risk_predict / nobf_blocks with more workgroups per level than any smaller case.  Every
comparison is an equality of bytes with the numpy references.  tests/test_gpu_big_pictures.py runs the same cases
through the C ABI."""
import numpy as np
import pytest

import big_cases as BC
import cu_trace_ref
import labels_ref
import maps_cases as MC
import maps_ref
import report_cases as RC
import report_ref
import risk_ref
from cu_trace_testlib import load_emu as load_trace_emu
from test_maps import emu_maps, emu_match
from test_report import emu_report
from test_risk import emu_predict, emu_train, load_emu as load_risk_emu, ptrs

SIZES = sorted(BC.WIDTHS)
OK = 0


def poisoned(shape, dtype):
    return np.frombuffer(b"\xa5" * (int(np.prod(shape)) * np.dtype(dtype).itemsize), dtype).reshape(shape).copy()


# ---- fcu_picture_report
@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("n_ctu", SIZES)
def test_report_at_and_past_one_trip_of_the_record_walk(n_ctu, wide, built, pkg):
    """one picture into poisoned CTU records: the per-CTU records and the picture's sums, on the byte-exact load path and on the
    one the host would choose (wide for 128 and 129 CTUs, whose widths are multiples of 16)"""
    w, h = BC.size(n_ctu)
    org, rec, records, pic, ctu = BC.report_case(n_ctu, 5)
    buf = poisoned((1, n_ctu), pkg.engine.CTU_REPORT_DTYPE)
    got, got_ctu, path = emu_report(pkg, [(org, rec, records)], wide, ctu_buf=buf)
    assert path == (1 if wide and w % 16 == 0 else 0)
    report_ref.assert_equal(got[0], got_ctu[0], pic, ctu, (n_ctu, wide))


@pytest.mark.parametrize("n_ctu", SIZES)
def test_report_batch_of_three_past_one_trip(n_ctu, built, pkg):
    """three pictures of different content in one call: picture i's sums come from picture i's records, every trip of them"""
    cases = [BC.report_case(n_ctu, s) for s in (5, 8, 9)]
    got, got_ctu, _ = emu_report(pkg, [c[:3] for c in cases], ctu_buf=poisoned((3, n_ctu), pkg.engine.CTU_REPORT_DTYPE))
    for i, c in enumerate(cases):
        report_ref.assert_equal(got[i], got_ctu[i], c[3], c[4], (n_ctu, i))
    assert len({int(g["ssd"][0]) for g in got}) == 3 and len({int(g["bits"]) for g in got}) == 3


def test_report_of_planes_one_byte_off_past_one_trip(built, pkg):
    """129 CTUs, a width the wide loads would take: planes one byte off their alignment go the byte-exact way"""
    org, rec, records, pic, ctu = BC.report_case(129, 5)
    got, got_ctu, path = emu_report(pkg, [([RC.aligned(p, 1) for p in org], [RC.aligned(p, 1) for p in rec], records)])
    assert path == 0
    report_ref.assert_equal(got[0], got_ctu[0], pic, ctu)


# ---- fcu_split_match
@pytest.mark.parametrize("n_ctu", SIZES)
def test_split_match_at_and_past_one_trip_of_the_record_walk(n_ctu, built, pkg):
    """A against B (a seeded third of the CTUs differs: the first, the last and the first of the second trip among them), A against
    itself and B against A in one call"""
    w, h = BC.size(n_ctu)
    a, b, want, third = BC.match_case(n_ctu, 21)
    ctu = poisoned((3, n_ctu), pkg.engine.CTU_MATCH_DTYPE)
    got, ctu = emu_match(pkg, w, h, [a, a, b], [b, a, a], ctu)
    maps_ref.assert_match_equal(got[0], want, n_ctu)
    maps_ref.assert_match_equal(got[1], maps_ref.split_match(pkg, a, a, w, h), (n_ctu, "self"))
    swapped = dict(want, node=want["node"].transpose(0, 2, 1), only_a=want["only_b"], only_b=want["only_a"])
    maps_ref.assert_match_equal(got[2], swapped, (n_ctu, "swapped"))
    for k in maps_ref.MATCH_KEYS:                              # the per-CTU records add up to the picture's
        assert np.array_equal(ctu[0][k].astype(np.int64).sum(axis=0), np.asarray(got[0][k]).astype(np.int64)), k
    same = ctu[0]["part_equal"] == ctu[0]["part_total"]
    assert not ctu["pad"].any() and same[[i for i in range(n_ctu) if i not in third]].all() and not same[third].all()


# ---- fcu_label_score, fcu_trace_maps
def emu_score(lib, w, h, traces, labels, stale):
    n, nc = len(traces), traces[0].shape[0]
    tr, lb = [np.ascontiguousarray(t) for t in traces], [np.ascontiguousarray(q, np.int8) for q in labels]
    ctu = np.frombuffer(bytes([stale]) * (n * nc * 128), np.uint8).copy().view(cu_trace_ref.CTU_SCORE).reshape(n, nc)
    rec = np.frombuffer(bytes([stale]) * (n * 224), np.uint8).copy().view(cu_trace_ref.PIC_SCORE)
    assert lib.cu_trace_emu_score(w, h, n, ptrs(tr), ptrs(lb), rec.ctypes.data, ctu.ctypes.data) == OK, lib.cu_trace_emu_last_error()
    return ctu, rec


def test_label_score_sums_130_ctu_records_in_raster_order(built):
    """two pictures against two label arrays: per CTU and per picture the reference's bytes -- the loss sums bit for bit in the
    documented order, which the case tells from the reversed one (big_cases.score_case asserts it); a repeated call into other
    stale bytes gives the same"""
    lib = load_trace_emu()
    w, h = BC.size(BC.MANY)
    traces, labels, want_ctu, want_pic, _ = BC.score_case()
    ctu, rec = emu_score(lib, w, h, traces, labels, 0xA5)
    for i in range(2):
        assert ctu[i].tobytes() == want_ctu[i].tobytes(), i
        assert rec[i]["v"][:, 4:].tobytes() == want_pic[i]["v"][:, 4:].tobytes(), (i, rec[i]["v"][:, 4:], want_pic[i]["v"][:, 4:])
        assert rec[i].tobytes() == want_pic[i].tobytes(), i
        assert (BC.reversed_sums(ctu[i])[3] != rec[i]["v"][3, 4:]).any()
    assert rec["open"][:, 3].all() and rec["scored"][:, 3].all()
    ctu2, rec2 = emu_score(lib, w, h, traces, labels, 0x3C)
    assert ctu2.tobytes() == ctu.tobytes() and rec2.tobytes() == rec.tobytes()


def test_trace_maps_of_130_ctus(built):
    lib = load_trace_emu()
    w, h = BC.size(BC.MANY)
    traces, _, _, _, want = BC.score_case()
    NL = labels_ref.label_count(w, h)
    tr = [np.ascontiguousarray(t) for t in traces]
    lab, j0, j1 = poisoned((2, NL), np.int8), poisoned((2, NL), np.float64), poisoned((2, NL), np.float64)
    assert lib.cu_trace_emu_maps(w, h, 2, ptrs(tr), lab.ctypes.data, j0.ctypes.data, j1.ctypes.data) == OK, lib.cu_trace_emu_last_error()
    for i in range(2):
        for got, wnt in zip((lab[i], j0[i], j1[i]), want[i]):
            assert got.tobytes() == wnt.tobytes(), i
    assert (lab == labels_ref.FORCED).any() and (lab == labels_ref.SPLIT).any() and (lab == labels_ref.ABSENT).any()


# ---- fcu_decision_maps, fcu_nobf_maps
def test_decision_maps_of_130_ctus(built, pkg):
    w, h = BC.size(BC.MANY)
    r, obf, want = BC.maps_case()
    got, path, _ = emu_maps(w, h, [r], MC.ALL_FIELDS, mv=True, labels=True, obfs=[obf])
    assert path == 2
    maps_ref.assert_maps_equal(got[0], MC.select(want, MC.ALL_FIELDS), "strip")
    assert all((want["labels"][d] == maps_ref.FORCED).all() for d in range(3)) and (want["n_obf"][3] > 0).any()


def test_nobf_maps_of_130_ctus(built):
    lib = load_risk_emu()
    w, h = BC.size(BC.MANY)
    NL = labels_ref.label_count(w, h)
    cases = [BC.maps_case(s) for s in (11, 12)]
    obf = [np.ascontiguousarray(c[1]) for c in cases]
    out = poisoned((2, NL), np.uint16)
    assert lib.risk_emu_nobf(w, h, 2, ptrs(obf), out.ctypes.data) == OK
    for i, c in enumerate(cases):
        assert out[i].tobytes() == np.concatenate([m.reshape(-1) for m in c[2]["n_obf"]]).astype(np.uint16).tobytes(), i


# ---- the risk-table model
def test_risk_train_where_the_cap_on_the_slots_binds(built):
    """16 pictures of 130 CTUs = 2080 units on 128 workgroups: waves of two and of three units, risk_add over every slot.  Model
    bytes and `dropped`, over stale bytes, after a smaller batch and again"""
    lib = load_risk_emu()
    w, h = BC.size(BC.MANY)
    traces, keys, model, dropped, _, _ = BC.risk_case()
    got, d = emu_train(lib, w, h, traces, keys, stale=0xA5)
    assert got.tobytes() == model.tobytes() and d == dropped
    small, _ = emu_train(lib, w, h, traces[:BC.RISK_SPLIT], keys[:BC.RISK_SPLIT])
    assert small.tobytes() != model.tobytes()
    emu_train(lib, w, h, traces, keys, model=got)
    assert got.tobytes() == model.tobytes()
    one, d1 = emu_train(lib, w, h, traces, keys, groups=1)      # the same sums from one workgroup that walks every unit
    assert one.tobytes() == model.tobytes() and d1 == dropped


def test_risk_accumulate_below_and_at_the_cap(built):
    """3 + 13 pictures in two calls (both below the cap) equal the one batch at the cap; and the batch at the cap with 3 pictures
    accumulated on top equals the reference of all 19"""
    lib = load_risk_emu()
    w, h = BC.size(BC.MANY)
    traces, keys, model, dropped, _, _ = BC.risk_case()
    k = BC.RISK_SPLIT
    m, d1 = emu_train(lib, w, h, traces[:k], keys[:k])
    _, d2 = emu_train(lib, w, h, traces[k:], keys[k:], model=m, accumulate=1)
    assert m.tobytes() == model.tobytes() and d1 + d2 == dropped
    want, d3 = risk_ref.train(traces[:k], keys[:k], w, h, model=model)
    full, _ = emu_train(lib, w, h, traces, keys)
    _, d4 = emu_train(lib, w, h, traces[:k], keys[:k], model=full, accumulate=1)
    assert full.tobytes() == want.tobytes() and d4 == d3 == d1 and want.tobytes() != model.tobytes()


@pytest.mark.parametrize("min_count", [1, 3])
def test_risk_predict_of_130_ctus(min_count, built):
    lib = load_risk_emu()
    w, h = BC.size(BC.MANY)
    _, keys, model, _, labels, _ = BC.risk_case()
    got = emu_predict(lib, w, h, keys[:3] + keys[-1:], model, min_count, stale=0xA5)
    for i, j in enumerate((0, 1, 2, BC.RISK_PICS - 1)):
        assert got[i].tobytes() == labels[min_count][j].tobytes(), j
    assert (got == risk_ref.FORCED).any() and (got == risk_ref.ABSENT).any() and (got == risk_ref.SPLIT).any() and (got == risk_ref.NOT_SPLIT).any()
