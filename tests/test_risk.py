"""The risk-table model on the emulator: the kernel bodies of fcu_risk_train, fcu_risk_predict and fcu_nobf_maps (csrc/fcu_risk.h)
compiled for the CPU (tests/emu/risk_emu.cpp) against the plain-numpy reference (tests/risk_ref.py).  Every comparison is an
equality of bytes.  tests/test_gpu_risk.py repeats the cases through the C ABI."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import cu_trace_ref
import hmo_py
import labels_ref
import maps_cases
import maps_ref
import risk_cases
import risk_ref
from cu_trace_testlib import PICS, emu_trace, inputs, trace_emu  # noqa: F401

OK, ERR_ARG = 0, -2
_P = C.c_void_p
SIGNATURES = {"train": ([C.c_int] * 3 + [_P] * 3 + [C.c_int, _P, C.c_int], C.c_int), "predict": ([C.c_int] * 3 + [_P, _P, C.c_int, _P], C.c_int),
              "nobf": ([C.c_int] * 3 + [_P, _P], C.c_int), "table": ([_P, C.c_int, _P], None), "last_error": ([], C.c_char_p), "sizeof": ([], C.c_int),
              "label_count": ([C.c_int] * 2, C.c_int)}


@functools.lru_cache(maxsize=None)
def load_emu():
    lib = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu", "librisk_emu.so"))
    for name, (argtypes, restype) in SIGNATURES.items():
        f = getattr(lib, "risk_emu_" + name)
        f.argtypes, f.restype = argtypes, restype
    return lib


@pytest.fixture(scope="session")
def risk_emu(built):
    return load_emu()


def ptrs(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def emu_train(lib, w, h, traces, keys, model=None, accumulate=0, groups=0, stale=0x5C):
    """risk_emu_train into `model` (or a buffer of stale bytes): (model, dropped)"""
    tr, ky = [np.ascontiguousarray(t) for t in traces], [np.ascontiguousarray(k, np.uint16) for k in keys]
    m = np.frombuffer(bytes([stale]) * risk_ref.MODEL.itemsize, np.uint8).copy().view(risk_ref.MODEL) if model is None else model
    dropped = C.c_uint32(0xDEAD)
    assert lib.risk_emu_train(w, h, len(tr), ptrs(tr), ptrs(ky), m.ctypes.data, accumulate, C.byref(dropped), groups) == OK, lib.risk_emu_last_error()
    return m, dropped.value


def emu_predict(lib, w, h, keys, model, min_count, stale=0x33):
    ky = [np.ascontiguousarray(k, np.uint16) for k in keys]
    n, NL = len(ky), labels_ref.label_count(w, h)
    out = np.full(n * NL + 16, stale, np.uint8)
    m = np.ascontiguousarray(model)
    assert lib.risk_emu_predict(w, h, n, ptrs(ky), m.ctypes.data, min_count, out.ctypes.data + 8) == OK, lib.risk_emu_last_error()
    assert np.all(out[:8] == stale) and np.all(out[8 + n * NL:] == stale)      # nothing written outside
    return out[8:8 + n * NL].view(np.int8).reshape(n, NL).copy()


def test_layout(risk_emu, built, pkg):
    e = pkg.engine
    assert risk_emu.risk_emu_sizeof() == 24672 == risk_ref.MODEL.itemsize == e.RISK_MODEL_DTYPE.itemsize and e.RISK_MODEL_DTYPE == risk_ref.MODEL
    L = C.CDLL(pkg.lib_path())
    assert L.fcu_abi_sizeof(17) == 24672
    for w, h in risk_cases.SIZES:
        assert risk_emu.risk_emu_label_count(w, h) == labels_ref.label_count(w, h)


@pytest.mark.parametrize("size", risk_cases.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("n_pics", [1, 3])
def test_model_equals_the_reference(risk_emu, size, n_pics):
    """byte-equal model and `dropped`, over stale bytes (accumulate 0 clears nothing), for one picture and a batch of three, whatever
    the number of workgroups the batch is dealt to; a repeated call gives identical bytes"""
    w, h = size
    traces, keys, model, dropped, _ = risk_cases.case(w, h, n_pics)
    got, d = emu_train(risk_emu, w, h, traces, keys)
    assert got.tobytes() == model.tobytes() and d == dropped
    for groups, stale in ((1, 0xA7), (5, 0x00)):
        again, d2 = emu_train(risk_emu, w, h, traces, keys, groups=groups, stale=stale)
        assert again.tobytes() == model.tobytes() and d2 == dropped, groups
    emu_train(risk_emu, w, h, traces, keys, model=got)
    assert got.tobytes() == model.tobytes()


@pytest.mark.parametrize("size", risk_cases.SIZES, ids=lambda s: "%dx%d" % s)
def test_accumulate_in_two_calls_equals_one_batch(risk_emu, size):
    w, h = size
    traces, keys, model, dropped, _ = risk_cases.case(w, h, 3)
    m, d1 = emu_train(risk_emu, w, h, traces[:1], keys[:1])
    _, d2 = emu_train(risk_emu, w, h, traces[1:], keys[1:], model=m, accumulate=1)
    assert m.tobytes() == model.tobytes() and d1 + d2 == dropped
    assert m.tobytes() == risk_ref.train(traces[1:], keys[1:], w, h, model=risk_ref.train(traces[:1], keys[:1], w, h)[0])[0].tobytes()


@pytest.mark.parametrize("size", risk_cases.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("min_count", risk_cases.MIN_COUNTS)
def test_labels_and_table_equal_the_reference(risk_emu, size, min_count):
    w, h = size
    _, keys, model, _, labels = risk_cases.case(w, h, 3)
    got = emu_predict(risk_emu, w, h, keys, model, min_count)
    for i in range(3):
        assert got[i].tobytes() == labels[min_count][i].tobytes(), i
    tab = np.full((4, 257), 0x44, np.int8)
    risk_emu.risk_emu_table(np.ascontiguousarray(model).ctypes.data, min_count, tab.ctypes.data)
    assert tab.tobytes() == risk_ref.table(model, min_count).tobytes()
    if w * h >= 64 * 64:                                      # the tie gives SPLIT; the empty bin and the two-sample bin follow min_count
        assert tab[3, risk_cases.KEY_TIE] == (risk_ref.SPLIT if min_count < 3 or model["count"][3, risk_cases.KEY_TIE].sum() >= 3 else risk_ref.ABSENT)
        assert tab[3, risk_cases.KEY_EMPTY] == (risk_ref.SPLIT if min_count == 0 else risk_ref.ABSENT)
        assert tab[3, risk_cases.KEY_TWO] == (risk_ref.ABSENT if min_count == 3 else tab[3, risk_cases.KEY_TWO]) and (got == risk_ref.FORCED).any() == (w % 64 != 0 or h % 64 != 0)
        assert (got == risk_ref.ABSENT).any()


@pytest.mark.parametrize("size", maps_cases.SIZES, ids=lambda s: "%dx%d" % s)
def test_nobf_maps_equal_the_maps_reference(risk_emu, size):
    """the N_OBF map of an undecided picture is the one fcu_decision_maps gives: maps_ref on the cases of maps_cases, two pictures"""
    w, h = size
    NL = labels_ref.label_count(w, h)
    obf = [np.ascontiguousarray(maps_cases.case(w, h, s)[1]) for s in (3, 4)]
    out = np.full(2 * NL + 8, 0x6B6B, np.uint16)
    assert risk_emu.risk_emu_nobf(w, h, 2, ptrs(obf), out.ctypes.data + 8) == OK
    assert np.all(out[:4] == 0x6B6B) and np.all(out[4 + 2 * NL:] == 0x6B6B)
    for i, s in enumerate((3, 4)):
        want = np.concatenate([m.reshape(-1) for m in maps_cases.case(w, h, s)[2]["n_obf"]])
        assert out[4 + i * NL:4 + (i + 1) * NL].tobytes() == want.astype(np.uint16).tobytes(), i


@pytest.mark.parametrize("size", [(208, 136), (128, 64)], ids=lambda s: "%dx%d" % s)
def test_a_hand_written_model_gives_the_naive_labels(risk_emu, size):
    """bin 0 -> NOT_SPLIT, every other bin -> SPLIT, predicted on the N_OBF keys: the label array the Naive model gives
    (labels_ref.obf_labels), which test_labels.py shows to decide what the OBF map decides"""
    w, h = size
    NL = labels_ref.label_count(w, h)
    model = np.zeros((), risk_ref.MODEL)
    model["risk"][:, 0, 0], model["risk"][:, 1:, 1] = 5, 5      # bin 0: risk[1] < risk[0]; the others: risk[0] < risk[1]
    model["count"][...] = 1
    for name, obf in labels_ref.obf_maps(w, h).items():
        obf = np.ascontiguousarray(obf)
        keys = np.zeros(NL, np.uint16)
        assert risk_emu.risk_emu_nobf(w, h, 1, ptrs([obf]), keys.ctypes.data) == OK
        got = emu_predict(risk_emu, w, h, [keys], model, 1)[0]
        assert got.tobytes() == labels_ref.obf_labels(obf, w, h).tobytes(), name


def test_refusals_name_their_argument(risk_emu):
    w, h = 64, 64
    traces, keys, model, _, _ = risk_cases.case(w, h, 1)
    NL = labels_ref.label_count(w, h)
    tr, ky, m = ptrs([np.ascontiguousarray(traces[0])]), ptrs([np.ascontiguousarray(keys[0])]), np.zeros(24672 + 8, np.uint8)
    none = (C.c_void_p * 1)(None)
    out, obf = np.zeros(NL, np.int8), np.zeros((16, 16), np.int16)
    L, mp = risk_emu, m.ctypes.data
    assert mp % 8 == 0
    for args, word in (((0, tr, ky, mp, 0, None, 0), b"n_pics"), ((1, None, ky, mp, 0, None, 0), b"dev_trace is null"), ((1, tr, None, mp, 0, None, 0), b"dev_keys is null"),
                       ((1, none, ky, mp, 0, None, 0), b"dev_trace[0]"), ((1, tr, none, mp, 0, None, 0), b"dev_keys[0]"), ((1, tr, ky, None, 0, None, 0), b"dev_model is null"),
                       ((1, tr, ky, mp + 4, 0, None, 0), b"dev_model starts at a multiple of 8"), ((1, tr, ky, mp, 2, None, 0), b"accumulate")):
        assert L.risk_emu_train(w, h, *args) == ERR_ARG and word in L.risk_emu_last_error(), word
    many = (1 << 22) // NL + 1                                 # the 2^22 limit is checked before any entry is read
    big = (C.c_void_p * many)(*([tr[0]] * many))
    assert L.risk_emu_train(w, h, many, big, big, mp, 0, None, 0) == ERR_ARG and b"2^22" in L.risk_emu_last_error()
    for args, word in (((0, ky, mp, 1, out.ctypes.data), b"n_pics"), ((1, None, mp, 1, out.ctypes.data), b"dev_keys is null"), ((1, none, mp, 1, out.ctypes.data), b"dev_keys[0]"),
                       ((1, ky, None, 1, out.ctypes.data), b"dev_model is null"), ((1, ky, mp + 4, 1, out.ctypes.data), b"multiple of 8"), ((1, ky, mp, -1, out.ctypes.data), b"min_count"),
                       ((1, ky, mp, 1, None), b"dev_labels is null")):
        assert L.risk_emu_predict(w, h, *args) == ERR_ARG and word in L.risk_emu_last_error(), word
    for args, word in (((0, ptrs([obf]), out.ctypes.data), b"n_pics"), ((1, None, out.ctypes.data), b"dev_obf is null"), ((1, none, out.ctypes.data), b"dev_obf[0]"), ((1, ptrs([obf]), None), b"dev_nobf is null")):
        assert L.risk_emu_nobf(w, h, *args) == ERR_ARG and word in L.risk_emu_last_error(), word


def test_one_real_picture_loses_no_more_than_the_fixed_labellings(risk_emu, pkg):
    """128x64, QP 32, decided exhaustively with a trace (the emulated engine); trained on its own N_OBF keys and predicted on them
    with min_count 1.  The model minimises the quantised loss over all key-wise labellings and every sample loses less than 1/256
    to the floor, so loss(model) <= loss(L) + n / 256 + 1e-9 loss(L) (the double-sum slack fcu_label_score documents) for the three
    key-wise labellings Naive, all SPLIT and all NOT_SPLIT.  loss = FPLoss + FNLoss counted by cu_trace_ref in doubles"""
    w, h = PICS["i128"][:2]
    tr = emu_trace(pkg, "i128")["trace"]
    assert tr["valid"].all() and tr["split_tried"].all() and tr["whole_tried"].all()
    obf = np.ascontiguousarray(hmo_py.obf_prepass(inputs(pkg, "i128")[0][0])[0])      # the picture's own OBF map (the oracle's pre-pass)
    NL = labels_ref.label_count(w, h)
    keys = np.zeros(NL, np.uint16)
    assert risk_emu.risk_emu_nobf(w, h, 1, ptrs([obf]), keys.ctypes.data) == OK
    assert keys.tobytes() == np.concatenate([m.reshape(-1) for m in maps_ref.nobf_maps(obf, w, h)]).astype(np.uint16).tobytes()
    model, dropped = emu_train(risk_emu, w, h, [tr], [keys])
    assert dropped == 0 and model.tobytes() == risk_ref.train([tr], [keys], w, h)[0].tobytes()
    lab = emu_predict(risk_emu, w, h, [keys], model, 1)[0]
    assert lab.tobytes() == risk_ref.predict(keys, model, 1, w, h).tobytes()
    got, n = risk_ref.loss(tr, lab, w, h)
    assert n == tr.size and (cu_trace_ref.score(tr, lab, w, h)[1]["open"] == 0).all()
    naive = labels_ref.obf_labels(obf, w, h)
    assert 0 < (naive == risk_ref.SPLIT).sum() < NL
    for name, other in (("naive", naive), ("split", np.full(NL, risk_ref.SPLIT, np.int8)), ("not_split", np.full(NL, risk_ref.NOT_SPLIT, np.int8))):
        ref_loss = risk_ref.loss(tr, other, w, h)[0]
        print("loss(model) = %.6f, loss(%s) = %.6f, n = %d" % (got, name, ref_loss, n))
        assert got <= ref_loss + n / 256 + 1e-9 * ref_loss, (name, got, ref_loss)
