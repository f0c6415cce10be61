"""What the CU-trace tests share (tests/test_cu_trace.py on the emulator, tests/test_gpu_cu_trace.py through the C ABI): the pictures,
the oracle's runs (it has no trace: everything is pinned through what it publishes -- the Verifying counters and total_cost),
the OBF maps that single out one CU, the ctypes binding of the emulator driver (tests/emu/cu_trace_emu.cpp, built by
__graft_entry__.build()) and one picture through it."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import cu_trace_ref as ref
import emu_py
import hmo_py
import labels_ref
import search_trace as st

_P = C.c_void_p
SIGNATURES = {
    "create": ([C.c_int] * 6 + [_P] * 7 + [C.c_int, C.c_double, C.c_int, C.c_int, _P, _P, C.c_int], _P),
    "destroy": ([_P], None), "n": ([_P], C.c_int), "run": ([_P], C.c_int),
    "set_decision": ([_P, C.c_int, _P, _P, C.c_int, _P], C.c_int), "set_labels": ([_P, _P], C.c_int), "set_trace": ([_P, _P], C.c_int),
    "set_trace_one": ([_P, C.c_int, _P, _P], C.c_int), "get_state_full": ([_P, C.c_int, _P, _P], None), "get_verify": ([_P, _P], None),
    "host": ([C.c_int] * 3, _P), "ranges": ([_P], None), "index": ([C.c_int] * 2, C.c_int), "sizeof": ([C.c_int], C.c_int),
    "score": ([C.c_int] * 3 + [_P] * 4, C.c_int), "maps": ([C.c_int] * 3 + [_P] * 4, C.c_int), "last_error": ([], C.c_char_p),
}
OK, ERR_ARG, ERR_STATE = 0, -2, -4
ALL_ON, ALL_OFF = (1, 1, 1, 1), (0, 0, 0, 0)


@functools.lru_cache(maxsize=None)
def load_emu():
    lib = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu", "libcu_trace_emu.so"))
    for name, (argtypes, restype) in SIGNATURES.items():
        f = getattr(lib, "cu_trace_emu_" + name)
        f.argtypes, f.restype = argtypes, restype
    return lib


@pytest.fixture(scope="session")
def trace_emu(built):
    return load_emu()


# ---- the pictures.  name: (width, height, QP, P picture)
PICS = {
    "one": (64, 64, 32, False),                 # one CTU: 85 CUs
    "i128": (128, 64, 32, False),               # two whole CTUs
    "cut": (136, 72, 27, False),                # cut CTUs on both edges
    "p": (128, 128, 32, True),                  # a P picture on a decided I picture, TZ search, one reference
}
P_BASE_QP, P_SEARCH_RANGE = 29, 8                # lowdelay_P: the P picture at POC 1 has slice QP 29 + 3 = 32


@functools.lru_cache(maxsize=None)
def inputs(pkg, pic):
    """(frame planes, p): p = None for an I picture, else dict lam, sr, fast, ref (the decided I picture's reconstruction)"""
    w, h, qp, is_p = PICS[pic]
    if not is_p:
        return tuple(np.ascontiguousarray(q) for q in pkg.synth.mixed(w, h, seed=9)), None
    f0, f1 = (st.moving_frame(pkg.synth, "mixed", w, h, 7, poc) for poc in range(2))
    _, qp0, lam0 = hmo_py.ldp_slice(0, P_BASE_QP)
    e = hmo_py.Encoder(*f0, qp0, lambda_override=lam0)
    e.compress_frame()
    _, qp1, lam1 = hmo_py.ldp_slice(1, P_BASE_QP)
    assert qp1 == qp
    return tuple(np.ascontiguousarray(q) for q in f1), dict(lam=lam1, sr=P_SEARCH_RANGE, fast=1, ref=[q.copy() for q in e.rec])


def _enc_kw(p):
    return {} if p is None else dict(ref=p["ref"], lambda_override=p["lam"], search_range=p["sr"], fast_search=p["fast"])


def n_ctus(pic):
    w, h = PICS[pic][:2]
    return ((w + 63) // 64) * ((h + 63) // 64)


def oracle(pkg, pic, state=hmo_py.TRAINING, obf=None, sw_skip=ALL_OFF, sw_term=ALL_OFF, slice_ctus=0):
    """the oracle's run of the picture as one chain (slice_ctus: SliceMode 1 slices inside it).  Returns dict verify [4, 6] (the
    counters of the whole picture), total_cost [n_ctu], ctus (bytes), rec, ctx, frac"""
    w, h, qp, is_p = PICS[pic]
    f, p = inputs(pkg, pic)
    enc = hmo_py.Encoder(*f, qp, slice_ctus=slice_ctus, **(dict(search_state_per_slice=1) if slice_ctus else {}), **_enc_kw(p))
    if state != hmo_py.TRAINING:
        enc.set_decision(state, np.ascontiguousarray(obf, np.int16), sw_skip, sw_term)
    enc.compress_frame()
    ctx, frac = enc.cabac(full=True)
    return dict(verify=enc.verify_counts() if state != hmo_py.TRAINING else None, total_cost=np.array([enc.ctu(a).total_cost for a in range(enc.n_ctu)]),
                ctus=enc.all_ctus_bytes(), rec=[q.copy() for q in enc.rec], ctx=ctx, frac=frac)


def emulate(lib, pkg, pic, kind=0, a=0, b=0, state=hmo_py.TRAINING, labels=None, obf=None, decision=None, trace=True, trace_buf=None):
    """One picture through the emulated chains (kind / a / b: cu_trace_emu_create).  trace: bind a trace (trace_buf: the array to
    use, else one filled with 0x5C -- the engine must clear what it visits).  Returns dict out (bytes), rec, states, verify, trace
    (structured [n_ctu, 85], or None)."""
    w, h, qp, is_p = PICS[pic]
    f, p = inputs(pkg, pic)
    org = [np.ascontiguousarray(q) for q in f]
    rec = [np.full_like(q, 0x5A) for q in org]
    n_ctu = n_ctus(pic)
    out = (hmo_py.Ctu * n_ctu)()
    C.memset(out, 0xA5, C.sizeof(out))
    pargs = [0, 0.0, 0, 0, None, None, 0]
    if p is not None:
        pads = emu_py.pad_planes([np.ascontiguousarray(q) for q in p["ref"]])
        ptrs = (C.c_void_p * 3)(*[q.ctypes.data for q in pads])
        pocs = np.array([0], np.int32)
        pargs = [1, p["lam"], p["sr"], p["fast"], ptrs, pocs.ctypes.data, 1]
    hd = lib.cu_trace_emu_create(kind, w, h, qp, a, b, *[q.ctypes.data for q in org], *[q.ctypes.data for q in rec], C.addressof(out), *pargs)
    assert hd, "the binder refused valid arguments"
    try:
        n = lib.cu_trace_emu_n(hd)
        sk, te, dex = decision if decision is not None else (ALL_OFF, ALL_OFF, 0)
        sk8, te8 = np.array(sk, np.uint8), np.array(te, np.uint8)
        obf16 = None if obf is None else np.ascontiguousarray(obf, np.int16)
        lab8 = None if labels is None else np.ascontiguousarray(labels, np.int8)
        tr = None
        if trace:
            tr = trace_buf if trace_buf is not None else np.frombuffer(bytes([0x5C]) * (n_ctu * 85 * 24), np.uint8).copy().view(ref.CU_TRACE).reshape(n_ctu, 85)
            assert lib.cu_trace_emu_set_trace(hd, tr.ctypes.data) == OK, lib.cu_trace_emu_last_error()

        def set_decision():
            assert lib.cu_trace_emu_set_decision(hd, state, sk8.ctypes.data, te8.ctypes.data, dex, None if obf16 is None else obf16.ctypes.data) == OK, lib.cu_trace_emu_last_error()

        def set_labels():
            if lab8 is not None:
                assert lib.cu_trace_emu_set_labels(hd, lab8.ctypes.data) == OK, lib.cu_trace_emu_last_error()
        for step in ((set_decision, set_labels) if obf16 is not None or state == hmo_py.TRAINING else (set_labels, set_decision)):
            step()
        assert lib.cu_trace_emu_run(hd) == n
        states = []
        for i in range(n):
            ctx, frac = np.zeros(176, np.uint8), C.c_uint64(0)
            lib.cu_trace_emu_get_state_full(hd, i, ctx.ctypes.data, C.byref(frac))
            states.append((ctx, frac.value))
        v = np.zeros((4, 6), np.float64)
        lib.cu_trace_emu_get_verify(hd, v.ctypes.data)
        return dict(out=bytes(out), rec=rec, states=states, verify=v, trace=tr)
    finally:
        lib.cu_trace_emu_destroy(hd)


@functools.lru_cache(maxsize=None)
def emu_trace(pkg, pic, kind=0, a=0, b=0):
    """the emulator's exhaustive (Training) run of a picture with a trace bound, computed once and kept (do not modify)"""
    return emulate(load_emu(), pkg, pic, kind, a, b)


# ---- the CUs of a picture and the OBF maps that single one out
def whole_cus(pic):
    """[(ctu, record index, depth, x, y, label element)] of the CUs that lie wholly inside the picture"""
    w, h = PICS[pic][:2]
    return [(a, t, d, x, y, idx) for a, t, d, x, y, idx, whole in ref.nodes(w, h) if whole]


def single_cu_obf(pic, d, x, y, positive_on_cu):
    """positive on the CU's 4x4 cells only, or everywhere but there"""
    w, h = PICS[pic][:2]
    s4 = (64 >> d) // 4
    obf = np.zeros((h // 4, w // 4), np.int16) if positive_on_cu else np.full((h // 4, w // 4), 3, np.int16)
    obf[y // 4:y // 4 + s4, x // 4:x // 4 + s4] = 3 if positive_on_cu else 0
    return obf


def assert_cu_pinned(verify, r, d, tag):
    """the oracle's Verifying counters on the map single_cu_obf(... positive_on_cu = not split_won) against record r of depth d: one
    FP (one FN) at that depth, and its loss sum is |J0 - J1| of the record alone -- one term added to 0.0, so exactly"""
    k = 3 if r["split_won"] else 1
    assert verify[d, k] == 1, tag + (verify[d],)
    assert verify[d, 4 + (k == 3)] == abs(float(r["j0"]) - float(r["j1"])), tag + (verify[d], float(r["j0"]), float(r["j1"]))


def score_labels(pic, name):
    """the label arrays the score tests use: what an OBF map expresses"""
    w, h = PICS[pic][:2]
    return labels_ref.obf_labels(labels_ref.obf_maps(w, h)[name], w, h)


def assert_losses_close(got, want, tag=()):
    """1e-9 relative: the terms are non-negative, so reordering n of them moves a sum by less than n 2^-53 relative (include/fcu.h)"""
    assert np.all(np.abs(got - want) <= 1e-9 * np.abs(want)), tag + (got, want)
