"""What the label tests share (tests/test_labels.py on the emulator, tests/test_gpu_labels.py through the C ABI): the pictures and
their chain layouts, the synthetic OBF maps and the decisions, the oracle's run of hmo_set_decision with an OBF map (computed once
per case and kept), the ctypes binding of the emulator driver (tests/emu/labels_emu.cpp, built by __graft_entry__.build()) and one
picture through it."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import emu_py
import hmo_py
import labels_ref
import search_trace as st
from tile_oracle import TileRef, tile_reference
from wpp_oracle import WppOracle

_P = C.c_void_p
SIGNATURES = {
    "create": ([C.c_int] * 6 + [_P] * 7 + [C.c_int, C.c_double, C.c_int, C.c_int, _P, _P, C.c_int], _P),
    "destroy": ([_P], None), "n": ([_P], C.c_int), "run": ([_P], C.c_int),
    "set_decision": ([_P, C.c_int, _P, _P, C.c_int, _P], C.c_int), "set_labels": ([_P, _P], C.c_int),
    "set_labels_one": ([_P, C.c_int, _P], C.c_int), "set_decision_one": ([_P, C.c_int, C.c_int, _P], C.c_int),
    "chain": ([_P, C.c_int, _P], C.c_int), "get_state_full": ([_P, C.c_int, _P, _P], None), "get_verify": ([_P, _P], None),
    "tu_trials": ([_P], C.c_ulonglong), "host": ([C.c_int] * 3, _P), "count": ([_P], C.c_int), "ranges": ([_P], None),
    "from_rasters": ([C.c_int] * 3 + [_P] * 3, C.c_int), "last_error": ([], C.c_char_p),
}
OK, ERR_ARG, ERR_STATE = 0, -2, -4


@functools.lru_cache(maxsize=None)
def load_emu():
    lib = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu", "liblabels_emu.so"))
    for name, (argtypes, restype) in SIGNATURES.items():
        f = getattr(lib, "labels_emu_" + name)
        f.argtypes, f.restype = argtypes, restype
    return lib


@pytest.fixture(scope="session")
def labels_emu(built):
    return load_emu()


# ---- the pictures.  name: (width, height, kind, a, b, P picture); kind / a / b as labels_emu_create takes them: 0 = slice chains of
# a CTUs (0: one chain), 1 = WaveFrontSynchro rows, 2 = a x b tiles
CASES = {
    "one": (128, 128, 0, 0, 0, False),          # four CTUs, one chain
    "cut": (136, 72, 0, 0, 0, False),           # cut CTUs on both edges: FORCED nodes
    "p": (128, 64, 0, 0, 0, True),              # a P picture on a decided I picture, TZ search, one reference
    "slices": (128, 128, 0, 2, 0, False),       # two slices of two CTUs
    "wpp": (128, 128, 1, 0, 0, False),          # two CTU rows as WaveFrontSynchro chains
    "tiles": (128, 128, 2, 2, 1, False),        # 2 x 1 tiles
}
CASE_QPS = [("one", 32), ("one", 37), ("cut", 32), ("p", 32), ("slices", 32), ("wpp", 32), ("tiles", 32)]
OBF_NAMES = ("random", "zero", "positive")
ALL_ON = (1, 1, 1, 1)


def _pattern(seed):
    """a seeded per-depth switch pattern (sw_skip, sw_term) with switches of both kinds on and off"""
    rng = np.random.default_rng(seed)
    while True:
        sk, te = rng.integers(0, 2, 4), rng.integers(0, 2, 4)
        if 0 < sk.sum() < 4 and 0 < te.sum() < 4:
            return tuple(int(v) for v in sk), tuple(int(v) for v in te)


# (sw_skip, sw_term, depth_exception): all switches on and two seeded per-depth patterns, each with depth_exception 0 and 1
DECISIONS = [(sk, te, dex) for sk, te in ((ALL_ON, ALL_ON), _pattern(101), _pattern(202)) for dex in (0, 1)]
P_BASE_QP, P_SEARCH_RANGE = 29, 8              # lowdelay_P: the P picture at POC 1 has slice QP 29 + 3 = 32


@functools.lru_cache(maxsize=None)
def inputs(pkg, case, qp):
    """(frame planes, p): p = None for an I picture, else dict lam, sr, fast, ref (the decided I picture's reconstruction)"""
    w, h, kind, a, b, is_p = CASES[case]
    if not is_p:
        return tuple(np.ascontiguousarray(q) for q in pkg.synth.mixed(w, h, seed=9)), None
    f0, f1 = (st.moving_frame(pkg.synth, "mixed", w, h, 7, poc) for poc in range(2))
    _, qp0, lam0 = hmo_py.ldp_slice(0, P_BASE_QP)
    e = hmo_py.Encoder(*f0, qp0, lambda_override=lam0)
    e.compress_frame()
    _, qp1, lam1 = hmo_py.ldp_slice(1, P_BASE_QP)
    assert qp1 == qp
    return tuple(np.ascontiguousarray(q) for q in f1), dict(lam=lam1, sr=P_SEARCH_RANGE, fast=1, ref=[q.copy() for q in e.rec])


@functools.lru_cache(maxsize=None)
def obf_map(case, name):
    w, h = CASES[case][:2]
    return labels_ref.obf_maps(w, h)[name]


def _enc_kw(p):
    return {} if p is None else dict(ref=p["ref"], lambda_override=p["lam"], search_range=p["sr"], fast_search=p["fast"])


@functools.lru_cache(maxsize=None)
def reference(pkg, case, qp, state, obf_name=None, decision=None):
    """The oracle's run of the picture: hmo_set_decision(state, switches, depth_exception, OBF map) on every chain's part, or the
    plain exhaustive run (state TRAINING).  Returns a TileRef-shaped object: ctus, rec, chains (ctx, frac, mv, n_ctu), excluded,
    verify -- what tile_oracle.assert_picture_equal compares."""
    w, h, kind, a, b, is_p = CASES[case]
    f, p = inputs(pkg, case, qp)
    dec = None
    if state != hmo_py.TRAINING:
        sk, te, dex = decision if decision is not None else ((0,) * 4, (0,) * 4, 0)
        dec = (state, obf_map(case, obf_name), sk, te, dex)
    if kind == 2:
        return tile_reference(f, qp, (a, b), wpp=False, decision=dec, **_enc_kw(p))
    r = TileRef(f, qp, (1, 1))
    r.ctus, r.excluded, r.chains, r.verify = b"", [], [], np.zeros((4, 6), np.float64)
    if kind == 1:
        o = WppOracle(*f, qp, decision=dec, **_enc_kw(p)).run()
        enc = o.enc
        for k in range(r.H):
            r._chain(o.row_state[k], o.row_int_mv[k], r.W, False)
        r.verify = o.verify
    else:
        n_ctu = r.W * r.H
        sl = a or n_ctu
        enc = hmo_py.Encoder(*f, qp, slice_ctus=a, **(dict(search_state_per_slice=1) if a else {}), **_enc_kw(p))
        for c in range(n_ctu):
            if c % sl == 0 and dec is not None:               # the counters of this slice chain alone
                enc.set_decision(*dec[:4], depth_exception=dec[4])
            enc.compress_ctu(c)
            if (c + 1) % sl == 0 or c + 1 == n_ctu:
                r._chain(enc.cabac(full=True), enc.test_int_mv(), min(sl, n_ctu - (c // sl) * sl), False)
                if dec is not None:
                    r.verify += enc.verify_counts()
    r.ctus = enc.all_ctus_bytes()
    r.rec = [q.copy() for q in enc.rec]
    return r


def emulate(lib, pkg, case, qp, state, labels=None, obf=None, decision=None):
    """One picture through the emulated chains.  labels: int8 [NL] or None; obf: int16 map or None; decision: (sw_skip, sw_term,
    depth_exception).  The order of the calls is the library's: the decision with an OBF map first and the labels after, or --
    without an OBF map -- the labels first.  Returns dict out (bytes of the Ctu array), rec, states, verify, trials."""
    w, h, kind, a, b, is_p = CASES[case]
    f, p = inputs(pkg, case, qp)
    org = [np.ascontiguousarray(q) for q in f]
    rec = [np.full_like(q, 0x5A) for q in org]
    n_ctu = ((w + 63) // 64) * ((h + 63) // 64)
    out = (hmo_py.Ctu * n_ctu)()
    C.memset(out, 0xA5, C.sizeof(out))
    pargs = [0, 0.0, 0, 0, None, None, 0]
    if p is not None:
        pads = emu_py.pad_planes([np.ascontiguousarray(q) for q in p["ref"]])
        ptrs = (C.c_void_p * 3)(*[q.ctypes.data for q in pads])
        pocs = np.array([0], np.int32)
        pargs = [1, p["lam"], p["sr"], p["fast"], ptrs, pocs.ctypes.data, 1]
    hd = lib.labels_emu_create(kind, w, h, qp, a, b, *[q.ctypes.data for q in org], *[q.ctypes.data for q in rec], C.addressof(out), *pargs)
    assert hd, "the binder refused valid arguments"
    try:
        n = lib.labels_emu_n(hd)
        sk, te, dex = decision if decision is not None else ((0,) * 4, (0,) * 4, 0)
        sk8, te8 = np.array(sk, np.uint8), np.array(te, np.uint8)
        obf16 = None if obf is None else np.ascontiguousarray(obf, np.int16)
        lab8 = None if labels is None else np.ascontiguousarray(labels, np.int8)

        def set_decision():
            assert lib.labels_emu_set_decision(hd, state, sk8.ctypes.data, te8.ctypes.data, dex, None if obf16 is None else obf16.ctypes.data) == OK, lib.labels_emu_last_error()

        def set_labels():
            if lab8 is not None:
                assert lab8.size == labels_ref.label_count(w, h)
                assert lib.labels_emu_set_labels(hd, lab8.ctypes.data) == OK, lib.labels_emu_last_error()
        for step in ((set_decision, set_labels) if obf16 is not None or state == hmo_py.TRAINING else (set_labels, set_decision)):
            step()
        assert lib.labels_emu_run(hd) == n
        states = []
        for i in range(n):
            ctx, frac = np.zeros(176, np.uint8), C.c_uint64(0)
            lib.labels_emu_get_state_full(hd, i, ctx.ctypes.data, C.byref(frac))
            states.append((ctx, frac.value))
        v = np.zeros((4, 6), np.float64)
        lib.labels_emu_get_verify(hd, v.ctypes.data)
        return dict(out=bytes(out), rec=rec, states=states, verify=v, trials=int(lib.labels_emu_tu_trials(hd)))
    finally:
        lib.labels_emu_destroy(hd)


def sorted_ctx(case):
    """the contexts to compare after a chain: all of an I picture's, a P picture's as the P tests select them"""
    return st.O_SORTED if CASES[case][5] else None


def assert_verify_equal(got, want, tag=()):
    """counts exact; the f64 loss sums equal too: engine and oracle add the same terms in the same order, chain by chain"""
    assert np.array_equal(got[:, :4], want[:, :4]), tag + ("TP / FP / TN / FN", got[:, :4], want[:, :4])
    assert np.array_equal(got[:, 4:], want[:, 4:]), tag + ("loss sums", got[:, 4:], want[:, 4:])
