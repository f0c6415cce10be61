"""level_choice() (csrc/fcu_engine.h): the emulator built with -DFCU_EMU_CHECK_RDOQ_LEVELS
(tests/emu/rdoq_level_emu.cpp: every coefficient with uiMaxAbsLevel > 0 of every rdoq() / rdoq_wave() call is also priced by
coded_level() + ic_rate(), the definition, and the emulator aborts on a difference in level, costs, rates or deltaU) against the
oracle, on every fcu_ctu_out array, the reconstruction and the CABAC state; and a check -- by the emulator's counters
(fcu_emu_level_cnt) -- that the frames reach every case of the level choice."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emu_py
import hmo_py
from rdoq_level_cases import COUNTERS, INTRA_CASES, LDP_CLIP, MUST_BE_ZERO, frame, ldp_pictures

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
LIB = os.path.join(EMU_DIR, "libfcu_emu_rdoq_level.so")
PROTOS = ("fcu_emu_create", "fcu_emu_destroy", "fcu_emu_compress_ctu", "fcu_emu_get_state", "fcu_emu_set_decision", "fcu_emu_get_verify",
          "fcu_emu_tu_trials", "fcu_emu_set_p", "fcu_emu_set_lambda", "fcu_emu_get_state_full", "fcu_emu_set_rdoq", "fcu_emu_set_amp",
          "fcu_emu_set_cabac_b", "fcu_emu_set_col")


@pytest.fixture(scope="module")
def lib(built):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-shared", "-o", LIB, "rdoq_level_emu.cpp"], cwd=EMU_DIR)
    std = emu_py.load()
    chk = C.CDLL(LIB)
    for name in PROTOS:                                          # the plain emulator's prototypes are the check build's too
        f, g = getattr(std, name), getattr(chk, name)
        g.argtypes, g.restype = f.argtypes, f.restype
    return chk


@pytest.fixture(scope="module")
def counts():
    """what the picture tests of this session counted, and how many of them ran"""
    return {"total": np.zeros(len(COUNTERS), np.int64), "ran": 0}


def _emu_picture(e, o, full, what):
    """one picture, CTU by CTU, on the oracle and on the checking emulator: arrays and coder state after every CTU, the
    reconstruction at the end"""
    import search_trace as st
    for a in range(o.n_ctu):
        o.compress_ctu(a)
        e.compress_ctu(a)
        A, B = o.ctu_arrays(a), e.ctu_arrays(a)
        for k, v in A.items():
            assert (np.array_equal(v, B[k]) if isinstance(v, np.ndarray) else v == B[k]), (what, a, k)
        (ca, fa), (cb, fb) = o.cabac(full=full), e.cabac(full=full)
        assert fa == fb, (what, a, "Q15 count")
        assert np.array_equal(ca[st.O_SORTED], cb[st.O_SORTED]) if full else np.array_equal(ca, cb), (what, a, "contexts")
    for p, q in zip(o.rec, e.rec):
        assert np.array_equal(p, q), (what, "reconstruction")


def _counted(lib, acc, run):
    cnt = (C.c_ulonglong * len(COUNTERS)).in_dll(lib, "fcu_emu_level_cnt")
    before = np.array(list(cnt), dtype=np.int64)
    run()
    d = np.array(list(cnt), dtype=np.int64) - before
    acc["total"] += d
    acc["ran"] += 1
    print(dict(zip(COUNTERS, d.tolist())))


N_PICTURE_TESTS = len(INTRA_CASES) + 1                          # the intra frames and the clip


@pytest.mark.parametrize("case", INTRA_CASES, ids=lambda c: "%s-%dx%d-qp%d" % c)
def test_intra_frames_price_levels_as_the_definition(lib, counts, pkg, monkeypatch, case):
    monkeypatch.setattr(emu_py, "load", lambda: lib)
    src, w, h, qp = case
    f = frame(pkg, src, w, h)
    e = emu_py.EmuEncoder(*f, qp)
    assert e.lib is lib
    _counted(lib, counts, lambda: _emu_picture(e, hmo_py.Encoder(*f, qp), False, case))


def test_lowdelay_p_clip_prices_levels_as_the_definition(lib, counts, pkg, monkeypatch):
    monkeypatch.setattr(emu_py, "load", lambda: lib)
    _, _, _, base_qp, _, _, sr = LDP_CLIP

    def run():
        prev = None
        for poc, f in enumerate(ldp_pictures(pkg)):
            _, qp, lam = hmo_py.ldp_slice(poc, base_qp)
            if poc == 0:
                o, e = hmo_py.Encoder(*f, qp, lambda_override=lam), emu_py.EmuEncoder(*f, qp, lam=lam)
            else:
                o = hmo_py.Encoder(*f, qp, lambda_override=lam, search_range=sr, fast_search=1, ref=prev)
                e = emu_py.EmuEncoder(*f, qp, lam=lam, search_range=sr, fast_search=1, ref=prev)
            _emu_picture(e, o, True, ("ldp", poc))
            o.deblock()
            prev = [a.copy() for a in o.rec]
    _counted(lib, counts, run)


def test_every_case_of_the_level_choice_was_reached(counts):
    """The counters are those of the picture tests above, summed over the set (pytest keeps a module's tests in file order).
    Selected without all of them (-k, a node id), or after one of them failed, the sums are not those of the set: the test
    fails and says that, instead of reporting counters as missing."""
    assert counts["ran"] == N_PICTURE_TESTS, \
        "only %d of the %d picture tests ran to their end in this session: run the whole module" % (counts["ran"], N_PICTURE_TESTS)
    c = dict(zip(COUNTERS, counts["total"].tolist()))
    print(c)
    assert c.pop(MUST_BE_ZERO) == 0, "a remainder of 32768 or more: levels are clipped to 32767"
    missing = [k for k, v in c.items() if v == 0]
    assert not missing, missing
