"""rdoq_wave's passes after the walk on lane registers (4x4 / 8x8 blocks) and sign hiding on the wave (every size):
the shipped emulator and the emulator built with -DFCU_EMU_CHECK_RDOQ_TAIL (tests/emu/rdoq_tail_emu.cpp: every rdoq_wave call
also runs rdoq_finish() serially on what the pool form stores and aborts on a difference) against the oracle, on every
fcu_ctu_out array, the reconstruction and the CABAC state; and a check -- by the emulator's counters (fcu_emu_tail_cnt,
csrc/fcu_engine.h) -- that the frames reach every case of those passes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emu_py
import hmo_py
from rdoq_tail_cases import COUNTERS, INTRA_CASES, LDP_CLIP, MUST_BE_ZERO, frame, ldp_pictures

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
LIB = os.path.join(EMU_DIR, "libfcu_emu_rdoq_tail.so")
PROTOS = ("fcu_emu_create", "fcu_emu_destroy", "fcu_emu_compress_ctu", "fcu_emu_get_state", "fcu_emu_set_decision", "fcu_emu_get_verify",
          "fcu_emu_tu_trials", "fcu_emu_set_p", "fcu_emu_set_lambda", "fcu_emu_get_state_full", "fcu_emu_set_rdoq", "fcu_emu_set_amp",
          "fcu_emu_set_cabac_b", "fcu_emu_set_col")


@pytest.fixture(scope="module")
def libs(built):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-shared", "-o", LIB, "rdoq_tail_emu.cpp"], cwd=EMU_DIR)
    std = emu_py.load()
    chk = C.CDLL(LIB)
    for name in PROTOS:                                          # the plain emulator's prototypes are the check build's too
        f, g = getattr(std, name), getattr(chk, name)
        g.argtypes, g.restype = f.argtypes, f.restype
    return {"shipped": std, "check": chk}


def _oracle_picture(o, full):
    """one picture on the oracle, CTU by CTU: arrays and coder state after every CTU, the reconstruction at the end"""
    per_ctu = []
    for a in range(o.n_ctu):
        o.compress_ctu(a)
        per_ctu.append((o.ctu_arrays(a), o.cabac(full=full)))
    return per_ctu, [p.copy() for p in o.rec]


@pytest.fixture(scope="module")
def oracle(pkg, built):
    """the reference of every case, computed once"""
    res = {}
    for case in INTRA_CASES:
        src, w, h, qp = case
        res[case] = _oracle_picture(hmo_py.Encoder(*frame(pkg, src, w, h), qp), False)
    _, _, _, base_qp, _, _, sr = LDP_CLIP
    clip, prev = [], None
    for poc, f in enumerate(ldp_pictures(pkg)):
        _, qp, lam = hmo_py.ldp_slice(poc, base_qp)
        o = hmo_py.Encoder(*f, qp, lambda_override=lam) if poc == 0 else hmo_py.Encoder(*f, qp, lambda_override=lam, search_range=sr, fast_search=1, ref=prev)
        per_ctu, rec = _oracle_picture(o, True)
        clip.append((f, qp, lam, prev, per_ctu, rec))
        o.deblock()
        prev = [a.copy() for a in o.rec]
    res["ldp"] = clip
    return res


def _emu_picture(e, per_ctu, rec, full, what):
    import search_trace as st
    for a, (A, (ca, fa)) in enumerate(per_ctu):
        e.compress_ctu(a)
        B = e.ctu_arrays(a)
        for k, v in A.items():
            assert (np.array_equal(v, B[k]) if isinstance(v, np.ndarray) else v == B[k]), (what, a, k)
        cb, fb = e.cabac(full=full)
        assert fa == fb, (what, a, "Q15 count")
        assert np.array_equal(ca[st.O_SORTED], cb[st.O_SORTED]) if full else np.array_equal(ca, cb), (what, a, "contexts")
    for p, q in zip(rec, e.rec):
        assert np.array_equal(p, q), (what, "reconstruction")


N_PICTURE_TESTS = len(INTRA_CASES) + 1                          # per build: the intra frames and the clip


@pytest.fixture(scope="module")
def counts(libs):
    """per build: what the picture tests of this session counted, and how many of them ran"""
    return {b: {"total": np.zeros(len(COUNTERS), np.int64), "ran": 0} for b in ("shipped", "check")}


def _counted(lib, acc, run):
    cnt = (C.c_ulonglong * len(COUNTERS)).in_dll(lib, "fcu_emu_tail_cnt")
    before = np.array(list(cnt), dtype=np.int64)
    run()
    d = np.array(list(cnt), dtype=np.int64) - before
    acc["total"] += d
    acc["ran"] += 1
    print(dict(zip(COUNTERS, d.tolist())))


@pytest.mark.parametrize("build", ["shipped", "check"])
@pytest.mark.parametrize("case", INTRA_CASES, ids=lambda c: "%s-%dx%d-qp%d" % c)
def test_intra_frames_are_bit_exact(libs, oracle, counts, pkg, monkeypatch, case, build):
    monkeypatch.setattr(emu_py, "load", lambda: libs[build])
    src, w, h, qp = case
    per_ctu, rec = oracle[case]
    e = emu_py.EmuEncoder(*frame(pkg, src, w, h), qp)
    assert e.lib is libs[build]
    _counted(libs[build], counts[build], lambda: _emu_picture(e, per_ctu, rec, False, case))


@pytest.mark.parametrize("build", ["shipped", "check"])
def test_lowdelay_p_clip_is_bit_exact(libs, oracle, counts, monkeypatch, build):
    monkeypatch.setattr(emu_py, "load", lambda: libs[build])
    sr = LDP_CLIP[6]

    def run():
        for poc, (f, qp, lam, prev, per_ctu, rec) in enumerate(oracle["ldp"]):
            e = emu_py.EmuEncoder(*f, qp, lam=lam) if poc == 0 else emu_py.EmuEncoder(*f, qp, lam=lam, search_range=sr, fast_search=1, ref=prev)
            _emu_picture(e, per_ctu, rec, True, ("ldp", poc))
    _counted(libs[build], counts[build], run)


@pytest.mark.parametrize("build", ["shipped", "check"])
def test_every_case_of_the_tail_passes_was_reached(counts, build):
    """The counters are those of the picture tests above, summed over the set (pytest keeps a module's tests in file order).
    Selected without all of them (-k, a node id), or after one of them failed, the sums are not those of the set: the test
    fails and says that, instead of reporting counters as missing."""
    assert counts[build]["ran"] == N_PICTURE_TESTS, \
        "only %d of the %d picture tests of the %s build ran to their end in this session: run the whole module" % (counts[build]["ran"], N_PICTURE_TESTS, build)
    c = dict(zip(COUNTERS, counts[build]["total"].tolist()))
    print(build, c)
    assert c.pop(MUST_BE_ZERO) == 0, "a group without a position of finite sign-hiding cost: rdoq_wave gives that case no meaning"
    missing = [k for k, v in c.items() if v == 0]
    assert not missing, missing
