"""Group-ahead loads of the lane-private walks (rdoq<0>, code_coeff_body): the emulator against the oracle on
frames whose transform units meet the walks' edge cases, and a check -- by the emulator's own counters
(fcu_emu_walk_cnt, csrc/fcu_engine.h) -- that each edge case was really reached.  The emulator aborts (FCU_CHECK_LSCAN) when
a group load of rdoq<0> forms an address outside the pool it reads (Scratch::p_lscan)."""
import ctypes as C

import numpy as np
import pytest

import hmo_py
from walk_prefetch_cases import CASES, frame

NAMES = ["rdoq_calls", "rdoq_top_is_group0", "rdoq_ahead_groups", "rdoq_only_group0", "rdoq_only_last_group", "rdoq_all_zero",
         "bits_calls", "bits_one_empty_run_between", "bits_second_round"]


@pytest.fixture(scope="module")
def runs(built, pkg):
    """every case once: the mismatches against the oracle and what the walks counted"""
    import emu_py
    lib = emu_py.load()
    cnt = (C.c_ulonglong * len(NAMES)).in_dll(lib, "fcu_emu_walk_cnt")
    res = {}
    for case in CASES:
        src, w, h, qp = case
        Y, U, V = frame(pkg, src, w, h)
        o = hmo_py.Encoder(Y, U, V, qp)
        e = emu_py.EmuEncoder(Y, U, V, qp)
        before = np.array(list(cnt), dtype=np.int64)
        bad = []
        for a in range(o.n_ctu):
            o.compress_ctu(a)
            e.compress_ctu(a)
            A, B = o.ctu_arrays(a), e.ctu_arrays(a)
            for k, v in A.items():
                if not (np.array_equal(v, B[k]) if isinstance(v, np.ndarray) else v == B[k]):
                    bad.append((a, k))
            ca, fa = o.cabac()
            cb, fb = e.cabac()
            if not (np.array_equal(ca, cb) and fa == fb):
                bad.append((a, "cabac"))
        for i, (p, q) in enumerate(zip(o.rec, e.rec)):
            if not np.array_equal(p, q):
                bad.append(("rec", i))
        res[case] = (bad, dict(zip(NAMES, (np.array(list(cnt), dtype=np.int64) - before).tolist())))
    return res


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%dx%d-qp%d" % c)
def test_emulator_is_bit_exact(runs, case):
    bad, counts = runs[case]
    print(case, counts)
    assert not bad, bad


def _total(runs, name, source=None):
    return sum(c[name] for k, (_, c) in runs.items() if source is None or k[0] == source)


def test_walks_ran_with_group_ahead_loads(runs):
    assert _total(runs, "rdoq_ahead_groups") > 0 and _total(runs, "bits_calls") > 0


def test_only_level_in_group_0_is_reached(runs):
    """no successor group: rdoq<0> starts in group 0, or ends with its last level there"""
    assert _total(runs, "rdoq_top_is_group0") > 0 and _total(runs, "rdoq_only_group0") > 0


def test_only_level_in_last_group_is_reached(runs):
    assert _total(runs, "rdoq_only_last_group") > 0


def test_all_zero_tu_is_reached(runs):
    """RDOQ leaves before its first load; the bit counter is not called for such a TU (its callers test the cbf)"""
    assert _total(runs, "rdoq_all_zero", "flat") > 0 and _total(runs, "bits_calls", "flat") == 0


def test_one_empty_run_between_non_empty_ones_is_reached(runs):
    """a 32x32 TU whose levels leave exactly one 128-byte run empty between two non-empty ones"""
    assert _total(runs, "bits_one_empty_run_between") > 0


def test_second_bit_count_round_is_reached(runs):
    """a 4x4 PU with 17-20 candidate variants"""
    assert _total(runs, "bits_second_round") > 0
