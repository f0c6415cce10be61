"""The register path of the 4x4 / 8x8 trials (pu_first_pass_batched) on the wave emulator: the engine as
shipped and the engine without the path (-DFCU_SMALL_TU_POOLS, every size through the candidate pools) must give the same
fcu_ctu_out, reconstruction and CABAC state, and both must equal the oracle.  The emulator's counters (fcu_emu_small_cnt, csrc/fcu_engine.h) say whether the frames reached the edge cases; they
are checked on the pool build first."""
import ctypes as C
import os

import numpy as np
import pytest

import hmo_py
from small_tu_cases import CASES, COUNTERS, frame

BUILDS = {"pools": "libfcu_emu_pools.so", "shipped": "libfcu_emu.so"}


def _load(name):
    """another build of the emulator with the prototypes emu_py.load() gives the shipped one"""
    import emu_py
    std = emu_py.load()
    if name == "libfcu_emu.so":
        return std
    lib = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(emu_py.__file__)), "emu", name))
    for k, f in list(vars(std).items()):
        if isinstance(f, std._FuncPtr):
            g = getattr(lib, k)
            g.argtypes, g.restype = f.argtypes, f.restype
    return lib


def _run(lib, Y, U, V, qp, monkeypatch):
    import emu_py
    monkeypatch.setattr(emu_py, "load", lambda: lib)
    e = emu_py.EmuEncoder(Y, U, V, qp)
    cnt = (C.c_ulonglong * len(COUNTERS)).in_dll(lib, "fcu_emu_small_cnt")
    before = np.array(list(cnt), dtype=np.int64)
    ctus, states = [], []
    for a in range(e.n_ctu):
        e.compress_ctu(a)
        ctus.append(e.ctu_arrays(a))
        states.append(e.cabac())
    counts = dict(zip(COUNTERS, (np.array(list(cnt), dtype=np.int64) - before).tolist()))
    return ctus, states, [p.copy() for p in e.rec], counts


@pytest.fixture(scope="module")
def runs(built, pkg):
    mp = pytest.MonkeyPatch()
    res = {}
    try:
        libs = {b: _load(n) for b, n in BUILDS.items()}
        for case in CASES:
            src, w, h, qp = case
            Y, U, V = frame(pkg, src, w, h)
            o = hmo_py.Encoder(Y, U, V, qp)
            ref_ctus, ref_states = [], []
            for a in range(o.n_ctu):
                o.compress_ctu(a)
                ref_ctus.append(o.ctu_arrays(a))
                ref_states.append(o.cabac())
            res[case] = {"oracle": (ref_ctus, ref_states, [p.copy() for p in o.rec], None)}
            for b, lib in libs.items():
                res[case][b] = _run(lib, Y, U, V, qp, mp)
    finally:
        mp.undo()
    return res


def _diff(A, B):
    bad = []
    for a, (x, y) in enumerate(zip(A[0], B[0])):
        bad += [(a, k) for k, v in x.items() if not (np.array_equal(v, y[k]) if isinstance(v, np.ndarray) else v == y[k])]
    bad += [(a, "cabac") for a, (x, y) in enumerate(zip(A[1], B[1])) if not (np.array_equal(x[0], y[0]) and x[1] == y[1])]
    bad += [("rec", i) for i, (p, q) in enumerate(zip(A[2], B[2])) if not np.array_equal(p, q)]
    return bad


@pytest.mark.parametrize("counter", COUNTERS)
def test_pool_build_reaches_the_edge_cases(runs, counter):
    """a transform-skip winner, a trial whose levels are all zero, a 4x4 batch of more than 16 variants, a chroma 4x4 trial"""
    total = sum(r["pools"][3][counter] for r in runs.values())
    print(counter, {k: r["pools"][3][counter] for k, r in runs.items()})
    assert total > 0


@pytest.mark.parametrize("counter", COUNTERS)
def test_shipped_build_reaches_the_edge_cases(runs, counter):
    assert sum(r["shipped"][3][counter] for r in runs.values()) == sum(r["pools"][3][counter] for r in runs.values()) > 0


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%dx%d-qp%d" % c)
def test_build_equals_the_oracle(runs, case, build):
    bad = _diff(runs[case]["oracle"], runs[case][build])
    assert not bad, bad


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%dx%d-qp%d" % c)
def test_register_path_equals_the_pool_path(runs, case):
    bad = _diff(runs[case]["pools"], runs[case]["shipped"])
    assert not bad, bad
