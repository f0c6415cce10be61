"""Properties of the test-side WaveFrontSynchro reference (tests/wpp_oracle.py) on the unchanged oracle."""
import ctypes as C

import numpy as np
import pytest

import hmo_py
from wpp_oracle import wpp_oracle


def _reset_state(qp):
    """the slot after resetEntropy of an I slice: 176 contexts, Q15 counter 0"""
    c = hmo_py.Cabac()
    lib = hmo_py.load()
    lib.hmo_cabac_init_tab.restype = None
    lib.hmo_cabac_init_tab.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.hmo_cabac_init_tab(C.addressof(c), qp, hmo_py.SLICE_I, 0)
    return np.ctypeslib.as_array(c.ctx).copy(), int(c.frac)


@pytest.mark.parametrize("gen,w,h,qp", [("mixed", 256, 192, 32), ("textured", 200, 136, 37)])
def test_row_zero_is_the_plain_one_slice_run(built, pkg, gen, w, h, qp):
    Y, U, V = getattr(pkg.synth, gen)(w, h, seed=11)
    o = wpp_oracle(Y, U, V, qp)
    ref = hmo_py.Encoder(Y, U, V, qp)
    for a in range(o.W):
        ref.compress_ctu(a)
        A, B = ref.ctu_arrays(a), o.enc.ctu_arrays(a)
        for k, v in A.items():
            assert np.array_equal(v, B[k]) if isinstance(v, np.ndarray) else v == B[k], (a, k)
    assert np.array_equal(ref.cabac(full=True)[0], o.row_state[0][0]) and ref.cabac(full=True)[1] == o.row_state[0][1]


@pytest.mark.parametrize("gen,w,h,qp", [("mixed", 256, 192, 32), ("smooth", 136, 72, 22), ("textured", 64, 192, 37)])
def test_row_starts_take_the_synchronised_contexts(built, pkg, gen, w, h, qp):
    Y, U, V = getattr(pkg.synth, gen)(w, h, seed=3)
    o = wpp_oracle(Y, U, V, qp)
    reset_ctx, reset_frac = _reset_state(qp)
    assert reset_frac == 0
    for r in range(1, o.H):
        ctx, frac = o.row_start[r]
        assert frac == 0, r                                  # TEncBinCABAC::start: the counter is not carried over
        if o.W >= 2:
            assert np.array_equal(ctx, np.frombuffer(o.saved[r - 1], np.uint8)), r
            assert not np.array_equal(ctx, reset_ctx)       # the sync really took something
        else:
            assert np.array_equal(ctx, reset_ctx), r         # no above-right CTU: the plain reset


@pytest.mark.parametrize("w,h", [(256, 192), (64, 192)])
def test_wpp_changes_the_decisions(built, pkg, w, h):
    """the restarts at the row starts are visible: some CTU or the final state differs from the run without WPP"""
    Y, U, V = pkg.synth.mixed(w, h, seed=5)
    o = wpp_oracle(Y, U, V, 32)
    ref = hmo_py.Encoder(Y, U, V, 32)
    ref.compress_frame()
    differs = any(ref.ctu(a).total_bits != o.enc.ctu(a).total_bits or ref.ctu(a).total_cost != o.enc.ctu(a).total_cost
                  for a in range(ref.n_ctu))
    assert differs
