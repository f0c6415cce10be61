"""The frames of tests/test_small_tu_emu.py (4x4 / 8x8 trials: many and few levels, all-zero trials, picture-edge CUs, a
transform-skip winner, 4x4 batches of 17-20 variants) on the device against the oracle, every TComDataCU array and the
reconstruction bit-exact; and one picture through the WaveFrontSynchro kernel (fcu_ctu_engine_wpp)."""
import numpy as np
import pytest

import hmo_py
from small_tu_cases import CASES, frame
from test_gpu_parity import _compare_ctu
from wpp_oracle import wpp_oracle
from wpp_testlib import _compare, _poisoned

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%dx%d-qp%d" % c)
def test_small_tu_frames_match_oracle(pkg, case):
    src, w, h, qp = case
    f = frame(pkg, src, w, h)
    eng = pkg.CuEngine(w, h, max_chains=1)
    eng.init_chain(0, f, qp=qp)
    eng.compress_chains(0, 1, eng.n_ctu)
    eng.sync()
    ref = hmo_py.Encoder(*f, qp)
    ref.compress_frame()
    for a in range(eng.n_ctu):
        _compare_ctu(eng.ctu_out(0, a), ref.ctu_arrays(a), f"{src} {w}x{h} qp{qp} ctu{a}")
    for p, q in zip(eng.rec_planes(0), ref.rec):
        assert np.array_equal(p, q), f"{src} {w}x{h} qp{qp}: reconstruction"
    eng.destroy()


def test_wpp_picture_matches_the_wpp_oracle(pkg):
    Y, U, V = pkg.synth.textured(128, 128, seed=13)
    o = wpp_oracle(Y, U, V, 27)
    eng = pkg.CuEngine(128, 128, max_chains=2)
    rec, out = _poisoned(eng, (Y, U, V))
    n, _, _ = eng.init_wpp_picture(0, (Y, U, V), 27, rec=rec, out=out)
    eng.compress_wpp(0, n)
    _compare(o, rec, out, "textured 128x128 qp27", eng, 0)
    eng.destroy()
