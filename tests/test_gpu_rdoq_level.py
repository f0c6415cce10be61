"""The frames of tests/test_rdoq_level_emu.py (level_choice(): the level choice of RDOQ's first loop and the rates of its record
in one pass; uiMaxAbsLevel 1, 2 and more, lowered and zeroed levels, c1Idx >= 8, c2Idx >= 1, Rice parameter 0 to 4, remainders in
the escape branch, the inter RQT's calls) on the device against the oracle, every TComDataCU array and the reconstruction
bit-exact; and one picture through the WaveFrontSynchro kernel (fcu_ctu_engine_wpp)."""
import numpy as np
import pytest

import hmo_py
from rdoq_level_cases import INTRA_CASES, LDP_CLIP, frame, ldp_pictures
from test_gpu_parity import _compare_ctu
from wpp_oracle import wpp_oracle
from wpp_testlib import _compare, _poisoned

pytestmark = pytest.mark.gpu


def _same_picture(eng, ref, what):
    for a in range(eng.n_ctu):
        _compare_ctu(eng.ctu_out(0, a), ref.ctu_arrays(a), f"{what} ctu{a}")
    for p, q in zip(eng.rec_planes(0), ref.rec):
        assert np.array_equal(p, q), f"{what}: reconstruction"


@pytest.mark.parametrize("case", INTRA_CASES, ids=lambda c: "%s-%dx%d-qp%d" % c)
def test_intra_frames_match_oracle(pkg, case):
    src, w, h, qp = case
    f = frame(pkg, src, w, h)
    eng = pkg.CuEngine(w, h, max_chains=1)
    eng.init_chain(0, f, qp=qp)
    eng.compress_chains(0, 1, eng.n_ctu)
    eng.sync()
    ref = hmo_py.Encoder(*f, qp)
    ref.compress_frame()
    _same_picture(eng, ref, f"{src} {w}x{h} qp{qp}")
    eng.destroy()


def test_lowdelay_p_clip_matches_oracle(pkg):
    _, w, h, base_qp, _, _, sr = LDP_CLIP
    eng = pkg.CuEngine(w, h, max_chains=1)
    prev = None
    for poc, f in enumerate(ldp_pictures(pkg)):
        _, qp, lam = hmo_py.ldp_slice(poc, base_qp)
        fp = pkg.engine.ldp_slice(base_qp, poc)
        assert fp.qp == qp
        if poc == 0:
            ref = hmo_py.Encoder(*f, qp, lambda_override=lam)
            eng.init_chain(0, f, fp.qp, params=fp)
        else:
            fp.search_range, fp.fast_search = sr, 1
            ref = hmo_py.Encoder(*f, qp, lambda_override=lam, search_range=sr, fast_search=1, ref=prev)
            eng.init_chain(0, f, fp.qp, params=fp, ref=eng.pad_reference(prev))
        eng.compress_chains(0, 1, eng.n_ctu)
        eng.sync()
        ref.compress_frame()
        _same_picture(eng, ref, f"lowdelay_P picture {poc}")
        ref.deblock()
        prev = [a.copy() for a in ref.rec]
    eng.destroy()


def test_wpp_picture_matches_the_wpp_oracle(pkg):
    Y, U, V = pkg.synth.mixed(128, 128, seed=13)
    o = wpp_oracle(Y, U, V, 22)
    eng = pkg.CuEngine(128, 128, max_chains=2)
    rec, out = _poisoned(eng, (Y, U, V))
    n, _, _ = eng.init_wpp_picture(0, (Y, U, V), 22, rec=rec, out=out)
    eng.compress_wpp(0, n)
    _compare(o, rec, out, "mixed 128x128 qp22", eng, 0)
    eng.destroy()
