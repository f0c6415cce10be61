"""WaveFrontSynchro on the MI355X: row chains decided in one launch (fcu_wpp_begin / fcu_compress_wpp), each row waiting for
the row above, against the test-side WPP reference (tests/wpp_oracle.py) -- every CTU, the reconstruction, the rows' coder
states -- plus the argument checks of the two entry points."""
import ctypes as C

import numpy as np
import pytest

import hmo_py
from wpp_oracle import wpp_oracle
from wpp_testlib import _compare, _poisoned

pytestmark = pytest.mark.gpu


def _run(pkg, Y, U, V, qp, **flags):
    eng = pkg.CuEngine(Y.shape[1], Y.shape[0], max_chains=(Y.shape[0] + 63) // 64)
    rec, out = _poisoned(eng, (Y, U, V))
    n, _, _ = eng.init_wpp_picture(0, (Y, U, V), qp, rec=rec, out=out, **flags)
    eng.compress_wpp(0, n)
    return eng, rec, out


@pytest.mark.parametrize("gen,w,h,qp", [("mixed", 256, 192, 22), ("textured", 64, 192, 37), ("smooth", 200, 136, 37),
                                        ("mixed", 136, 72, 22), ("textured", 256, 192, 37)])
def test_small_pictures_match_the_wpp_oracle(pkg, gen, w, h, qp):
    Y, U, V = getattr(pkg.synth, gen)(w, h, seed=9)
    o = wpp_oracle(Y, U, V, qp)
    eng, rec, out = _run(pkg, Y, U, V, qp)
    _compare(o, rec, out, f"{gen} {w}x{h} qp{qp}", eng, 0)
    eng.destroy()


@pytest.mark.parametrize("w,h", [(1920, 1080), (3840, 2160)])
def test_full_pictures_match_the_wpp_oracle(pkg, w, h):
    Y, U, V = pkg.synth.mixed(w, h, seed=21)
    o = wpp_oracle(Y, U, V, 32)
    eng, rec, out = _run(pkg, Y, U, V, 32)
    _compare(o, rec, out, f"{w}x{h}", eng, 0)
    eng.destroy()


def test_dependency_stress(pkg):
    """textured top rows, flat bottom rows: the bottom rows decide a CTU in a fraction of the time of the top ones and would
    overtake the rows above if a wait were missing"""
    w, h = 768, 640
    Y, U, V = pkg.synth.textured(w, h, seed=4)
    Y[192:] = 128
    U[96:] = 128
    V[96:] = 128
    o = wpp_oracle(Y, U, V, 27)
    eng, rec, out = _run(pkg, Y, U, V, 27)
    _compare(o, rec, out, "stress", eng, 0)
    eng.destroy()


def test_more_chains_than_resident(pkg):
    """256 pictures of 128x1088 (2 x 17 CTUs): 4352 row chains in one launch, more than the GPU keeps resident"""
    w, h, n_pics, seeds = 128, 1088, 256, 4
    srcs = [pkg.synth.mixed(w, h, seed=s) for s in range(seeds)]
    refs = [wpp_oracle(*s, 32) for s in srcs]
    rows = (h + 63) // 64
    eng = pkg.CuEngine(w, h, max_chains=n_pics * rows)
    assert n_pics * rows > 256 * max(1, eng.lib.fcu_chains_per_cu())
    pics = []
    for i in range(n_pics):
        rec, out = _poisoned(eng, srcs[i % seeds])
        eng.init_wpp_picture(i * rows, srcs[i % seeds], 32, rec=rec, out=out)
        pics.append((rec, out))
    assert eng.lib.fcu_compress_wpp(eng.h, 0, n_pics * rows, None) == 0, eng.lib.fcu_last_error().decode()
    for i, (rec, out) in enumerate(pics):
        _compare(refs[i % seeds], rec, out, f"picture {i}")
    eng.destroy()


def test_pictures_with_different_qps_in_one_launch(pkg):
    w, h, qps = 256, 192, (22, 32, 37)
    Y, U, V = pkg.synth.mixed(w, h, seed=13)
    rows = (h + 63) // 64
    eng = pkg.CuEngine(w, h, max_chains=len(qps) * rows)
    together = []
    for i, qp in enumerate(qps):
        rec, out = _poisoned(eng, (Y, U, V))
        eng.init_wpp_picture(i * rows, (Y, U, V), qp, rec=rec, out=out)
        together.append((rec, out))
    eng.compress_wpp(0, len(qps) * rows)
    for i, qp in enumerate(qps):                             # each picture alone, on the same chains
        rec, out = _poisoned(eng, (Y, U, V))
        eng.init_wpp_picture(0, (Y, U, V), qp, rec=rec, out=out)
        eng.compress_wpp(0, rows)
        assert np.array_equal(out.cpu().numpy(), together[i][1].cpu().numpy()), qp
        for p, q in zip(rec, together[i][0]):
            assert np.array_equal(p.cpu().numpy(), q.cpu().numpy()), qp
    _compare(wpp_oracle(Y, U, V, qps[1]), *together[1], "qp 32 of three")
    eng.destroy()


def test_decision_states_match_the_wpp_oracle(pkg):
    eng_mod = pkg.engine
    w, h, qp = 384, 256, 32
    Y, U, V = pkg.synth.mixed(w, h, seed=5)
    obf_o, _ = hmo_py.obf_prepass(Y)
    rows = (h + 63) // 64
    eng = pkg.CuEngine(w, h, max_chains=rows)
    obf_dev = eng.obf_prepass(Y)[0][0].contiguous()
    assert np.array_equal(obf_dev.cpu().numpy(), obf_o)

    def check(state, sw):
        o = wpp_oracle(Y, U, V, qp, decision=(state, obf_o, sw[0], sw[1], 0))
        rec, out = _poisoned(eng, (Y, U, V))
        eng.init_wpp_picture(0, (Y, U, V), qp, rec=rec, out=out)
        for r in range(rows):
            eng.set_decision(r, state, obf_dev, *sw)
        eng.compress_wpp(0, rows)
        _compare(o, rec, out, f"state {state}", eng, 0)
        return o

    o = check(eng_mod.VERIFYING, ((0, 0, 0, 0), (0, 0, 0, 0)))
    ver = eng.verify_counts(0, rows)
    assert np.array_equal(ver, o.verify) and ver[:, :4].sum() > 0
    check(eng_mod.TESTING, eng_mod.decision_switch(ver))
    check(eng_mod.TESTING, ((1, 1, 1, 1), (1, 1, 1, 1)))
    check(eng_mod.TRAINING, ((0, 0, 0, 0), (0, 0, 0, 0)))
    eng.destroy()


def test_sequence_decider_with_wpp(pkg):
    w, h, qp = 256, 192, 32
    srcs = [pkg.synth.mixed(w, h, seed=s) for s in (1, 2)]
    with pytest.raises(ValueError):
        pkg.sequence.SequenceDecider(w, h, qp, slice_ctus=4, wpp=True)
    dec = pkg.sequence.SequenceDecider(w, h, qp, fast=False, in_flight=2, wpp=True)
    res = dec.decide_group(srcs)
    for (Y, U, V), r in zip(srcs, res):
        o = wpp_oracle(Y, U, V, qp)
        o.enc.deblock()
        _compare(o, r["rec"], r["out"], f"POC {r['poc']} deblocked")
    dec.close()


def test_argument_checks(pkg):
    eng_mod = pkg.engine
    w, h = 192, 128
    Y, U, V = pkg.synth.mixed(w, h, seed=2)
    eng = pkg.CuEngine(w, h, max_chains=3)
    lib = eng.lib
    assert lib.fcu_wpp_rows(eng.h) == 2
    planes = [eng.torch.as_tensor(a).cuda() for a in (Y, U, V)]
    rec = [p.clone() for p in planes]
    out = eng.torch.zeros(eng.n_ctu * eng_mod.CTU_OUT_BYTES, dtype=eng.torch.uint8, device="cuda")
    ptrs = [p.data_ptr() for p in planes] + [p.data_ptr() for p in rec] + [out.data_ptr()]

    def begin(first, fp):
        return lib.fcu_wpp_begin(eng.h, first, C.byref(fp), *ptrs)

    fp = eng_mod.ldp_slice(32, 1)
    fp.slice_ctus = 0
    assert begin(0, fp) == -2                                # a P slice
    fp = eng_mod.FrameParams()
    lib.fcu_default_frame_params(C.byref(fp), 32)
    fp.slice_ctus = 3
    assert begin(0, fp) == -2                                # WPP with SliceMode 1
    fp.slice_ctus = 0
    assert begin(2, fp) == -2                                # too few chains left for two rows
    assert begin(0, fp) == 0
    assert lib.fcu_compress_chains(eng.h, 0, 2, 3, None) == -4       # row chains belong to fcu_compress_wpp
    assert lib.fcu_compress_ctu(eng.h, 0, 0, C.byref(eng_mod.CtuOut())) == -4
    assert lib.fcu_compress_wpp(eng.h, 1, 1, None) == -4     # not a whole picture
    eng.init_chain(2, (Y, U, V), 32)
    assert lib.fcu_compress_wpp(eng.h, 2, 1, None) == -4     # a plain chain
    assert lib.fcu_compress_wpp(eng.h, 0, 2, None) == 0
    assert lib.fcu_compress_wpp(eng.h, 0, 2, None) == -4     # already decided
    eng.destroy()
