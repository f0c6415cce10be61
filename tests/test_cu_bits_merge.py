"""Bits of a 2Nx2N intra candidate CU without the second walk (check_rd_cost_intra): the CU's coder, Q15 count and
bins are merged from the coder of the luma search's chosen walk and a chroma coder -- the chroma search's own when the CU has
one chroma leaf, a chroma-only walk in final order otherwise; NxN CUs keep the full walk.  The emulator is built a second time
with -DFCU_EMU_CHECK_CU_MERGE (tests/emu/cu_merge_emu.cpp): every merged CU is also walked, and bits, bins, Q15 count and all
context bytes must agree, on top of the always-on check that no context is moved by both searches.  Every case then asserts
emulator == oracle on all output fields, the reconstruction and the coder state, and that the content drove all three paths."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emu_py
import hmo_py
import search_trace as st
from test_rmd_ties import _flat, _tiles

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
LIB = os.path.join(EMU_DIR, "libfcu_emu_cu_merge.so")


@pytest.fixture(scope="module")
def check_lib(built, monkeypatch_module):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-shared", "-o", LIB, "cu_merge_emu.cpp"], cwd=EMU_DIR)
    std = emu_py.load()                                          # the plain emulator: its prototypes are this library's too
    lib = C.CDLL(LIB)
    for name in ("fcu_emu_create", "fcu_emu_destroy", "fcu_emu_compress_ctu", "fcu_emu_get_state", "fcu_emu_set_decision", "fcu_emu_get_verify",
                 "fcu_emu_tu_trials", "fcu_emu_set_p", "fcu_emu_set_lambda", "fcu_emu_get_state_full", "fcu_emu_set_rdoq", "fcu_emu_set_amp",
                 "fcu_emu_set_cabac_b", "fcu_emu_set_col"):
        f, g = getattr(std, name), getattr(lib, name)
        g.argtypes, g.restype = f.argtypes, f.restype
    lib.fcu_emu_cu_paths.argtypes = [C.c_void_p, C.c_int]
    monkeypatch_module.setattr(emu_py, "load", lambda: lib)
    return lib


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


def _paths(lib):
    v = (C.c_ulonglong * 3)()
    lib.fcu_emu_cu_paths(v, 1)
    return [int(x) for x in v]


def _same_ctu(o, e, a, full=False):
    A, B = o.ctu_arrays(a), e.ctu_arrays(a)
    for k, v in A.items():
        assert (np.array_equal(v, B[k]) if isinstance(v, np.ndarray) else v == B[k]), (a, k)
    (ca, fa), (cb, fb) = o.cabac(full=full), e.cabac(full=full)
    assert fa == fb, (a, "Q15 count")
    assert np.array_equal(ca[st.O_SORTED], cb[st.O_SORTED]) if full else np.array_equal(ca, cb), (a, "contexts")
    return A


# (picture, width, height, QP, tools or None for the defaults).  tools: transform_skip | ts_fast << 1 | sign_hiding << 2 | strong_smoothing << 3
INTRA_CASES = [
    ("textured", 128, 64, 22, None),      # the bench's kind of content: split trees, several chroma leaves
    ("textured", 128, 64, 37, None),
    ("mixed", 136, 72, 22, None),         # partial CTUs on both edges
    ("tiles", 136, 72, 37, None),         # flat 16x16 tiles: single leaves, zero cbf; partial CTUs
    ("flat", 128, 64, 22, None),
    ("textured", 64, 64, 22, 13),         # transform skip tried for every 4x4 TU
    ("textured", 64, 64, 37, 15),         # transform skip with TransformSkipFast
]


def _picture(pkg, gen, w, h):
    if gen == "flat":
        return _flat(w, h, 11)
    if gen == "tiles":
        return _tiles(w, h, 11)
    return getattr(pkg.synth, gen)(w, h, seed=5)


@pytest.mark.parametrize("gen,w,h,qp,tools", INTRA_CASES)
def test_intra_pictures_merged_bits_equal_walk_and_oracle(check_lib, pkg, gen, w, h, qp, tools):
    Y, U, V = _picture(pkg, gen, w, h)
    if tools is None:
        o, e = hmo_py.Encoder(Y, U, V, qp), emu_py.EmuEncoder(Y, U, V, qp)
    else:
        o = hmo_py.Encoder(Y, U, V, qp, transform_skip=tools & 1, transform_skip_fast=(tools >> 1) & 1, sign_hiding=(tools >> 2) & 1, strong_smoothing=(tools >> 3) & 1)
        e = emu_py.EmuEncoder(Y, U, V, qp, tools=tools)
    assert e.lib is check_lib
    _paths(check_lib)
    for a in range(o.n_ctu):
        o.compress_ctu(a)
        e.compress_ctu(a)
        _same_ctu(o, e, a)
    for p, q in zip(o.rec, e.rec):
        assert np.array_equal(p, q)
    own, rewalk, walked = _paths(check_lib)
    print("CUs merged with the search's chroma coder %d, merged with a chroma-only walk %d, walked %d" % (own, rewalk, walked))
    assert own > 0 and walked > 0                                # single chroma leaves everywhere; NxN at depth 3 is always walked
    assert own + rewalk > (own + rewalk + walked) / 2
    assert rewalk > 0                                            # a 64x64 CU always has four chroma leaves; textured content splits smaller trees too


def test_lowdelay_p_clip_with_intra_cus(check_lib, pkg):
    """Intra candidate CUs of P pictures: the luma walk carries skip flag and pred mode at part 0 (contexts of the appended
    inter range), the merge takes them with the luma group."""
    gen, w, h, base_qp, seed, n_pic, sr = "textured", 128, 64, 27, 3, 3, 8
    prev = None
    n_intra_p = 0
    _paths(check_lib)
    for poc in range(n_pic):
        f = st.moving_frame(pkg.synth, gen, w, h, seed, poc)
        if poc:                                                  # content the reference picture does not hold: the right CTU of every P picture
            n = st.moving_frame(pkg.synth, "mixed", w, h, seed + 7 * poc, poc)
            f = tuple(np.ascontiguousarray(np.concatenate([a[:, :a.shape[1] // 2], b[:, b.shape[1] // 2:]], axis=1)) for a, b in zip(f, n))
        _, qp, lam = hmo_py.ldp_slice(poc, base_qp)
        if poc == 0:
            o, e = hmo_py.Encoder(*f, qp, lambda_override=lam), emu_py.EmuEncoder(*f, qp, lam=lam)
        else:
            o = hmo_py.Encoder(*f, qp, lambda_override=lam, search_range=sr, fast_search=1, ref=prev)
            e = emu_py.EmuEncoder(*f, qp, lam=lam, search_range=sr, fast_search=1, ref=prev)
        for a in range(o.n_ctu):
            o.compress_ctu(a)
            e.compress_ctu(a)
            A = _same_ctu(o, e, a, full=True)
            if poc:
                n_intra_p += int((A["pred_mode"] == 1).sum())
        for p, q in zip(o.rec, e.rec):
            assert np.array_equal(p, q), (poc, "reconstruction")
        if poc == 0:
            _paths(check_lib)                                    # count the P pictures only
        o.deblock()
        prev = [a.copy() for a in o.rec]
    own, rewalk, walked = _paths(check_lib)
    print("P pictures: partitions decided intra %d; CUs merged %d + %d, walked %d" % (n_intra_p, own, rewalk, walked))
    assert n_intra_p > 0
    assert own > 0 and rewalk > 0 and walked > 0
