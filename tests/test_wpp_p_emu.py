"""The engine source's WaveFrontSynchro row chains of P pictures on the CPU wave emulator (tests/emu/wpp_p_emu.cpp) against the
P-slice WPP reference (tests/wpp_oracle_p.py): every fcu_ctu_out field, the reconstruction, each row's final coder state and
the search state (m_integerMv2Nx2N) each row ends with, in all four slots; the emulator's read-before-write count of the TZ
start vectors stays zero."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emu_py
import hmo_py
import search_trace as st
from test_wpp_p_oracle import split_motion_clip
from wpp_oracle_p import wpp_p_clip

EMU = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="session")
def wpp_p_emu(built):
    """tests/emu/libwpp_p_emu.so, built with the g++ flags build() gives the other emulators"""
    so, src = os.path.join(EMU, "libwpp_p_emu.so"), os.path.join(EMU, "wpp_p_emu.cpp")
    csrc = os.path.join(ROOT, "fast-cu-decision-hevc_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")] + [os.path.join(ROOT, "include", "fcu.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-shared", "-o", "libwpp_p_emu.so", "wpp_p_emu.cpp"], cwd=EMU)
    lib = C.CDLL(so)
    lib.wpp_p_emu_create.restype = C.c_void_p
    lib.wpp_p_emu_create.argtypes = [C.c_int] * 3 + [C.c_double] + [C.c_int] * 4 + [C.c_void_p] * 7 + \
        [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    lib.wpp_p_emu_destroy.argtypes = [C.c_void_p]
    lib.wpp_p_emu_rows.argtypes = [C.c_void_p]
    lib.wpp_p_emu_run.argtypes = [C.c_void_p]
    lib.wpp_p_emu_set_decision.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.wpp_p_emu_get_state_full.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.wpp_p_emu_get_search_state.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.wpp_p_emu_read_before_write.argtypes = [C.c_void_p]
    return lib


def emulate_picture(lib, f, qp, lam, refs, ref_pocs, poc, col_ref_pocs, col, int_mv, sr, fast, amp, btab, decision=None, row0_known=1):
    """one P picture through the emulated row chains; returns (out Ctu array, rec planes, per-row (ctx, frac), per-row search
    state, read-before-write count)"""
    h, w = f[0].shape
    org = [np.ascontiguousarray(a) for a in f]
    rec = [np.full_like(a, 0x5A) for a in org]                # poisoned
    n_ctu = ((w + 63) // 64) * ((h + 63) // 64)
    out = (hmo_py.Ctu * n_ctu)()
    C.memset(out, 0xA5, C.sizeof(out))
    pads = [emu_py.pad_planes([np.ascontiguousarray(a) for a in r]) for r in refs]
    ptrs = (C.c_void_p * (3 * len(refs)))(*[a.ctypes.data for p in pads for a in p])
    pocs = np.ascontiguousarray(ref_pocs, np.int32)
    crp = np.ascontiguousarray(col_ref_pocs, np.int32)
    colbuf = None if col is None else np.frombuffer(bytes(col), np.uint8).copy()
    mv = np.ascontiguousarray([v for p in int_mv for v in p], np.int32)
    hd = lib.wpp_p_emu_create(w, h, qp, lam, sr, fast, amp, btab, *[a.ctypes.data for a in org], *[a.ctypes.data for a in rec], C.addressof(out),
                              len(refs), ptrs, pocs.ctypes.data, poc, crp.ctypes.data, len(crp),
                              None if colbuf is None else colbuf.ctypes.data, mv.ctypes.data, row0_known)
    try:
        rows = lib.wpp_p_emu_rows(hd)
        if decision is not None:
            obf16 = np.ascontiguousarray(decision[1], np.int16)
            sk, te = np.array(decision[2], np.uint8), np.array(decision[3], np.uint8)
            lib.wpp_p_emu_set_decision(hd, decision[0], sk.ctypes.data, te.ctypes.data, decision[4], obf16.ctypes.data)
        assert lib.wpp_p_emu_run(hd) == rows
        states, mvs = [], []
        for r in range(rows):
            ctx, frac = np.zeros(176, np.uint8), C.c_uint64(0)
            lib.wpp_p_emu_get_state_full(hd, r, ctx.ctypes.data, C.byref(frac))
            states.append((ctx, frac.value))
            xy = np.zeros(8, np.int32)
            lib.wpp_p_emu_get_search_state(hd, r, xy.ctypes.data)
            mvs.append([(int(xy[2 * k]), int(xy[2 * k + 1])) for k in range(4)])
        return out, rec, states, mvs, lib.wpp_p_emu_read_before_write(hd)
    finally:
        lib.wpp_p_emu_destroy(hd)


# gen, w, h, base_qp, n_pic, search range, TZ, references (rps), TMVP, AMP, cabac_b_table
CASES = [
    ("shear_mixed", 256, 112, 30, 3, 16, 1, (2, "recent"), 1, 1, 0),     # partial bottom row (48 high), two references
    ("mixed", 192, 176, 32, 4, 16, 1, (4, "hm"), 0, 0, 1),              # the cfg's reference sets, B tables, partial bottom row
    ("textured", 192, 128, 27, 3, 8, 0, (1, "hm"), 1, 0, 0),            # full search: no slot is ever written
    ("mixed", 192, 48, 30, 4, 16, 1, (1, "hm"), 1, 1, 0),               # one partial row: the search state crosses pictures only
    ("shear_textured", 56, 136, 30, 3, 16, 1, (2, "recent"), 0, 1, 0),  # 56 wide: every row begins on a boundary CTU
]


def _run_case(pkg, wpp_p_emu, gen, w, h, base_qp, n_pic, sr, fast, nref_rps, tmvp, amp, btab, decision=None, frames=None):
    nref, rps = nref_rps
    if frames is None:
        frames = [st.moving_frame(pkg.synth, gen, w, h, 7, poc) for poc in range(n_pic)]
    res = wpp_p_clip(frames, base_qp, ref_pocs=lambda poc, n: pkg.lowdelay.ref_pocs(poc, n, rps), n_refs=nref, search_range=sr,
                     fast_search=fast, tmvp=tmvp, amp=amp, cabac_b_table=btab, decision=decision)
    int_mv = [(0, 0)] * 4
    n_inter = 0
    for poc in range(1, n_pic):
        R, prev = res[poc], res[poc - 1]
        o = R["o"]
        _, qp, lam = hmo_py.ldp_slice(poc, base_qp)
        if nref > 1:
            rl = R["ref_pocs"]
            refs, pocs, crp = [res[q]["rec"] for q in rl], rl, res[rl[0]]["ref_pocs"] or [rl[0] - 1]
            cur = poc
        else:
            refs, pocs, crp, cur = [prev["rec"]], [0], [-1], 1       # fcu_chain_set_reference: one picture at POC distance 1
        out, rec, states, mvs, rbw = emulate_picture(wpp_p_emu, frames[poc], qp, lam, refs, pocs, cur, crp, prev["ctus"] if tmvp else None,
                                                     int_mv, sr, fast, amp, btab, decision)
        assert rbw == 0, (poc, "a TZ search read a start vector the row had neither written nor inherited")
        for a in range(o.enc.n_ctu):
            A = o.enc.ctu_arrays(a)
            c = out[a]
            for k, v in A.items():
                g = getattr(c, k)
                g = np.ctypeslib.as_array(g) if hasattr(g, "_length_") else g
                assert np.array_equal(v, g) if isinstance(v, np.ndarray) else v == g, (poc, a, k)
            n_inter += int((A["pred_mode"] == 0).sum())
        for p, q in zip(R["rec_unfiltered"], rec):
            assert np.array_equal(p, q), (poc, "reconstruction")
        for r in range(o.H):
            assert np.array_equal(states[r][0][st.O_SORTED], o.row_state[r][0][st.O_SORTED]) and states[r][1] == o.row_state[r][1], (poc, r, "coder state")
            assert mvs[r] == o.row_int_mv[r], (poc, r, "search state after the row")
        int_mv = mvs[-1]                                            # the last row's state: the next picture's row 0
        assert int_mv == R["int_mv"]
    assert n_inter > 0
    return res


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}_{c[1]}x{c[2]}_ref{c[7][0]}_tz{c[6]}" for c in CASES])
def test_emulated_wpp_p_rows_are_bit_exact(wpp_p_emu, pkg, case):
    _run_case(pkg, wpp_p_emu, *case)


@pytest.mark.parametrize("w,h,still,nref", [(256, 112, (0, 0, 128, 64), 2), (192, 48, None, 1)])
def test_emulated_wpp_p_rows_on_the_hand_off_fixtures(wpp_p_emu, pkg, w, h, still, nref):
    """the clips of tests/test_wpp_p_oracle.py whose decisions depend on the search state carried into the bottom row / into
    a picture"""
    frames = split_motion_clip(w, h, 3, 5 if still else 3, still=still)
    _run_case(pkg, wpp_p_emu, "split", w, h, 30, 3, 64, 1, (nref, "recent"), 0, 1 if still else 0, 0, frames=frames)


def test_emulated_wpp_p_rows_in_the_testing_state(wpp_p_emu, pkg):
    """the fork's Testing state with every switch on (Skip2Nx2N drops intra only, so the depth-0 searches still run)"""
    gen, w, h = "shear_mixed", 192, 112
    obf, _ = hmo_py.obf_prepass(st.moving_frame(pkg.synth, gen, w, h, 7, 1)[0])
    decision = (hmo_py.TESTING, obf, (1, 1, 1, 1), (1, 1, 1, 1), 1)
    _run_case(pkg, wpp_p_emu, gen, w, h, 32, 2, 16, 1, (1, "hm"), 0, 0, 0, decision=decision)


def test_read_before_write_count_fires(wpp_p_emu, pkg):
    """the count is live: a 48-high picture has no full CTU, so its TZ searches read start vectors they did not write, and a
    row 0 whose start state is declared unknown shows them"""
    gen, w, h, base_qp = "mixed", 128, 48, 30
    frames = [st.moving_frame(pkg.synth, gen, w, h, 7, poc) for poc in range(2)]
    res = wpp_p_clip(frames, base_qp, search_range=16)
    _, qp, lam = hmo_py.ldp_slice(1, base_qp)
    args = (wpp_p_emu, frames[1], qp, lam, [res[0]["rec"]], [0], 1, [-1], None, [(0, 0)] * 4, 16, 1, 0, 0)
    assert emulate_picture(*args)[4] == 0
    assert emulate_picture(*args, row0_known=0)[4] > 0
