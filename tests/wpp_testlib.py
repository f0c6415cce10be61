"""What the WaveFrontSynchro tests share: the ctypes binding of the emulator driver (tests/emu/wpp_emu.cpp, built by
__graft_entry__.build()), one picture through its row chains, and the comparisons of a decided picture with the reference
(tests/wpp_oracle.py) on the emulator and on the GPU."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import emu_py
import hmo_py
import search_trace as st

CTU_DT = np.dtype(hmo_py.Ctu)
TOOLS = 0b1011        # transform skip + its fast variant, no sign hiding, strong intra smoothing

_P = C.c_void_p
SIGNATURES = {
    "slice_rule": ([C.c_int] * 3, C.c_int),
    "create": ([C.c_int] * 6 + [_P] * 7 + [C.c_int, C.c_double] + [C.c_int] * 4 + [_P, _P, C.c_int, _P, C.c_int, _P, _P, C.c_int], _P),
    "destroy": ([_P], None), "rows": ([_P], C.c_int), "run": ([_P], C.c_int), "slice_ctus": ([_P], C.c_int), "read_before_write": ([_P], C.c_int),
    "above": ([_P, C.c_int], C.c_int),
    "set_decision": ([_P, C.c_int, _P, _P, C.c_int, _P], None),
    "get_state_full": ([_P, C.c_int, _P, _P], None), "get_verify": ([_P, _P], None), "get_search_state": ([_P, C.c_int, _P], None),
}
I_PICTURE = [0, 0.0, 0, 0, 0, 0, None, None, 0, None, 0, None]      # create's arguments from n_ref to col


@functools.lru_cache(maxsize=None)
def load_emu():
    lib = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu", "libwpp_emu.so"))
    for name, (argtypes, restype) in SIGNATURES.items():
        f = getattr(lib, "wpp_emu_" + name)
        f.argtypes, f.restype = argtypes, restype
    return lib


@pytest.fixture(scope="session")
def wpp_emu(built):
    return load_emu()


def flags_of(tools):
    """hmo_py.Encoder's tool flags of the emulator's `tools` bits (-1: the defaults)"""
    return {} if tools < 0 else dict(transform_skip=tools & 1, transform_skip_fast=(tools >> 1) & 1, sign_hiding=(tools >> 2) & 1, strong_smoothing=(tools >> 3) & 1)


def emulate(lib, f, qp, slice_rows=0, tools=-1, decision=None, p=None, fp_slice_ctus=0, int_mv=None, start_known=1):
    """One picture through the emulated row chains.  slice_rows 0: one slice.  p: None (I picture) or a dict lam, sr, fast, amp,
    btab, refs, ref_pocs, poc, col_ref_pocs, col; int_mv: the search state row 0 of a one-slice P picture starts from.
    Returns a dict: out (Ctu array), rec, states [(ctx, frac)] per row, mvs per row, rbw, verify, above."""
    h, w = f[0].shape
    org = [np.ascontiguousarray(a) for a in f]
    rec = [np.full_like(a, 0x5A) for a in org]                # poisoned
    W, H = (w + 63) // 64, (h + 63) // 64
    out = (hmo_py.Ctu * (W * H))()
    C.memset(out, 0xA5, C.sizeof(out))
    pargs = I_PICTURE
    if p is not None:
        pads = [emu_py.pad_planes([np.ascontiguousarray(a) for a in r]) for r in p["refs"]]
        ptrs = (C.c_void_p * (3 * len(pads)))(*[a.ctypes.data for q in pads for a in q])
        pocs = np.ascontiguousarray(p["ref_pocs"], np.int32)
        crp = np.ascontiguousarray(p["col_ref_pocs"], np.int32)
        colbuf = None if p["col"] is None else np.frombuffer(bytes(p["col"]), np.uint8).copy()
        pargs = [len(pads), p["lam"], p["sr"], p["fast"], p["amp"], p["btab"], ptrs, pocs.ctypes.data, p["poc"], crp.ctypes.data, len(crp),
                 None if colbuf is None else colbuf.ctypes.data]
    mv = None if int_mv is None else np.ascontiguousarray([v for xy in int_mv for v in xy], np.int32)
    hd = lib.wpp_emu_create(w, h, qp, slice_rows, fp_slice_ctus, tools, *[a.ctypes.data for a in org], *[a.ctypes.data for a in rec], C.addressof(out), *pargs,
                            None if mv is None else mv.ctypes.data, start_known)
    assert hd, "the binder refused valid arguments"
    try:
        assert lib.wpp_emu_rows(hd) == H and lib.wpp_emu_slice_ctus(hd) == slice_rows * W
        above = [lib.wpp_emu_above(hd, r) for r in range(H)]
        assert above == [-1 if r % (slice_rows or H) == 0 else r - 1 for r in range(H)]      # a row that starts a slice waits on nothing
        if decision is not None:
            obf16 = np.ascontiguousarray(decision[1], np.int16)
            sk, te = np.array(decision[2], np.uint8), np.array(decision[3], np.uint8)
            lib.wpp_emu_set_decision(hd, decision[0], sk.ctypes.data, te.ctypes.data, decision[4], obf16.ctypes.data)
        assert lib.wpp_emu_run(hd) == H
        states, mvs = [], []
        for r in range(H):
            ctx, frac = np.zeros(176, np.uint8), C.c_uint64(0)
            lib.wpp_emu_get_state_full(hd, r, ctx.ctypes.data, C.byref(frac))
            states.append((ctx, frac.value))
            xy = np.zeros(8, np.int32)
            lib.wpp_emu_get_search_state(hd, r, xy.ctypes.data)
            mvs.append([(int(xy[2 * k]), int(xy[2 * k + 1])) for k in range(4)])
        v = np.zeros((4, 6), np.float64)
        lib.wpp_emu_get_verify(hd, v.ctypes.data)
        return dict(out=out, rec=rec, states=states, mvs=mvs, rbw=lib.wpp_emu_read_before_write(hd), verify=v, above=above)
    finally:
        lib.wpp_emu_destroy(hd)


def assert_ctus_equal(enc, out, tag=()):
    """every fcu_ctu_out field of every CTU; returns the number of inter partitions"""
    n_inter = 0
    for a in range(enc.n_ctu):
        A = enc.ctu_arrays(a)
        c = out[a]
        for k, v in A.items():
            g = getattr(c, k)
            g = np.ctypeslib.as_array(g) if hasattr(g, "_length_") else g
            assert np.array_equal(v, g) if isinstance(v, np.ndarray) else v == g, tag + (a, k)
        n_inter += int((A["pred_mode"] == 0).sum())
    return n_inter


def p_picture_args(res, poc, base_qp, nref, sr, fast, tmvp, amp, btab):
    """the emulator's / engine's arguments of picture poc >= 1 of a clip decided by wpp_oracle.wpp_p_clip"""
    R_, prev = res[poc], res[poc - 1]
    _, qp, lam = hmo_py.ldp_slice(poc, base_qp)
    if nref > 1:
        rl = R_["ref_pocs"]
        refs, pocs, crp, cur = [res[q]["rec"] for q in rl], rl, res[rl[0]]["ref_pocs"] or [rl[0] - 1], poc
    else:
        refs, pocs, crp, cur = [prev["rec"]], [0], [-1], 1       # fcu_chain_set_reference: one picture at POC distance 1
    return qp, dict(lam=lam, sr=sr, fast=fast, amp=amp, btab=btab, refs=refs, ref_pocs=pocs, poc=cur, col_ref_pocs=crp, col=prev["ctus"] if tmvp else None)


# ---- on the GPU
def _poisoned(eng, planes):
    torch = eng.torch
    dev = torch.device("cuda", eng.device)
    rec = [torch.full(tuple(p.shape), 0x5A, dtype=torch.uint8, device=dev) for p in planes]
    out = torch.full((eng.n_ctu * C.sizeof(hmo_py.Ctu),), 0xA5, dtype=torch.uint8, device=dev)
    return rec, out


def _compare_ctus(got_bytes, want_bytes, what, n=None):
    got, want = np.frombuffer(got_bytes, CTU_DT)[:n], np.frombuffer(want_bytes, CTU_DT)[:n]
    assert len(got) == len(want) and len(got) > 0
    for name in CTU_DT.names:
        bad = np.nonzero([not np.array_equal(a, b) for a, b in zip(got[name], want[name])])[0]
        assert bad.size == 0, f"{what}: field {name} differs at CTU {bad[:8].tolist()}"


def _compare(o, rec, out, what, eng=None, first=None, sorted_ctx=False):
    _compare_ctus(out.cpu().numpy().tobytes(), o.enc.all_ctus_bytes(), what)
    for p, q in zip(rec, o.enc.rec):
        assert np.array_equal(p.cpu().numpy(), q), what
    if eng is not None:
        sel = st.O_SORTED if sorted_ctx else slice(None)
        for r in range(o.H):
            ctx, frac = eng.ctx_state(first + r, full=True)
            assert np.array_equal(ctx[sel], o.row_state[r][0][sel]) and frac == o.row_state[r][1], f"{what}: row {r} coder state"
            assert eng.position(first + r) == (r + 1) * o.W
