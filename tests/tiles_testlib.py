"""What the tile tests share: the ctypes binding of the emulator driver (tests/emu/tiles_emu.cpp, built by
__graft_entry__.build()), one picture through its tile chains on the emulator, and the cases both the emulator tests and the
GPU tests decide (the reference of each computed once, tests/tile_oracle.py)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import emu_py
import hmo_py
import search_trace as st
from tile_oracle import grid, moved_planes, plateau_planes, tile_reference
from wpp_oracle import WppOracle

_P = C.c_void_p
SIGNATURES = {
    "grid": ([C.c_int] * 4 + [_P, _P], C.c_int), "chains": ([C.c_int] * 5, C.c_int),
    "create": ([C.c_int] * 8 + [_P] * 7 + [C.c_int, C.c_double] + [C.c_int] * 4 + [_P, _P, C.c_int, _P, C.c_int, _P, C.c_int], _P),
    "destroy": ([_P], None), "n": ([_P], C.c_int), "run": ([_P], C.c_int), "read_before_write": ([_P], C.c_int),
    "chain": ([_P, C.c_int, _P], C.c_int),
    "set_decision": ([_P, C.c_int, _P, _P, C.c_int, _P], None),
    "get_state_full": ([_P, C.c_int, _P, _P], None), "get_verify": ([_P, _P], None), "get_search_state": ([_P, C.c_int, _P], None),
}
I_PICTURE = [0, 0.0, 0, 0, 0, 0, None, None, 0, None, 0, None, 0]      # create's arguments from n_ref to tmvp


@functools.lru_cache(maxsize=None)
def load_emu():
    lib = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu", "libtiles_emu.so"))
    for name, (argtypes, restype) in SIGNATURES.items():
        f = getattr(lib, "tiles_emu_" + name)
        f.argtypes, f.restype = argtypes, restype
    return lib


@pytest.fixture(scope="session")
def tiles_emu(built):
    return load_emu()


def expected_chains(W, H, tiles, wpp):
    """what the binder must give every chain, in chain order: (tile_x0, tile_y0, tile_w, tile_h, next_ctu, end_ctu, wpp_above)"""
    cb, rb = grid(W, H, *tiles)
    res = []
    for ty in range(tiles[1]):
        for tx in range(tiles[0]):
            x0, y0, tw, th = cb[tx], rb[ty], cb[tx + 1] - cb[tx], rb[ty + 1] - rb[ty]
            if not wpp:
                res.append((x0, y0, tw, th, 0, tw * th, 0))
                continue
            for r in range(th):
                res.append((x0, y0, tw, th, r * tw, (r + 1) * tw, len(res) - 1 if r else -1))
    return res


def emulate(lib, f, qp, tiles, wpp, tools=-1, decision=None, p=None, reset_decision=False):
    """One picture through the emulated tile chains.  p: None (I picture) or a dict lam, sr, fast, amp, btab, ref (planes) and
    optionally col (bytes of the reference picture's Ctu array: TMVP on).
    decision: (state, obf of the picture, sw_skip, sw_term, depth_exception).  reset_decision: chain_set_decision (Training) on
    every chain after binding, as fcu_chain_set_decision rewrites the descriptor tail.
    Returns a dict: out (Ctu array), rec, states [(ctx, frac)] and mvs per chain, rbw, verify, chains (the binder's fields)."""
    h, w = f[0].shape
    org = [np.ascontiguousarray(a) for a in f]
    rec = [np.full_like(a, 0x5A) for a in org]                # poisoned
    W, H = (w + 63) // 64, (h + 63) // 64
    out = (hmo_py.Ctu * (W * H))()
    C.memset(out, 0xA5, C.sizeof(out))
    pargs = I_PICTURE
    if p is not None:
        pads = [emu_py.pad_planes([np.ascontiguousarray(a) for a in p["ref"]])]
        ptrs = (C.c_void_p * 3)(*[a.ctypes.data for a in pads[0]])
        pocs, crp = np.array([0], np.int32), np.array([-1], np.int32)
        colbuf = None if p.get("col") is None else np.frombuffer(p["col"], np.uint8).copy()
        pargs = [1, p["lam"], p["sr"], p["fast"], p["amp"], p["btab"], ptrs, pocs.ctypes.data, 1, crp.ctypes.data, 1,
                 None if colbuf is None else colbuf.ctypes.data, int(colbuf is not None)]
    hd = lib.tiles_emu_create(w, h, qp, tiles[0], tiles[1], int(wpp), 0, tools, *[a.ctypes.data for a in org], *[a.ctypes.data for a in rec], C.addressof(out), *pargs)
    assert hd, "the binder refused valid arguments"
    try:
        n = lib.tiles_emu_n(hd)
        assert n == lib.tiles_emu_chains(W, H, tiles[0], tiles[1], int(wpp)) == tiles[0] * (H if wpp else tiles[1])

        def fields():
            res = []
            for i in range(n):
                six = (C.c_int * 6)()
                above = lib.tiles_emu_chain(hd, i, six)
                res.append(tuple(six) + (above,))
            return res
        chains = fields()
        assert chains == expected_chains(W, H, tiles, wpp)
        zero4 = np.zeros(4, np.uint8)
        if reset_decision:
            lib.tiles_emu_set_decision(hd, hmo_py.TRAINING, zero4.ctypes.data, zero4.ctypes.data, 0, None)
            assert fields() == chains, "chain_set_decision touched the tile rectangle"
        if decision is not None:
            obf16 = np.ascontiguousarray(decision[1], np.int16)
            sk, te = np.array(decision[2], np.uint8), np.array(decision[3], np.uint8)
            lib.tiles_emu_set_decision(hd, decision[0], sk.ctypes.data, te.ctypes.data, decision[4], obf16.ctypes.data)
        assert lib.tiles_emu_run(hd) == n
        states, mvs = [], []
        for i in range(n):
            ctx, frac = np.zeros(176, np.uint8), C.c_uint64(0)
            lib.tiles_emu_get_state_full(hd, i, ctx.ctypes.data, C.byref(frac))
            states.append((ctx, frac.value))
            xy = np.zeros(8, np.int32)
            lib.tiles_emu_get_search_state(hd, i, xy.ctypes.data)
            mvs.append([(int(xy[2 * k]), int(xy[2 * k + 1])) for k in range(4)])
        v = np.zeros((4, 6), np.float64)
        lib.tiles_emu_get_verify(hd, v.ctypes.data)
        return dict(out=out, rec=rec, states=states, mvs=mvs, rbw=lib.tiles_emu_read_before_write(hd), verify=v, chains=chains)
    finally:
        lib.tiles_emu_destroy(hd)


# ---- the cases.  I picture: 192 x 136 = 3 x 3 CTUs with an 8-sample partial bottom row, tiles 2 x 2: widths 1 and 2, heights 1
# and 2 -- the one-CTU-wide tiles load nothing at a row start, the two-wide ones load and save at tile_x0 / tile_x0 + 1.
I_W, I_H, I_TILES, I_SEED = 192, 136, (2, 2), 9
I_QPS = (27, 37)


def i_frame(pkg):
    return pkg.synth.mixed(I_W, I_H, seed=I_SEED)


@functools.lru_cache(maxsize=None)
def i_reference(pkg, qp, wpp, testing=False):
    f = i_frame(pkg)
    return tile_reference(f, qp, I_TILES, wpp=wpp, decision=i_decision(f) if testing else None)


def i_decision(f):
    """the fork's Testing state with switches that prune (the picture's OBF map; the reference crops it per tile)"""
    obf, _ = hmo_py.obf_prepass(f[0])
    return (hmo_py.TESTING, obf, (1, 1, 0, 1), (1, 0, 1, 1), 0)


# One more I picture for the row wait: 512 x 128 = 8 x 2 CTUs, tiles 2 x 1 of 4 x 2 CTUs -- the second row of the tile at tile_x0 = 4
# waits for min(x + 2, 4) CTUs of the row above with x counted inside the tile (x + 2 < tile_w at x = 0, 1).
WIDE_W, WIDE_H, WIDE_TILES, WIDE_QP = 512, 128, (2, 1), 32


def wide_frame(pkg):
    return pkg.synth.mixed(WIDE_W, WIDE_H, seed=I_SEED)


@functools.lru_cache(maxsize=None)
def wide_reference(pkg, wpp):
    return tile_reference(wide_frame(pkg), WIDE_QP, WIDE_TILES, wpp=wpp)


# P pictures.  name: (w, h, tiles, mode, search range, TZ, AMP, plateau half-width M or None)
#  - tile columns: 256 x 128 (4 x 2 CTUs), tiles 2 x 1.  The reference planes are a source picture made plateaus of half-width M
#    around the column boundary; crop equivalence needs reach = max |mv| / 4 + SearchRange + 5 <= M (tile_oracle.reach_of,
#    asserted on the reference's own result).  The picture to decide is that REFERENCE moved by (4, 2) luma samples plus +-2
#    noise, so the plateau moves with the content and inter prediction works across the column boundary: the CUs at the left
#    edge of the right-hand tile are inter and so are their left neighbours in the other tile -- the case the mask of the
#    motion neighbours (fcu_inter.h: nb_motion) exists for (tile_oracle.left_edge_evidence, asserted).  Vectors are about
#    (16, 8) quarter samples, so with SearchRange 8 the reach is about 4 + 8 + 5 = 17, inside M = 32 <= 64 (HM's vector
#    clipping binds in neither run).  The AMP case moves bands of the left quarter of the picture, away from the boundary, with
#    a second vector (-4, 4);
#  - tile rows: 128 x 256 (2 x 4 CTUs), tiles 1 x 2 of equal height, against the sliced reference; the reference picture is the
#    plain previous picture.  rows_tz_tmvp: TMVP on (allowed without tile columns) -- the reference picture is a decided P
#    picture whose Ctu array is the collocated field.
P_M = 32
P_CASES = {
    "cols_tz": (256, 128, (2, 1), "crop", 8, 1, 0, P_M),
    "cols_full_amp": (256, 128, (2, 1), "crop", 4, 0, 1, P_M),
    "rows_tz": (128, 256, (1, 2), "sliced", 8, 1, 0, None),
    "rows_full": (128, 256, (1, 2), "sliced", 4, 0, 0, None),
    "rows_tz_tmvp": (128, 256, (1, 2), "sliced", 8, 1, 0, None),
}
P_TMVP = ("rows_tz_tmvp",)
P_BASE_QP = 30


@functools.lru_cache(maxsize=None)
def p_inputs(pkg, name):
    """(frame, qp, p) of a P case: p = the emulator's / engine's arguments, ref = the reference planes of the test"""
    w, h, tiles, mode, sr, fast, amp, M = P_CASES[name]
    _, qp, lam = hmo_py.ldp_slice(1, P_BASE_QP)
    p = dict(lam=lam, sr=sr, fast=fast, amp=amp, btab=0)
    if M is not None:
        f0 = st.moving_frame(pkg.synth, "mixed", w, h, 7, 0)
        ref = plateau_planes(f0, *grid((w + 63) // 64, (h + 63) // 64, *tiles), M)      # the planes need not be a reconstruction
        f = moved_planes(ref, 4, 2)
        if amp:
            b = moved_planes(ref, -4, 4)
            yy, xx = np.mgrid[0:h, 0:w]
            m = (xx < w // 4) & ((yy % 64) >= 48)
            f = [np.where(mk, q, r) for mk, q, r in zip((m, m[::2, ::2], m[::2, ::2]), b, f)]
        noise = np.random.default_rng(1234).integers(-2, 3, (h, w))
        f = [np.clip(f[0].astype(np.int16) + noise, 0, 255).astype(np.uint8), np.ascontiguousarray(f[1]), np.ascontiguousarray(f[2])]
        return tuple(f), qp, dict(p, ref=ref)
    if name in P_TMVP:
        f0, f1, f2 = (st.moving_frame(pkg.synth, "mixed", w, h, 7, poc) for poc in range(3))
        e = hmo_py.Encoder(*f1, qp, ref=f0, lambda_override=lam, search_range=sr, fast_search=fast)     # the collocated picture: a P picture
        e.compress_frame()
        return f2, qp, dict(p, ref=[q.copy() for q in e.rec], col=e.all_ctus_bytes())
    f0, f1 = (st.moving_frame(pkg.synth, "mixed", w, h, 7, poc) for poc in range(2))
    return f1, qp, dict(p, ref=[np.ascontiguousarray(a) for a in f0])


def _enc_kw(p):
    kw = dict(ref=p["ref"], lambda_override=p["lam"], search_range=p["sr"], fast_search=p["fast"], amp=p["amp"])
    if p.get("col") is not None:
        kw["col"] = p["col"]
    return kw


@functools.lru_cache(maxsize=None)
def p_reference(pkg, name, wpp):
    w, h, tiles, mode, sr, fast, amp, M = P_CASES[name]
    f, qp, p = p_inputs(pkg, name)
    return tile_reference(f, qp, tiles, wpp=wpp, mode=mode, **_enc_kw(p))


@functools.lru_cache(maxsize=None)
def p_untiled(pkg, name, wpp):
    """the same picture decided without tiles by the unchanged references: bytes of its Ctu array"""
    f, qp, p = p_inputs(pkg, name)
    if wpp:
        return WppOracle(*f, qp, **_enc_kw(p)).run().enc.all_ctus_bytes()
    e = hmo_py.Encoder(*f, qp, slice_ctus=0, **_enc_kw(p))
    e.compress_frame()
    return e.all_ctus_bytes()
