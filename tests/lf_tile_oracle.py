"""Reference for the loop filters of a picture with tiles (LFCrossTileBoundaryFlag 0 and 1), what the CPU tests
(tests/test_lf_tiles.py) and the GPU tests (tests/test_gpu_lf_tiles.py) share: the reference itself, the ctypes binding of the
emulator driver (tests/emu/lf_tiles_emu.cpp), and the cases with their references computed once.

Deblocking needs no new code.  LFCrossTileBoundaryFlag 1 is TileRef.deblocked(): the whole picture through the unchanged oracle.
With the flag 0 HM gives the 4x4 partitions whose left / top edge lies on a tile boundary no edge flag (TComLoopFilter.cpp:379,401,
430-434,609-613,754-758), as on the picture border.  That equals deblocking every tile's crop on its own with the unchanged oracle
and pasting the results (deblock_stitched): the border of a crop is never filtered, an edge reads 4 samples and writes 3 on either
side and so stays inside its tile, and the QP and the motion a partition's boundary strength looks at across a filtered edge are
its own tile's.

SAO is tests/emu/lf_tile_ref.c (sao_tiles): oracle/hmo_sao.c's hmo_sao_picture with two rules added and every function below it
the oracle's own -- merge candidates inside the CTU's tile for either value of the flag (TComPic.cpp:138-143), and with the flag 0
a CTU of another tile unavailable to the statistics and the offset pass (TComPicSym.cpp:378,449-459).

Not pinned by an HM run: like tests/tile_oracle.py, this reference rests on reading the HM lines cited; no run of HM with tiles has
recorded results to compare with.  What pins it instead, each point a test of tests/test_lf_tiles.py:
  - a 1 x 1 grid equals hmo_py.sao_picture, which the HM goldens (tests/golden/sao.npz) pin, for either value of the flag;
  - with the flag 0, every tile's statistics equal hmo_py.sao_picture(..., want_stats=True) on that tile's crop: a tile then sees
    what a picture cropped to it sees;
  - with the flag 1, the statistics equal those of the picture without tiles: only the merge candidates know about tiles."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import hmo_py
from tile_oracle import CTU_BYTES, grid, tile_reference

_HERE = os.path.dirname(os.path.abspath(__file__))
_P = C.c_void_p


# ---- the reference ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_lib():
    lib = C.CDLL(os.path.join(_HERE, "emu", "liblf_tile_ref.so"))
    lib.lf_ref_sao_tiles.argtypes = [C.c_int] * 4 + [_P] * 4 + [C.c_int] + [_P] * 5
    lib.lf_ref_sao_tiles.restype = None
    return lib


def starts(w, h, tiles):
    """(col_start, row_start): uint8 flags per CTU column / row, 1 = the first of a tile; one entry more than the picture has,
    so that index + 1 exists"""
    W, H = (w + 63) // 64, (h + 63) // 64
    cb, rb = grid(W, H, *tiles)
    cs, rs = np.zeros(W + 1, np.uint8), np.zeros(H + 1, np.uint8)
    cs[cb[:-1]] = 1
    rs[rb[:-1]] = 1
    return cs, rs


def sao_tiles(org, rec, qp, slice_type, lam, tiles, cross, enabled=(1, 1, 1), want_stats=False):
    """hmo_py.sao_picture for a picture cut into tiles = (C, R) with LFCrossTileBoundaryFlag = cross: in place on `rec`, returns
    (params int32 [n_ctu, 3, 35], off_count[3], stats int64 [n_ctu, 3, 2, 5, 32] or None)"""
    h, w = org[0].shape
    n = ((w + 63) // 64) * ((h + 63) // 64)
    for a in list(org) + list(rec):
        assert a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"]
    cs, rs = starts(w, h, tiles)
    po = (C.c_void_p * 3)(*[a.ctypes.data for a in org])
    pr = (C.c_void_p * 3)(*[a.ctypes.data for a in rec])
    lams = (C.c_double * 3)(*hmo_py.slice_lambdas(qp, lam))
    en = (C.c_int * 3)(*[int(v) for v in enabled])
    params = np.zeros((n, 3, 35), np.int32)
    stats = np.zeros((n, 3, 2, 5, 32), np.int64) if want_stats else None
    off = (C.c_int * 3)()
    _ref_lib().lf_ref_sao_tiles(w, h, qp, slice_type, C.cast(lams, _P), C.cast(en, _P), cs.ctypes.data, rs.ctypes.data, int(cross),
                                C.cast(po, _P), C.cast(pr, _P), params.ctypes.data, stats.ctypes.data if want_stats else None, C.cast(off, _P))
    return params, list(off), stats


def tile_rects(w, h, tiles):
    """[(x0, y0, x1, y1)] of the tiles in CTUs, tile-scan order"""
    cb, rb = grid((w + 63) // 64, (h + 63) // 64, *tiles)
    return [(cb[tx], rb[ty], cb[tx + 1], rb[ty + 1]) for ty in range(tiles[1]) for tx in range(tiles[0])]


def crop(planes, rect, w, h):
    x0, y0, x1, y1 = rect
    return [p[(y0 * 64) >> s:min(y1 * 64, h) >> s, (x0 * 64) >> s:min(x1 * 64, w) >> s].copy() for p, s in zip(planes, (0, 1, 1))]      # (a copy, never a view)


def paste(planes, rect, parts):
    x0, y0, _, _ = rect
    for p, q, s in zip(planes, parts, (0, 1, 1)):
        p[(y0 * 64) >> s:((y0 * 64) >> s) + q.shape[0], (x0 * 64) >> s:((x0 * 64) >> s) + q.shape[1]] = q


def deblock_stitched(ctus, w, h, rec, tiles):
    """LFCrossTileBoundaryFlag 0: every tile's crop deblocked on its own by the unchanged oracle, pasted.  ctus: bytes of the
    picture's Ctu array; rec: the planes before deblocking (not modified).  Returns new planes."""
    W = (w + 63) // 64
    out = [p.copy() for p in rec]
    for rect in tile_rects(w, h, tiles):
        x0, y0, x1, y1 = rect
        raw = b"".join(ctus[(y * W + x) * CTU_BYTES:(y * W + x + 1) * CTU_BYTES] for y in range(y0, y1) for x in range(x0, x1))
        part = crop(rec, rect, w, h)
        hmo_py.deblock_pic(raw, part[0].shape[1], part[0].shape[0], part)
        paste(out, rect, part)
    return out


def deblocked(ref, tiles, cross):
    """the decided picture `ref` (tile_oracle.TileRef) after deblocking with LFCrossTileBoundaryFlag = cross"""
    return ref.deblocked() if cross else deblock_stitched(ref.ctus, ref.w, ref.h, ref.rec, tiles)


# ---- the emulator driver ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def load_emu():
    lib = C.CDLL(os.path.join(_HERE, "emu", "liblf_tiles_emu.so"))
    lib.lf_tiles_emu_grid.argtypes = [C.c_int] * 5 + [_P]
    lib.lf_tiles_emu_deblock.argtypes = [_P] * 4 + [C.c_int] * 7
    lib.lf_tiles_emu_sao.argtypes = [C.c_int] * 4 + [_P, _P] + [C.c_int] * 3 + [_P] * 9
    return lib


@pytest.fixture(scope="session")
def lf_emu(built):
    return load_emu()


def emu_deblock(lib, ctus, w, h, rec, tiles, cross):
    """in place on rec"""
    buf = np.frombuffer(ctus, np.uint8).copy()
    assert lib.lf_tiles_emu_deblock(buf.ctypes.data, *[a.ctypes.data for a in rec], w, h, 0, 0, tiles[0], tiles[1], int(cross)) == 1


def emu_sao(lib, org, rec, qp, slice_type, lam, tiles, cross, enabled=(1, 1, 1)):
    """in place on rec; returns (coded uint8 [n, 108], off_count int32 [3], stats int64 in the reference's layout [n, 3, 2, 5, 32])"""
    h, w = org[0].shape
    n = ((w + 63) // 64) * ((h + 63) // 64)
    lams, en = np.array(hmo_py.slice_lambdas(qp, lam), np.float64), np.array(enabled, np.int32)
    coded, off = np.zeros((n, 108), np.uint8), np.zeros(3, np.int32)
    stats = np.zeros((n, 3, 5, 2, 32), np.int32)
    assert lib.lf_tiles_emu_sao(w, h, slice_type, qp, lams.ctypes.data, en.ctypes.data, tiles[0], tiles[1], int(cross), *[a.ctypes.data for a in org],
                                *[a.ctypes.data for a in rec], coded.ctypes.data, off.ctypes.data, stats.ctypes.data) == 1
    return coded, off, np.ascontiguousarray(stats.astype(np.int64).transpose(0, 1, 3, 2, 4))


# ---- the cases -------------------------------------------------------------------------------------------------------------
# 208 x 136 = 4 x 3 CTUs whose last column (16 samples) and last row (8 samples) are partial.  2 x 2: columns {0,1 | 2,3}, rows
# {0 | 1,2} -- an interior tile corner, and CTU (2, 1) has a left and an above neighbour in the picture that both belong to other
# tiles.  3 x 1: columns {0 | 1 | 2,3} -- a one-CTU-wide tile with tile edges on both sides, and the partial column next to a
# tile's inner CTU.  1 x 2: rows {0 | 1,2} -- row boundaries only.
W, H = 208, 136
GRIDS = ((2, 2), (3, 1), (1, 2))
QP, CONTENT, SEED = 32, "textured", 7
LAMBDA = 0.57 * 2.0 ** ((QP - 12) / 3.0)
SLICE_TYPES = (hmo_py.SLICE_I, hmo_py.SLICE_P)                 # the slice type SAO is told: the initial state of its two contexts


def frame(pkg):
    return [np.ascontiguousarray(a) for a in getattr(pkg.synth, CONTENT)(W, H, seed=SEED)]


@functools.lru_cache(maxsize=None)
def decided(pkg, tiles):
    """the picture decided through the tile path (tile_oracle.TileRef, I slice)"""
    return tile_reference(frame(pkg), QP, tiles)


@functools.lru_cache(maxsize=None)
def filtered(pkg, tiles, cross, slice_type, enabled=(1, 1, 1)):
    """decide -> deblock -> SAO by the reference: dict dbk (planes after deblocking), params, off, stats, rec (planes after SAO)"""
    dbk = deblocked(decided(pkg, tiles), tiles, cross)
    rec = [p.copy() for p in dbk]
    params, off, stats = sao_tiles(frame(pkg), rec, QP, slice_type, LAMBDA, tiles, cross, enabled=enabled, want_stats=True)
    return dict(dbk=dbk, params=params, off=off, stats=stats, rec=rec)
