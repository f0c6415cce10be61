"""Loop filters of a picture with tiles on the CPU: what pins the tile reference of tests/lf_tile_oracle.py (its docstring), the
tile variants of the kernel source on the emulator (tests/emu/lf_tiles_emu.cpp) against that reference for every grid x
LFCrossTileBoundaryFlag x slice type, that each case is not vacuous (asserted on the reference alone), and the rules of the two
drivers.  Every comparison is exact."""
import numpy as np
import pytest

import hmo_py
import lf_tile_oracle as L
import test_sao as T
from lf_tile_oracle import lf_emu  # noqa: F401 (fixture)

CASES = [(g, c) for g in L.GRIDS for c in (0, 1)]
IDS = ["%dx%d_cross%d" % (g[0], g[1], c) for g, c in CASES]


# ---- what pins the reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cross", (0, 1))
@pytest.mark.parametrize("slice_type", L.SLICE_TYPES)
def test_reference_with_one_tile_is_the_oracle(pkg, built, cross, slice_type):
    dbk = L.decided(pkg, (1, 1)).deblocked()
    a, b = [p.copy() for p in dbk], [p.copy() for p in dbk]
    want = hmo_py.sao_picture(L.frame(pkg), a, L.QP, slice_type, L.LAMBDA, want_stats=True)
    got = L.sao_tiles(L.frame(pkg), b, L.QP, slice_type, L.LAMBDA, (1, 1), cross, want_stats=True)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] and np.array_equal(got[2], want[2])
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    assert any(not np.array_equal(p, q) for p, q in zip(a, dbk)), "SAO changed nothing: the case shows nothing"


@pytest.mark.parametrize("tiles", L.GRIDS, ids=lambda g: "%dx%d" % g)
def test_reference_statistics_without_crossing_are_those_of_each_tiles_crop(pkg, built, tiles):
    f, r = L.frame(pkg), L.filtered(pkg, tiles, 0, hmo_py.SLICE_I)
    Wc = (L.W + 63) // 64
    for rect in L.tile_rects(L.W, L.H, tiles):
        x0, y0, x1, y1 = rect
        org, rec = L.crop(f, rect, L.W, L.H), L.crop(r["dbk"], rect, L.W, L.H)
        _, _, stats = hmo_py.sao_picture(org, rec, L.QP, hmo_py.SLICE_I, L.LAMBDA, want_stats=True)
        addr = [y * Wc + x for y in range(y0, y1) for x in range(x0, x1)]
        assert np.array_equal(r["stats"][addr], stats), rect


@pytest.mark.parametrize("tiles", L.GRIDS, ids=lambda g: "%dx%d" % g)
def test_reference_statistics_with_crossing_are_those_of_the_untiled_picture(pkg, built, tiles):
    r = L.filtered(pkg, tiles, 1, hmo_py.SLICE_I)
    rec = [p.copy() for p in r["dbk"]]
    _, _, stats = hmo_py.sao_picture(L.frame(pkg), rec, L.QP, hmo_py.SLICE_I, L.LAMBDA, want_stats=True)
    assert np.array_equal(r["stats"], stats)
    assert not np.array_equal(L.filtered(pkg, tiles, 0, hmo_py.SLICE_I)["stats"], stats), "the flag changes no statistic: the case shows nothing"


# ---- non-vacuity, on the reference alone -------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiles,cross", CASES, ids=IDS)
def test_the_untiled_sao_merges_across_a_tile_boundary(pkg, built, tiles, cross):
    """rule 1 changes the result: SAO without tiles of the same deblocked picture signals a merge whose candidate lies in another
    tile, and the tile reference signals something else"""
    r = L.filtered(pkg, tiles, cross, hmo_py.SLICE_I)
    rec = [p.copy() for p in r["dbk"]]
    params, _, _ = hmo_py.sao_picture(L.frame(pkg), rec, L.QP, hmo_py.SLICE_I, L.LAMBDA)
    cs, rs = L.starts(L.W, L.H, tiles)
    Wc = (L.W + 63) // 64
    across = [a for a in range(len(params)) if params[a, 0, 0] == 2 and (cs[a % Wc] if params[a, 0, 1] == 0 else rs[a // Wc])]
    assert across, "no merge across a tile boundary"
    assert all(r["params"][a, 0, 0] != 2 or r["params"][a, 0, 1] != params[a, 0, 1] for a in across)
    assert not np.array_equal(T.M.canon(r["params"]), T.M.canon(params))


@pytest.mark.parametrize("tiles", L.GRIDS, ids=lambda g: "%dx%d" % g)
def test_deblocking_without_crossing_differs_on_both_sides_of_a_tile_edge(pkg, built, tiles):
    """rule 3 changes the result: whole-picture deblocking and the stitched per-tile deblocking differ in a sample on either side
    of at least one tile edge -- and nowhere further than 4 samples from one"""
    ref = L.decided(pkg, tiles)
    whole, cut = ref.deblocked(), L.deblock_stitched(ref.ctus, L.W, L.H, ref.rec, tiles)
    d = whole[0] != cut[0]
    cs, rs = L.starts(L.W, L.H, tiles)
    sides = []
    for b in [64 * i for i in range(1, len(cs) - 1) if cs[i]]:
        sides.append(bool(d[:, b - 4:b].any() and d[:, b:b + 4].any()))
        d[:, b - 4:b + 4] = False
    for b in [64 * i for i in range(1, len(rs) - 1) if rs[i]]:
        sides.append(bool(d[b - 4:b, :].any() and d[b:b + 4, :].any()))
        d[b - 4:b + 4, :] = False
    assert any(sides), "no tile edge with a changed sample on both of its sides"
    assert not d.any(), "the flag changed a sample away from the tile edges"


# ---- the kernel source on the emulator ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiles,cross", CASES, ids=IDS)
def test_emulated_deblocking_matches_the_reference(pkg, lf_emu, tiles, cross):
    """flag 0: the per-tile oracle, stitched; flag 1: today's whole-picture deblocking"""
    ref = L.decided(pkg, tiles)
    rec = [p.copy() for p in ref.rec]
    L.emu_deblock(lf_emu, ref.ctus, L.W, L.H, rec, tiles, cross)
    for k, (p, q) in enumerate(zip(rec, L.deblocked(ref, tiles, cross))):
        assert np.array_equal(p, q), k


def _assert_sao(pkg, got, rec, r):
    coded, off, stats = got
    assert np.array_equal(stats, r["stats"]), "sao_stats"
    assert np.array_equal(T.M.canon(pkg.engine.sao_coded_to_array(coded)), T.M.canon(r["params"])), "sao_cands + sao_decide"
    for k, (p, q) in enumerate(zip(rec, r["rec"])):
        assert np.array_equal(p, q), ("sao_apply", k)
    assert list(off) == r["off"], "off_count"


@pytest.mark.parametrize("slice_type", L.SLICE_TYPES, ids=["I", "P"])
@pytest.mark.parametrize("tiles,cross", CASES, ids=IDS)
def test_emulated_sao_matches_the_reference(pkg, lf_emu, tiles, cross, slice_type):
    r = L.filtered(pkg, tiles, cross, slice_type)
    rec = [p.copy() for p in r["dbk"]]
    _assert_sao(pkg, L.emu_sao(lf_emu, L.frame(pkg), rec, L.QP, slice_type, L.LAMBDA, tiles, cross), rec, r)


def test_emulated_sao_with_a_component_switched_off(pkg, lf_emu):
    tiles, cross, en = (2, 2), 0, (1, 0, 1)
    r = L.filtered(pkg, tiles, cross, hmo_py.SLICE_P, en)
    assert r["off"][1] == 12 and np.array_equal(r["rec"][1], r["dbk"][1])
    rec = [p.copy() for p in r["dbk"]]
    _assert_sao(pkg, L.emu_sao(lf_emu, L.frame(pkg), rec, L.QP, hmo_py.SLICE_P, L.LAMBDA, tiles, cross, en), rec, r)


def test_emulated_one_tile_is_the_kernel_source_without_tiles(pkg, lf_emu):
    """a 1 x 1 grid through the tile variants == tests/emu/sao_emu.cpp / dbk_emu.cpp, byte for byte"""
    import ctypes as C
    import os
    ref = L.decided(pkg, (1, 1))
    for cross in (0, 1):
        a, b = [p.copy() for p in ref.rec], [p.copy() for p in ref.rec]
        L.emu_deblock(lf_emu, ref.ctus, L.W, L.H, a, (1, 1), cross)
        D = C.CDLL(os.path.join(T.ROOT, "tests", "emu", "libdbk_emu.so"))
        D.dbk_emu.argtypes = [C.c_void_p] * 4 + [C.c_int] * 4
        buf = np.frombuffer(ref.ctus, np.uint8).copy()
        D.dbk_emu(buf.ctypes.data, *[p.ctypes.data for p in b], L.W, L.H, 0, 0)
        assert all(np.array_equal(p, q) for p, q in zip(a, b))
        ra, rb = [p.copy() for p in a], [p.copy() for p in a]
        coded, off, stats = L.emu_sao(lf_emu, L.frame(pkg), ra, L.QP, 0, L.LAMBDA, (1, 1), cross)
        coded0, off0, stats0 = T._emu_sao(L.frame(pkg), rb, L.QP, 0, L.LAMBDA, (1, 1, 1), 0)
        assert np.array_equal(coded, coded0) and np.array_equal(off, off0) and np.array_equal(stats, stats0.astype(np.int64).transpose(0, 1, 3, 2, 4))
        assert all(np.array_equal(p, q) for p, q in zip(ra, rb))


def test_the_grid_masks_and_what_the_binder_refuses(lf_emu):
    m = np.zeros(8, np.uint64)
    assert lf_emu.lf_tiles_emu_grid(L.W, L.H, 3, 1, 0, m.ctypes.data) == 1
    assert list(m) == [0b0111, 0, 0, 0, 1, 0, 0, 0]            # columns {0 | 1 | 2, 3}, one tile row
    assert lf_emu.lf_tiles_emu_grid(64 * 200, 64 * 3, 3, 2, 1, m.ctypes.data) == 1
    assert [int(v) for v in m[:4]] == [1, 1 << (66 - 64), 1 << (133 - 128), 0]      # 200 CTU columns in three: from 0, 66, 133
    assert list(m[4:]) == [0b11, 0, 0, 0]
    for cols, rows, cross in ((5, 1, 0), (1, 4, 1), (0, 1, 0), (2, 2, 2), (2, 2, -1)):
        assert lf_emu.lf_tiles_emu_grid(L.W, L.H, cols, rows, cross, None) == 0
    assert lf_emu.lf_tiles_emu_grid(64 * 257, 64, 2, 1, 0, None) == 0      # beyond the masks


# ---- the drivers -------------------------------------------------------------------------------------------------------------
def test_driver_rules_for_the_flag(pkg):
    ld, sq = pkg.lowdelay.LowDelayPDecider, pkg.sequence.SequenceDecider
    for make in (lambda **kw: sq(256, 192, 32, **kw), lambda **kw: ld(256, 192, 32, **kw)):
        with pytest.raises(ValueError, match="sao.*lf_cross_tiles"):
            make(tiles=(2, 2), sao=True)                          # the flag must be chosen
        with pytest.raises(ValueError, match="lf_cross_tiles"):
            make(tiles=(2, 2), lf_cross_tiles=2)
        with pytest.raises(ValueError, match="lf_cross_tiles"):
            make(tiles=(2, 2), sao=True, lf_cross_tiles=2)
        with pytest.raises(ValueError, match="tiles"):
            make(lf_cross_tiles=0)                                # the flag without tiles
    for flag in (0, 1):
        with pytest.raises(ValueError, match="sao"):
            sq(256, 192, 32, tiles=(2, 2), sao=True, lf_cross_tiles=flag)      # this driver runs no SAO
    # accepted: the construction gets past the argument rules (without a GPU it ends at the engine, which has no CPU fallback)
    for kw in (dict(sao=True, lf_cross_tiles=0), dict(sao=True, lf_cross_tiles=1), dict(lf_cross_tiles=0), dict(sao=True, lf_cross_tiles=0, wpp=True)):
        try:
            d = ld(256, 192, 32, tiles=(2, 2), **kw)
        except pkg.engine.FcuError:
            continue
        assert d.tiles == (2, 2) and d.lf_cross_tiles == kw["lf_cross_tiles"] and d.do_sao == bool(kw.get("sao"))
        d.close()
