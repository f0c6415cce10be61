"""The tile reference itself (tests/tile_oracle.py) and the host arithmetic of the tile grid: fcu_tile_grid against HM's uniform
spacing, a 1 x 1 grid against the unchanged one-slice references, and the proof that the tiled 192 x 136 picture the other tile
tests decide is not the untiled picture nor the slices-of-rows picture -- a neighbour-masking bug must not be able to hide."""
import ctypes as C

import numpy as np
import pytest

import hmo_py
from tile_oracle import grid, left_edge_evidence, reach_of, tile_reference, tile_scan
from tiles_testlib import (I_QPS, I_TILES, P_CASES, P_TMVP, i_frame, i_reference, p_inputs, p_reference, p_untiled,
                           tiles_emu)  # noqa: F401 (tiles_emu: the fixture)
from wpp_oracle import wpp_oracle

GRIDS = [(60, 34, 4, 2), (3, 3, 2, 2), (30, 17, 4, 2), (5, 4, 5, 4), (7, 3, 3, 2), (4, 2, 1, 1)]


@pytest.mark.parametrize("W,H,Cn,Rn", GRIDS)
def test_tile_grid_is_hm_uniform_spacing(tiles_emu, pkg, W, H, Cn, Rn):
    want = ([i * W // Cn for i in range(Cn + 1)], [i * H // Rn for i in range(Rn + 1)])
    assert grid(W, H, Cn, Rn) == want
    cb, rb = (C.c_int * (Cn + 1))(), (C.c_int * (Rn + 1))()
    assert tiles_emu.tiles_emu_grid(W, H, Cn, Rn, cb, rb) == 1 and (list(cb), list(rb)) == want      # fcu_host.h: tile_grid
    assert pkg.engine.tile_grid(W, H, Cn, Rn) == want                                                   # fcu_tile_grid of libfcu.so
    assert all(b > a for a, b in zip(want[0], want[0][1:])) and all(b > a for a, b in zip(want[1], want[1][1:]))     # no empty tile
    assert sorted(tile_scan(W, H, Cn, Rn)) == list(range(W * H))
    assert tiles_emu.tiles_emu_chains(W, H, Cn, Rn, 0) == Cn * Rn and tiles_emu.tiles_emu_chains(W, H, Cn, Rn, 1) == Cn * H


def test_the_4k_example_of_the_header(pkg):
    cb, rb = pkg.engine.tile_grid(60, 34, 4, 2)
    assert cb == [0, 15, 30, 45, 60] and rb == [0, 17, 34]
    assert 15 + 2 * (17 - 1) == 47 and 60 + 2 * (34 - 1) == 126       # the critical paths DESIGN.md 3h quotes, in CTU-times


@pytest.mark.parametrize("W,H,Cn,Rn", [(3, 3, 4, 1), (3, 3, 1, 4), (3, 3, 0, 1), (3, 3, 1, 0), (3, 3, -1, 2)])
def test_a_grid_with_an_empty_tile_is_rejected(tiles_emu, pkg, W, H, Cn, Rn):
    assert tiles_emu.tiles_emu_grid(W, H, Cn, Rn, None, None) == 0
    assert tiles_emu.tiles_emu_chains(W, H, Cn, Rn, 0) == -1 and tiles_emu.tiles_emu_chains(W, H, Cn, Rn, 1) == -1
    assert pkg.load_lib().fcu_tile_grid(W, H, Cn, Rn, None, None) == -2          # FCU_ERR_ARG
    with pytest.raises(ValueError):
        pkg.engine.tile_grid(W, H, Cn, Rn)


def test_a_1x1_grid_is_the_one_slice_reference(pkg):
    f = i_frame(pkg)
    one = hmo_py.Encoder(*f, 27, slice_ctus=0)
    one.compress_frame()
    t = tile_reference(f, 27, (1, 1))
    assert t.ctus == one.all_ctus_bytes() and t.excluded == [] and len(t.chains) == 1
    assert np.array_equal(t.chains[0]["ctx"], one.cabac(full=True)[0]) and t.chains[0]["frac"] == one.cabac(full=True)[1]
    w = wpp_oracle(*f, 27)
    tw = tile_reference(f, 27, (1, 1), wpp=True)
    assert tw.ctus == w.enc.all_ctus_bytes() and [c["frac"] for c in tw.chains] == [s[1] for s in w.row_state]


@pytest.mark.parametrize("qp", I_QPS)
def test_the_tiled_picture_is_neither_the_untiled_nor_the_sliced_picture(pkg, qp):
    f = i_frame(pkg)
    dt = np.dtype(hmo_py.Ctu)
    for wpp in (False, True):
        t = i_reference(pkg, qp, wpp)
        assert t.excluded == [0, 2, 6] and len(t.chains) == (6 if wpp else 4)      # last CTU of tiles 0, 1, 2 of the 3 x 3 picture
        if wpp:
            untiled = wpp_oracle(*f, qp).enc.all_ctus_bytes()
            sliced = wpp_oracle(*f, qp, 1).enc.all_ctus_bytes()
        else:
            e = hmo_py.Encoder(*f, qp, slice_ctus=0)
            e.compress_frame()
            untiled = e.all_ctus_bytes()
            e = hmo_py.Encoder(*f, qp, slice_ctus=3)           # slices of one CTU row
            e.compress_frame()
            sliced = e.all_ctus_bytes()
        assert t.ctus != untiled and t.ctus != sliced
        # the CTU at the left edge of the right-hand tiles (column 1) loses its left neighbours: CTU 1 (first row, tile 1) and
        # CTU 4 (tile 3) must not equal their untiled twins, while CTU 0 -- first CTU of the picture either way -- must
        a, b = np.frombuffer(t.ctus, dt), np.frombuffer(untiled, dt)
        assert a[0] == b[0]
        assert a[1] != b[1] and a[4] != b[4], "a CU at a tile's left edge equals its untiled twin: masking cannot be seen on this input"


def test_p_references_are_inter_pictures_within_reach_of_their_plateaus(pkg):
    """the precondition of the crop comparison, on the reference's own result: max |mv| / 4 + SearchRange + 5 <= M"""
    for name, (w, h, tiles, mode, sr, fast, amp, M) in P_CASES.items():
        for wpp in (False, True):
            t = p_reference(pkg, name, wpp)
            reach, n_inter = reach_of(t.ctus, sr)
            assert n_inter > 0, name
            if M is not None:
                assert M <= 64 and reach <= M, (name, reach)
            assert len(t.excluded) == tiles[0] * tiles[1] - 1


@pytest.mark.parametrize("name", [n for n, c in P_CASES.items() if c[2][0] > 1])
def test_p_pictures_with_tile_columns_show_the_mask_of_the_motion_neighbours(pkg, name):
    """On the reference's own result: CUs at the left edge of the right-hand tile are inter, have inter left neighbours in the
    other tile, and their merge / AMVP data differ from their twins of the untiled picture -- so an engine that masked the
    motion neighbours vertically only (or not at all) cannot match the tiled reference on these inputs."""
    for wpp in (False, True):
        t = p_reference(pkg, name, wpp)
        untiled = p_untiled(pkg, name, wpp)
        n_nb, n_diff = left_edge_evidence(t, untiled)
        assert n_nb > 0, "no inter CU at a tile's left edge with an inter left neighbour in the other tile"
        assert n_diff > 0, "the CUs at the tile's left edge equal their untiled twins: the mask cannot be seen on this input"
        assert t.ctus != untiled


def test_tmvp_with_tile_rows_uses_the_collocated_field(pkg):
    for name in P_TMVP:
        f, qp, p = p_inputs(pkg, name)
        assert p["col"] is not None and (np.frombuffer(p["col"], np.dtype(hmo_py.Ctu))["pred_mode"] == 0).sum() > 0      # a field with motion
        w, h, tiles, mode, sr, fast, amp, M = P_CASES[name]
        without = tile_reference(f, qp, tiles, mode=mode, ref=p["ref"], lambda_override=p["lam"], search_range=sr, fast_search=fast, amp=amp)
        assert p_reference(pkg, name, False).ctus != without.ctus, "TMVP changes nothing on this input"
