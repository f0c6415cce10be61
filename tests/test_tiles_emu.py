"""Tiles on the CPU wave emulator: the engine source's tile chains (tests/emu/tiles_emu.cpp, bound with the rules libfcu.so's
binder uses: fcu_host.h tile_grid / tile_bind / wpp_bind_tile_row) against the reference of tests/tile_oracle.py -- every
fcu_ctu_out field of every CTU, the reconstruction, the coder state after every chain (the Q15 counter left out after the last
CTU of every tile but the last: end_of_slice_segment_flag, tile_oracle's docstring) and for P pictures the search state after
every chain, with the emulator's read-before-write count of the TZ start vectors at zero.  The emulator aborts when a value
claimed wave-uniform (FCU_UNI) differs between lanes, so these runs also keep that check silent on the tile code."""
import ctypes as C

import numpy as np
import pytest

import emu_py
import hmo_py
import search_trace as st
import wpp_testlib
from tile_oracle import assert_picture_equal, tile_reference
from tiles_testlib import (I_PICTURE, I_QPS, I_TILES, P_CASES, WIDE_QP, WIDE_TILES, emulate, i_decision, i_frame, i_reference, p_inputs,
                           p_reference, tiles_emu, wide_frame, wide_reference)  # noqa: F401 (tiles_emu: the fixture)
from wpp_testlib import wpp_emu  # noqa: F401 (fixture)


@pytest.mark.parametrize("wpp", [False, True], ids=["tile_chains", "wpp_in_tiles"])
@pytest.mark.parametrize("qp", I_QPS)
def test_emulated_tiles_of_an_i_picture_are_bit_exact(tiles_emu, pkg, qp, wpp):
    ref = i_reference(pkg, qp, wpp)
    e = emulate(tiles_emu, i_frame(pkg), qp, I_TILES, wpp)
    skipped = assert_picture_equal(ref, bytes(e["out"]), e["rec"], e["states"])
    assert skipped == 3 and len(ref.excluded) == 3            # no more than one CTU per tile, none in the last
    rec = [p.copy() for p in e["rec"]]                       # deblocking crosses the tile boundaries, on the whole picture
    hmo_py.deblock_pic(bytes(e["out"]), 192, 136, rec)
    for p, q in zip(rec, ref.deblocked()):
        assert np.array_equal(p, q)


@pytest.mark.parametrize("wpp", [False, True], ids=["tile_chains", "wpp_in_tiles"])
def test_emulated_tiles_in_the_testing_state(tiles_emu, pkg, wpp):
    """the fork's pruning with the PICTURE's OBF map on the engine side, the map cropped per tile for the reference"""
    f = i_frame(pkg)
    ref = i_reference(pkg, 37, wpp, True)
    assert ref.ctus != i_reference(pkg, 37, wpp).ctus         # the switches prune something on this picture
    e = emulate(tiles_emu, f, 37, I_TILES, wpp, decision=i_decision(f))
    assert_picture_equal(ref, bytes(e["out"]), e["rec"], e["states"])


def test_set_decision_after_binding_leaves_the_tile_rectangle_intact(tiles_emu, pkg):
    """The host half only: chain_set_decision (fcu_host.h), which the emulator and libfcu.so share, leaves the tile fields of
    the host descriptor alone, and the picture decided after the call is still the tiled one.  The trap of ADVICE.md finding 4
    is the other half -- fcu_chain_set_decision in fcu_kernels.hip copies the descriptor tail, tile rectangle included, from
    that host descriptor to the device -- and only a GPU run can see it:
    tests/test_gpu_tiles.py::test_set_decision_after_binding_keeps_the_tiles_on_the_device."""
    for wpp in (False, True):
        e = emulate(tiles_emu, i_frame(pkg), 27, I_TILES, wpp, reset_decision=True)      # (asserts the fields are unchanged)
        assert_picture_equal(i_reference(pkg, 27, wpp), bytes(e["out"]), e["rec"], e["states"])


@pytest.mark.parametrize("wpp", [False, True], ids=["tile_chains", "wpp_in_tiles"])
def test_emulated_four_wide_tiles_are_bit_exact(tiles_emu, pkg, wpp):
    """512 x 128 as 2 x 1 tiles of 4 x 2 CTUs: rows longer than two CTUs in a tile with tile_x0 > 0 (the save after the tile's
    second CTU is not the row's end, the row wait counts x inside the tile)"""
    e = emulate(tiles_emu, wide_frame(pkg), WIDE_QP, WIDE_TILES, wpp)
    assert assert_picture_equal(wide_reference(pkg, wpp), bytes(e["out"]), e["rec"], e["states"]) == 1


def _same_ctus(a, b):
    """field by field (the padding of the records is not written)"""
    dt = np.dtype(hmo_py.Ctu)
    x, y = np.frombuffer(bytes(a), dt), np.frombuffer(bytes(b), dt)
    return len(x) == len(y) and all(np.array_equal(x[n], y[n]) for n in dt.names)


def test_a_1x1_grid_equals_the_existing_one_slice_paths(tiles_emu, wpp_emu, pkg):
    f = i_frame(pkg)
    plain = emu_py.EmuEncoder(*f, 27)
    plain.compress_frame()
    e = emulate(tiles_emu, f, 27, (1, 1), False)
    assert _same_ctus(e["out"], plain.out)
    for p, q in zip(e["rec"], plain.rec):
        assert np.array_equal(p, q)
    ctx, frac = plain.cabac(full=True)
    assert np.array_equal(e["states"][0][0], ctx) and e["states"][0][1] == frac
    w = wpp_testlib.emulate(wpp_emu, f, 27)
    ew = emulate(tiles_emu, f, 27, (1, 1), True)
    assert _same_ctus(ew["out"], w["out"])
    for p, q in zip(ew["rec"], w["rec"]):
        assert np.array_equal(p, q)
    for (c1, f1), (c2, f2) in zip(ew["states"], w["states"]):
        assert np.array_equal(c1, c2) and f1 == f2


@pytest.mark.parametrize("wpp", [False, True], ids=["tile_chains", "wpp_in_tiles"])
@pytest.mark.parametrize("name", list(P_CASES))
def test_emulated_tiles_of_a_p_picture_are_bit_exact(tiles_emu, pkg, name, wpp):
    ref = p_reference(pkg, name, wpp)
    f, qp, p = p_inputs(pkg, name)
    e = emulate(tiles_emu, f, qp, P_CASES[name][2], wpp, p=p)
    assert e["rbw"] == 0, "a TZ search read a start vector the row had neither written nor inherited"
    skipped = assert_picture_equal(ref, bytes(e["out"]), e["rec"], e["states"], e["mvs"], sorted_ctx=st.O_SORTED)
    assert skipped == 1


def test_binder_refuses_slices_tmvp_across_columns_and_empty_tiles(tiles_emu, pkg):
    f = [np.ascontiguousarray(a) for a in pkg.synth.mixed(256, 128, seed=9)]          # 4 x 2 CTUs
    rec = [np.zeros_like(a) for a in f]
    out = (hmo_py.Ctu * 8)()
    pad = emu_py.pad_planes(f)
    ptrs = (C.c_void_p * 3)(*[a.ctypes.data for a in pad])
    pocs, crp = np.array([0], np.int32), np.array([-1], np.int32)

    def create(cols, rows, wpp, fp_slice_ctus=0, tmvp=None):
        pargs = I_PICTURE if tmvp is None else [1, 30.0, 8, 1, 0, 0, ptrs, pocs.ctypes.data, 1, crp.ctypes.data, 1, None, tmvp]
        hd = tiles_emu.tiles_emu_create(256, 128, 32, cols, rows, wpp, fp_slice_ctus, -1, *[a.ctypes.data for a in f], *[a.ctypes.data for a in rec], C.addressof(out), *pargs)
        if hd:
            n = tiles_emu.tiles_emu_n(hd)
            tiles_emu.tiles_emu_destroy(hd)
            return n
        return None

    assert create(2, 2, 0) == 4 and create(2, 2, 1) == 4 and create(4, 1, 1) == 8 and create(2, 1, 0, tmvp=0) == 2
    assert create(1, 2, 0, tmvp=1) == 2                       # TMVP with tile rows only is allowed
    for wpp in (0, 1):
        assert create(2, 1, wpp, tmvp=1) is None              # tmvp = 1 with two columns
        assert create(2, 2, wpp, fp_slice_ctus=4) is None     # tiles together with SliceMode 1
        assert create(5, 1, wpp) is None and create(1, 3, wpp) is None and create(0, 1, wpp) is None      # an empty tile


def test_drivers_refuse_sao_and_slices_with_tiles(pkg):
    for make in (lambda **kw: pkg.sequence.SequenceDecider(256, 192, 32, **kw), lambda **kw: pkg.lowdelay.LowDelayPDecider(256, 192, 32, **kw)):
        with pytest.raises(ValueError, match="sao"):
            make(tiles=(2, 2), sao=True)
        with pytest.raises(ValueError, match="tiles"):
            make(tiles=(2, 2), slice_ctus=4)
        with pytest.raises(ValueError, match="tiles"):
            make(tiles=(2, 2), wpp=True, slice_rows=1)
        with pytest.raises(ValueError, match="empty"):
            make(tiles=(5, 1))
    with pytest.raises(ValueError, match="tmvp"):
        pkg.lowdelay.LowDelayPDecider(256, 192, 32, tiles=(2, 1), tmvp=True)
