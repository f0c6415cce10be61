"""Loop filters of a picture of slices on the CPU: what pins the slice reference of tests/lf_slice_oracle.py (the six points of its
docstring), the slice variants of the kernel source on the emulator (tests/emu/lf_slices_emu.cpp) against that reference for
every slice length x LFCrossSliceBoundaryFlag x slice type, the same independence on the emulator, and the argument rules of the
host, of PictureLayout and of the two drivers.  Every comparison is exact."""
import numpy as np
import pytest

import hmo_py
import lf_slice_oracle as L
import test_sao as T
from lf_slice_oracle import lf_emu  # noqa: F401 (fixture)
from wpp_testlib import CTU_DT

ALL = L.CUTS + L.ONE
CASES = [(s, c) for s in ALL for c in (0, 1)]
IDS = ["slice%d_cross%d" % (s, c) for s, c in CASES]
same = lambda a, b: all(np.array_equal(p, q) for p, q in zip(a, b))


def inside(planes, slice_ctus, s):
    """the samples of slice s, per plane"""
    return [p[L.slice_map(L.W, L.H, slice_ctus, comp) == s] for comp, p in enumerate(planes)]


# ---- 1. one slice, or the flag 1: the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("slice_ctus,cross", [(s, 1) for s in ALL] + [(s, 0) for s in L.ONE], ids=lambda v: str(v))
def test_reference_with_one_slice_or_crossing_is_the_oracle(pkg, built, slice_ctus, cross):
    d = L.decided(pkg, slice_ctus)
    want = [p.copy() for p in d.rec]
    hmo_py.deblock_pic(d.ctus, L.W, L.H, want)
    got = L.deblock_slices(d.ctus, L.W, L.H, d.rec, slice_ctus, cross)
    assert same(got, want) and not same(got, d.rec)
    for slice_type in L.SLICE_TYPES:
        a, b = [p.copy() for p in want], [p.copy() for p in want]
        w = hmo_py.sao_picture(d.frame, a, L.QP, slice_type, L.LAMBDA, slice_ctus=slice_ctus, want_stats=True)
        g = L.sao_slices(d.frame, b, L.QP, slice_type, L.LAMBDA, slice_ctus, cross)
        assert np.array_equal(g[0], w[0]) and g[1] == w[1] and np.array_equal(g[2], w[2])
        assert same(a, b) and not same(a, want), "SAO changed nothing: the case shows nothing"


# ---- 2. slices of whole CTU rows: the oracle on every slice's crop -----------------------------------------------------------
@pytest.mark.parametrize("slice_ctus", L.ROW_CUTS)
def test_reference_without_crossing_is_the_oracle_on_each_row_slices_crop(pkg, built, slice_ctus):
    d, r = L.decided(pkg, slice_ctus), L.filtered(pkg, slice_ctus, 0, hmo_py.SLICE_I)
    assert same(r["dbk"], L.deblock_stitched(d.ctus, L.W, L.H, d.rec, slice_ctus))
    Wc, Hc = L.dims(L.W, L.H)
    compared = 0
    for first, end in L.slice_ranges(L.W, L.H, slice_ctus):
        y0, y1 = first // Wc, end // Wc
        org, rec = L.crop_rows(d.frame, y0, y1, L.H), L.crop_rows(r["dbk"], y0, y1, L.H)
        _, _, stats = hmo_py.sao_picture(org, rec, L.QP, hmo_py.SLICE_I, L.LAMBDA, want_stats=True)
        rows = [y for y in range(y0, y1) if y + 1 < y1 or y1 == Hc]      # not the slice's last CTU row, unless it is the picture's
        for y in rows:
            assert np.array_equal(r["stats"][y * Wc:(y + 1) * Wc], stats[(y - y0) * Wc:(y - y0 + 1) * Wc]), (first, y)
        compared += len(rows)
    assert compared == {4: 1, 8: 2}[slice_ctus]


# ---- 3. slice independence: the definition of the flag -----------------------------------------------------------------------
def _independence(pkg, slice_ctus, deblock, stats_of, apply):
    d, r = L.decided(pkg, slice_ctus), L.filtered(pkg, slice_ctus, 0, hmo_py.SLICE_I)
    dbk = deblock(d.ctus, d.rec)
    assert same(dbk, r["dbk"])
    stats = stats_of(d.frame, dbk)
    recons = [L.all_new_params(L.N_CTU, t, 40 + t) for t in range(5)]
    applied = [apply(dbk, rc) for rc in recons]
    for s, (first, end) in enumerate(L.slice_ranges(L.W, L.H, slice_ctus)):
        noisy = L.randomised_outside(d.rec, L.W, L.H, slice_ctus, s, 1000 + s)
        assert same(inside(deblock(d.ctus, noisy), slice_ctus, s), inside(dbk, slice_ctus, s)), ("deblocking", s)
        noisy = L.randomised_outside(dbk, L.W, L.H, slice_ctus, s, 2000 + s)
        assert np.array_equal(stats_of(d.frame, noisy)[first:end], stats[first:end]), ("statistics", s)
        for t, rc in enumerate(recons):
            assert same(inside(apply(noisy, rc), slice_ctus, s), inside(applied[t], slice_ctus, s)), ("offset pass", s, t)
    # not vacuous: with the flag 1 the same noise reaches into a slice
    noisy = L.randomised_outside(d.rec, L.W, L.H, slice_ctus, 0, 1000)
    assert not same(inside(L.deblock_slices(d.ctus, L.W, L.H, noisy, slice_ctus, 1), slice_ctus, 0), inside(L.deblock_slices(d.ctus, L.W, L.H, d.rec, slice_ctus, 1), slice_ctus, 0))


@pytest.mark.parametrize("slice_ctus", L.CUTS)
def test_reference_slices_are_independent_without_crossing(pkg, built, slice_ctus):
    _independence(pkg, slice_ctus,
                  lambda ctus, rec: L.deblock_slices(ctus, L.W, L.H, rec, slice_ctus, 0),
                  lambda org, dbk: L.sao_slices(org, [p.copy() for p in dbk], L.QP, hmo_py.SLICE_I, L.LAMBDA, slice_ctus, 0)[2],
                  lambda dbk, rc: L.sao_apply_slices(dbk, rc, slice_ctus, 0))


@pytest.mark.parametrize("slice_ctus", L.CUTS)
def test_emulated_slices_are_independent_without_crossing(pkg, lf_emu, slice_ctus):
    _independence(pkg, slice_ctus,
                  lambda ctus, rec: L.emu_deblock(lf_emu, ctus, L.W, L.H, rec, slice_ctus, 0),
                  lambda org, dbk: L.emu_sao(lf_emu, org, [p.copy() for p in dbk], L.QP, hmo_py.SLICE_I, L.LAMBDA, slice_ctus, 0)[2],
                  lambda dbk, rc: L.emu_apply(lf_emu, dbk, rc, slice_ctus, 0))


# ---- 4. locality -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slice_ctus", L.CUTS)
def test_the_flag_changes_deblocked_samples_next_to_the_slice_boundary_line_only(pkg, built, slice_ctus):
    d = L.decided(pkg, slice_ctus)
    a, b = L.deblock_slices(d.ctus, L.W, L.H, d.rec, slice_ctus, 0), L.deblock_slices(d.ctus, L.W, L.H, d.rec, slice_ctus, 1)
    Wc, _ = L.dims(L.W, L.H)
    both_sides = False
    for comp, (p, q) in enumerate(zip(a, b)):
        sh, reach = L.SHIFT[comp], 2 if comp else 4
        near, diff = np.zeros(p.shape, bool), p != q
        ph, pw = p.shape
        for addr in range(L.N_CTU):
            v = L.slice_avail8(addr, L.W, L.H, slice_ctus)
            x0, y0 = (addr % Wc * 64) >> sh, (addr // Wc * 64) >> sh
            x1, y1 = min(x0 + (64 >> sh), pw), min(y0 + (64 >> sh), ph)
            if addr % Wc and not v["L"]:                                  # the segment x = x0, y0 <= y < y1
                near[max(y0 - reach, 0):y1 + reach, x0 - reach:x0 + reach] = True
                both_sides |= bool(diff[y0:y1, x0 - reach:x0].any() and diff[y0:y1, x0:x0 + reach].any())
            if addr >= Wc and not v["A"]:                                 # the segment y = y0, x0 <= x < x1
                near[y0 - reach:y0 + reach, max(x0 - reach, 0):x1 + reach] = True
                both_sides |= bool(diff[y0 - reach:y0, x0:x1].any() and diff[y0:y0 + reach, x0:x1].any())
        assert not (diff & ~near).any(), ("the flag changed a sample away from the slice boundary line", comp)
    assert both_sides, "no slice edge with a changed sample on both of its sides: the case shows nothing"


# ---- 5. the offset pass against the specification's per-sample rule ----------------------------------------------------------
@pytest.mark.parametrize("slice_ctus,cross", [(s, 0) for s in ALL] + [(5, 1)], ids=lambda v: str(v))
def test_reference_offset_pass_is_the_specifications_sample_rule(pkg, built, slice_ctus, cross):
    dbk = L.filtered(pkg, slice_ctus, cross, hmo_py.SLICE_I)["dbk"]
    for t in range(5):
        rc = L.all_new_params(L.N_CTU, t, 60 + t)
        got, want = L.sao_apply_slices(dbk, rc, slice_ctus, cross), L.sao_apply_spec(dbk, rc, slice_ctus, cross)
        for comp, (p, q) in enumerate(zip(got, want)):
            assert np.array_equal(p, q), (t, comp, np.argwhere(p != q)[:4])
        assert not same(got, dbk)
    r = L.filtered(pkg, slice_ctus, cross, hmo_py.SLICE_I)                # and with the parameters the decision chose
    assert same(L.sao_apply_spec(r["dbk"], r["recon"], slice_ctus, cross), r["rec"])


def test_the_staircase_separates_every_diagonal_from_its_sides(built):
    """slice_ctus 5 on 4 x 3 CTUs, slices {0-4 | 5-9 | 10, 11}: the four cases, by arithmetic"""
    v = {a: L.slice_avail8(a, L.W, L.H, 5) for a in range(L.N_CTU)}
    assert (v[9]["A"], v[9]["L"], v[9]["AL"]) == (1, 1, 0)      # a - W = 5 is the slice's first CTU
    assert (v[8]["A"], v[8]["AR"]) == (0, 1)                    # a - W + 1 = 5 is its first
    assert (v[6]["B"], v[6]["BL"]) == (0, 1)                    # a + W - 1 = 9 is its last
    assert (v[5]["B"], v[5]["R"], v[5]["BR"]) == (1, 1, 0)      # a + W = 9 is its last
    for s in (4, 8, 12, 0):                                     # slices of whole rows: the conjunctions hold
        for a in range(L.N_CTU):
            u = L.slice_avail8(a, L.W, L.H, s)
            assert (u["AL"], u["AR"], u["BL"], u["BR"]) == (u["A"] & u["L"], u["A"] & u["R"], u["B"] & u["L"], u["B"] & u["R"])


# ---- 6. the eight-flag restatement against the oracle's four-flag functions --------------------------------------------------
def test_eight_flag_block_functions_with_conjunctions_are_the_oracles(built):
    lib, rng = L.ref_lib(), np.random.default_rng(5)
    stride, off = 80, 8
    for comp, (w, h) in ((0, (64, 64)), (0, (16, 8)), (1, (32, 32)), (2, (8, 4))):
        src = rng.integers(0, 256, (h + 16, stride), dtype=np.uint8)
        src = (src // 16 * 16 + rng.integers(0, 3, src.shape)).astype(np.uint8)      # plateaus and edges: every class occurs
        org = np.clip(src.astype(np.int16) + rng.integers(-4, 5, src.shape), 0, 255).astype(np.uint8)
        ps, po = src.ctypes.data + off * stride + off, org.ctypes.data + off * stride + off
        for m in range(16):
            Lf, R, A, B = m & 1, (m >> 1) & 1, (m >> 2) & 1, (m >> 3) & 1
            s4, s8 = np.zeros((2, 5, 32), np.int64), np.zeros((2, 5, 32), np.int64)
            lib.lf_ref_blk_stats4(s4.ctypes.data, ps, po, stride, w, h, comp, Lf, R, A, B)
            lib.lf_ref_blk_stats8(s8.ctypes.data, ps, po, stride, w, h, comp, Lf, R, A, B, A & Lf)
            assert np.array_equal(s4, s8) and s4.any(), (comp, m)
            v = (L.C.c_int * 8)(Lf, R, A, B, A & Lf, A & R, B & Lf, B & R)
            for t in range(5):
                offs = np.zeros(32, np.int32)
                offs[:] = rng.integers(-7, 8, 32)
                r4, r8 = src.copy(), src.copy()
                lib.lf_ref_offset_block4(t, offs.ctypes.data, ps, r4.ctypes.data + off * stride + off, stride, w, h, Lf, R, A, B)
                lib.lf_ref_offset_block8(t, offs.ctypes.data, ps, r8.ctypes.data + off * stride + off, stride, w, h, v)
                assert np.array_equal(r4, r8) and not np.array_equal(r4, src), (comp, m, t)


# ---- the kernel source on the emulator ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("slice_ctus,cross", CASES, ids=IDS)
def test_emulated_deblocking_matches_the_reference(pkg, lf_emu, slice_ctus, cross):
    d = L.decided(pkg, slice_ctus)
    assert same(L.emu_deblock(lf_emu, d.ctus, L.W, L.H, d.rec, slice_ctus, cross), L.filtered(pkg, slice_ctus, cross, hmo_py.SLICE_I)["dbk"])


@pytest.mark.parametrize("cross", (0, 1))
@pytest.mark.parametrize("slice_ctus", L.P_CUTS)
def test_emulated_deblocking_of_a_p_picture_matches_the_reference(pkg, lf_emu, slice_ctus, cross):
    d = L.decided_p(pkg, slice_ctus)
    pm = np.frombuffer(d.ctus, CTU_DT)["pred_mode"]
    assert (pm == 0).mean() > 0.5, "the P picture is not mostly inter-predicted"
    want = L.deblock_slices(d.ctus, L.W, L.H, d.rec, slice_ctus, cross)
    assert same(L.emu_deblock(lf_emu, d.ctus, L.W, L.H, d.rec, slice_ctus, cross), want)
    assert not same(want, d.rec)
    if not cross:
        assert not same(want, L.deblock_slices(d.ctus, L.W, L.H, d.rec, slice_ctus, 1)), "the flag changes nothing in the P picture"


def _assert_sao(pkg, got, rec, r):
    coded, off, stats = got
    assert np.array_equal(stats, r["stats"]), "sao_stats"
    assert np.array_equal(T.M.canon(pkg.engine.sao_coded_to_array(coded)), T.M.canon(r["params"])), "sao_cands + sao_decide"
    for k, (p, q) in enumerate(zip(rec, r["rec"])):
        assert np.array_equal(p, q), ("sao_apply", k)
    assert list(off) == r["off"], "off_count"


@pytest.mark.parametrize("slice_type", L.SLICE_TYPES, ids=["I", "P"])
@pytest.mark.parametrize("slice_ctus,cross", CASES, ids=IDS)
def test_emulated_sao_matches_the_reference(pkg, lf_emu, slice_ctus, cross, slice_type):
    r = L.filtered(pkg, slice_ctus, cross, slice_type)
    rec = [p.copy() for p in r["dbk"]]
    _assert_sao(pkg, L.emu_sao(lf_emu, L.frame(pkg), rec, L.QP, slice_type, L.LAMBDA, slice_ctus, cross), rec, r)


@pytest.mark.parametrize("slice_ctus", L.CUTS)
def test_the_flag_changes_the_statistics_and_the_filtered_picture(pkg, built, slice_ctus):
    a, b = L.filtered(pkg, slice_ctus, 0, hmo_py.SLICE_I), L.filtered(pkg, slice_ctus, 1, hmo_py.SLICE_I)
    assert not np.array_equal(a["stats"], b["stats"]) and not same(a["rec"], b["rec"]), "the flag changes nothing: the case shows nothing"


def test_emulated_sao_with_a_component_switched_off(pkg, lf_emu):
    slice_ctus, en = 5, (1, 0, 1)
    r = L.filtered(pkg, slice_ctus, 0, hmo_py.SLICE_P, en)
    assert r["off"][1] == 12 and np.array_equal(r["rec"][1], r["dbk"][1])
    rec = [p.copy() for p in r["dbk"]]
    _assert_sao(pkg, L.emu_sao(lf_emu, L.frame(pkg), rec, L.QP, hmo_py.SLICE_P, L.LAMBDA, slice_ctus, 0, en), rec, r)


@pytest.mark.parametrize("slice_ctus", ALL)
def test_emulated_offset_pass_with_every_type_matches_the_reference(pkg, lf_emu, slice_ctus):
    """the decision rarely picks a diagonal class in every CTU of the staircase: here every CTU and component gets each type"""
    dbk = L.filtered(pkg, slice_ctus, 0, hmo_py.SLICE_I)["dbk"]
    for t in range(5):
        rc = L.all_new_params(L.N_CTU, t, 80 + t)
        assert same(L.emu_apply(lf_emu, dbk, rc, slice_ctus, 0), L.sao_apply_slices(dbk, rc, slice_ctus, 0)), t


# ---- 7. the argument rules ---------------------------------------------------------------------------------------------------
def test_which_kernels_run_and_what_the_host_refuses(lf_emu):
    n = L.C.c_int()
    variant = lambda s, c: lf_emu.lf_slices_emu_variant(L.W, L.H, s, c, L.C.byref(n))
    for s in L.CUTS:
        assert variant(s, 0) == 1 and n.value == s              # the slice variants
        assert variant(s, 1) == 0                               # the flag 1: the kernels without a cut
    for s in (0, 12, 13, 1 << 30):
        assert variant(s, 0) == 0 and n.value == 12             # one slice
    for s, c in ((-1, 0), (-1, 1), (4, 2), (4, -1)):
        assert variant(s, c) == -1


def test_layout_rules_for_the_flag(pkg):
    PL = pkg.layout.PictureLayout
    assert PL(256, 192, slice_ctus=4).lf_cross_slices == 1      # None resolves to HM's default
    assert PL(256, 192).lf_cross_slices == 1
    for flag in (0, 1):
        lo = PL(256, 192, slice_ctus=5, lf_cross_slices=flag)
        assert lo.lf_cross_slices == flag and lo.sao_slice_ctus == 5
        lo = PL(256, 192, wpp=True, slice_rows=2, lf_cross_slices=flag, sao=True)
        assert lo.lf_cross_slices == flag and lo.sao_slice_ctus == 8
    with pytest.raises(TypeError):
        PL(256, 192, 4, False, None, None, None, False, False, "", 0)      # keyword-only
    for kw, msg in ((dict(slice_ctus=4, lf_cross_slices=2), "lf_cross_slices .* is 0 or 1"),
                    (dict(slice_ctus=4, lf_cross_slices=-1), "lf_cross_slices .* is 0 or 1"),
                    (dict(lf_cross_slices=0), "lf_cross_slices is the loop filters' flag .* needs slice_ctus"),
                    (dict(wpp=True, lf_cross_slices=1), "lf_cross_slices is the loop filters' flag .* needs slice_ctus"),
                    (dict(slice_ctus=0, lf_cross_slices=0), "needs slice_ctus"),
                    (dict(tiles=(2, 2), lf_cross_slices=0), "lf_cross_slices .* tiles need one slice"),
                    (dict(tiles=(2, 2), lf_cross_tiles=0, lf_cross_slices=1), "lf_cross_slices .* tiles need one slice")):
        with pytest.raises(ValueError, match=msg):
            PL(256, 192, **kw)
        with pytest.raises(ValueError, match="^who: "):
            PL(256, 192, who="who", **kw)


def test_both_drivers_carry_the_flag(pkg):
    ld, sq = pkg.lowdelay.LowDelayPDecider, pkg.sequence.SequenceDecider
    for make, who in ((lambda **kw: sq(256, 192, 32, **kw), "SequenceDecider"), (lambda **kw: ld(256, 192, 32, **kw), "LowDelayPDecider")):
        with pytest.raises(ValueError, match=who + ": lf_cross_slices .* is 0 or 1"):
            make(slice_ctus=4, lf_cross_slices=2)
        with pytest.raises(ValueError, match=who + ": lf_cross_slices .* needs slice_ctus"):
            make(lf_cross_slices=0)
        with pytest.raises(ValueError, match=who + ": lf_cross_slices .* tiles"):
            make(tiles=(2, 2), lf_cross_slices=0)
        # accepted: the construction gets past the argument rules (without a GPU it ends at the engine, which has no CPU fallback)
        for kw in (dict(slice_ctus=5, lf_cross_slices=0), dict(slice_ctus=5, lf_cross_slices=1), dict(wpp=True, slice_rows=1, lf_cross_slices=0), dict(slice_ctus=5)):
            try:
                d = make(**kw)
            except pkg.engine.FcuError:
                continue
            assert d.lf_cross_slices == kw.get("lf_cross_slices", 1) and d.layout.lf_cross_slices == d.lf_cross_slices
            (d.close if hasattr(d, "close") else d.eng.destroy)()
    with pytest.raises(ValueError, match="sao"):
        sq(256, 192, 32, tiles=(2, 2), sao=True, lf_cross_tiles=0)      # SequenceDecider runs no SAO: unchanged
