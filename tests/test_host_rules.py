"""The host state machine of libfcu.so (HostState, csrc/fcu_host.h) on the CPU: the argument and state rules of the chain entry
points, the picture binder and the guards of the two launches, through the test-only driver tests/emu/host_emu.cpp (built by
__graft_entry__.build()).  The library's entry points call the same functions first and go to the device only after them, so a
code asserted here is the code the entry point returns; the GPU tests named below keep asserting them on the library itself.
A launch is the guard plus, where it accepts, the driver's "mark as launched"."""
import ctypes as C
import os

import pytest

ARG, STATE = -2, -4
CHAIN, WPP, WPP_P, SLICES, TILES, WPP_TILES = range(6)          # host_emu_begin's `kind`
_P = C.c_void_p
SIGNATURES = {
    "create": ([C.c_int] * 3, _P), "destroy": ([_P], None), "error": ([_P], C.c_char_p), "position": ([_P, C.c_int], C.c_int),
    "bound_chains": ([_P], C.c_int), "begin": ([_P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int], C.c_int),
    "set_range": ([_P] + [C.c_int] * 3, C.c_int), "set_references": ([_P, C.c_int, C.c_int, C.c_int, _P, C.c_int], C.c_int),
    "set_collocated_pocs": ([_P, C.c_int, C.c_int, _P, C.c_int], C.c_int), "set_collocated": ([_P, C.c_int, C.c_int], C.c_int),
    "chains_check": ([_P] + [C.c_int] * 3, C.c_int), "wpp_check": ([_P] + [C.c_int] * 2, C.c_int),
    "chains_launched": ([_P] + [C.c_int] * 3, None), "wpp_launched": ([_P] + [C.c_int] * 2, None),
    "compress_ctu": ([_P, C.c_int, C.c_uint], C.c_int),
}


@pytest.fixture(scope="module")
def emu(built):
    lib = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu", "libhost_emu.so"))
    for name, (argtypes, restype) in SIGNATURES.items():
        f = getattr(lib, "host_emu_" + name)
        f.argtypes, f.restype = argtypes, restype
    return lib


class Host:
    """one context: the calls named after the entry points they stand for"""

    def __init__(self, lib, w, h, max_chains):
        self.lib, self.h = lib, lib.host_emu_create(w, h, max_chains)
        assert self.h

    def begin(self, kind, first, fp, a=0, b=0, pic=0):
        return self.lib.host_emu_begin(self.h, kind, first, C.byref(fp), a, b, pic)

    def compress_chains(self, first, n, ctus):
        rc = self.lib.host_emu_chains_check(self.h, first, n, ctus)
        if rc == 0:
            self.lib.host_emu_chains_launched(self.h, first, n, ctus)
        return rc

    def wpp_check(self, first, n):
        return self.lib.host_emu_wpp_check(self.h, first, n)

    def compress_wpp(self, first, n):
        rc = self.wpp_check(first, n)
        if rc == 0:
            self.lib.host_emu_wpp_launched(self.h, first, n)
        return rc

    def set_reference(self, chain, tag=10):                     # fcu_chain_set_reference: one picture, POC 0 seen from POC 1
        return self.set_references(chain, tag, (0,), 1)

    def set_references(self, chain, tag, pocs, cur_poc):
        return self.lib.host_emu_set_references(self.h, chain, len(pocs), tag, (C.c_int * len(pocs))(*pocs), cur_poc)

    def set_collocated_pocs(self, chain, col_poc, pocs):
        return self.lib.host_emu_set_collocated_pocs(self.h, chain, col_poc, (C.c_int * len(pocs))(*pocs), len(pocs))

    def __getattr__(self, name):                                # set_range, set_collocated, compress_ctu, position, bound_chains, error
        f = getattr(self.lib, "host_emu_" + name)
        return lambda *a: f(self.h, *a)

    def close(self):
        self.lib.host_emu_destroy(self.h)


def i_params(pkg, qp=32):
    fp = pkg.engine.FrameParams()
    pkg.engine.load_lib().fcu_default_frame_params(C.byref(fp), qp)
    return fp


def test_wpp_argument_checks(emu, pkg):
    """tests/test_gpu_wpp.py::test_argument_checks, call for call"""
    H = Host(emu, 192, 128, 3)
    fp = pkg.engine.ldp_slice(32, 1)
    fp.slice_ctus = 0
    assert H.begin(WPP, 0, fp) == ARG and b"fcu_wpp_begin:" in H.error()       # a P slice
    fp = i_params(pkg)
    fp.slice_ctus = 3
    assert H.begin(WPP, 0, fp) == ARG                           # WPP with SliceMode 1
    fp.slice_ctus = 0
    assert H.begin(WPP, 2, fp) == ARG                           # too few chains left for two rows
    assert H.begin(WPP, 0, fp) == 0 and H.bound_chains() == 2
    assert H.compress_chains(0, 2, 3) == STATE                  # row chains belong to fcu_compress_wpp
    assert H.compress_ctu(0, 0) == STATE
    assert H.compress_wpp(1, 1) == STATE                        # not a whole picture
    assert H.begin(CHAIN, 2, fp) == 0
    assert H.compress_wpp(2, 1) == STATE                        # a plain chain
    assert H.compress_wpp(0, 2) == 0
    assert H.compress_wpp(0, 2) == STATE and b"already decided" in H.error()
    H.close()


def test_wpp_slices_argument_and_state_checks(emu, pkg):
    """the refusal block of tests/test_gpu_wpp_slices.py::test_argument_and_state_checks, call for call"""
    H = Host(emu, 192, 192, 7)                                  # W = 3, H = 3
    fp = i_params(pkg)
    for fp.slice_ctus in (4, 3, 7):
        assert H.begin(SLICES, 0, fp, 2) == ARG, fp.slice_ctus  # a slice that starts mid-row / a length that is not slice_rows x W
    fp.slice_ctus = 0
    assert H.begin(SLICES, 0, fp, 0) == ARG and H.begin(SLICES, 0, fp, -1) == ARG      # slice_rows below one
    assert H.begin(SLICES, 5, fp, 2) == ARG and H.begin(SLICES, -1, fp, 2) == ARG      # too few chains left for three rows
    fp.slice_ctus = 6
    assert H.begin(WPP, 0, fp) == ARG                           # the one-slice entry points keep rejecting slice_ctus
    assert H.begin(SLICES, 0, fp, 2) == 0                       # slice_ctus exactly slice_rows x W
    fp.slice_ctus = 0
    assert H.begin(SLICES, 0, fp, 2) == 0 and H.begin(SLICES, 3, fp, 1, pic=1) == 0    # two pictures: chains 0..2 and 3..5
    assert H.compress_chains(0, 3, 3) == STATE                  # row chains belong to fcu_compress_wpp
    assert H.set_range(2, 6, 3) == STATE
    assert H.compress_wpp(0, 2) == STATE                        # a partial picture: ends before the last row
    assert H.compress_wpp(2, 1) == STATE                        # ... starts at the first row of a later slice, not of the picture
    assert H.compress_wpp(1, 2) == STATE
    assert H.compress_wpp(4, 2) == STATE                        # (R = 1: every row starts a slice, still not a picture start)
    assert H.begin(CHAIN, 6, fp) == 0
    assert H.compress_wpp(3, 4) == STATE                        # a plain chain in the range
    assert H.compress_wpp(0, 6) == 0                            # both pictures
    assert [H.position(k) for k in range(6)] == [3, 6, 9, 3, 6, 9]
    assert H.compress_wpp(0, 3) == STATE                        # already decided
    fpp = pkg.engine.ldp_slice(32, 1)                           # a P row without a reference picture
    fpp.tmvp = 0
    assert H.begin(SLICES, 0, fpp, 2) == 0
    assert H.set_reference(0) == 0 and H.set_reference(1) == 0
    assert H.compress_wpp(0, 3) == STATE                        # row 2 (a slice of its own) still without one
    assert H.set_reference(2) == 0
    assert H.compress_wpp(0, 3) == 0
    H.close()


def test_tiles_argument_and_state_checks(emu, pkg):
    """tests/test_gpu_tiles.py::test_argument_and_state_checks, call for call"""
    H = Host(emu, 192, 136, 6)
    fp = i_params(pkg)
    for kind in (TILES, WPP_TILES):
        assert H.begin(kind, 0, fp, 4, 1) == ARG and H.begin(kind, 0, fp, 1, 4) == ARG      # an empty tile
        assert H.begin(kind, 0, fp, 0, 1) == ARG
        fp.slice_ctus = 3
        assert H.begin(kind, 0, fp, 2, 2) == ARG                # tiles together with SliceMode 1
        fp.slice_ctus = 0
        fp.slice_type, fp.lambda_, fp.tmvp = 1, 30.0, 1
        assert H.begin(kind, 0, fp, 2, 1) == ARG                # TMVP across tile columns
        assert H.begin(kind, 0, fp, 1, 2) == 0                  # ... tile rows only: allowed
        fp.slice_type, fp.lambda_, fp.tmvp = 0, 0.0, 0
    assert H.begin(TILES, 3, fp, 2, 2) == ARG                   # 4 chains from 3: too few
    assert H.begin(WPP_TILES, 1, fp, 2, 2) == ARG               # 6 chains from 1: too few
    assert H.begin(TILES, 0, fp, 2, 2) == 0 and H.bound_chains() == 4
    assert H.set_range(1, 0, 9) == STATE                        # a tile chain keeps its tile
    assert H.compress_wpp(0, 4) == STATE                        # tile chains are advanced by fcu_compress_chains
    assert H.begin(WPP_TILES, 0, fp, 2, 2) == 0 and H.bound_chains() == 6
    assert H.compress_chains(0, 6, 9) == STATE                  # row chains are decided by fcu_compress_wpp
    assert H.compress_wpp(0, 5) == STATE                        # the range must end with the picture's last tile
    assert H.compress_wpp(1, 5) == STATE                        # ... and start with its first
    assert H.compress_wpp(0, 6) == 0
    assert H.compress_wpp(0, 6) == STATE                        # already decided
    H.close()


def test_chain_range_must_follow_slices(emu, pkg):
    """the set_range lines of tests/test_gpu_parity.py: the refusals of test_chain_range_must_follow_slices, the slice chains
    of test_4k_slices_at_other_qps; and the order of fcu_chain_set_range's checks: state before range"""
    H = Host(emu, 256, 128, 2)
    fp = i_params(pkg)
    fp.slice_ctus = 4
    assert H.set_range(0, 2, 4) == STATE                        # not bound (the range is wrong too: the state check comes first)
    assert H.set_range(2, 0, 4) == ARG
    assert H.begin(CHAIN, 0, fp) == 0
    assert H.set_range(0, 2, 4) == ARG                          # does not start at a slice boundary
    assert H.set_range(0, 4, 3) == ARG                          # does not end at one
    assert H.set_range(0, 4, 4) == 0 and H.position(0) == 4
    assert H.compress_ctu(0, 3) == STATE and H.compress_ctu(0, 4) == 0 and H.position(0) == 5      # raster order from the range's start
    H.close()
    H, sl, rows = Host(emu, 3840, 2160, 6), 60, 6
    fp.slice_ctus = sl
    for k in range(rows):
        assert H.begin(CHAIN, k, fp) == 0 and H.set_range(k, k * sl, sl) == 0
    assert H.compress_chains(0, rows, sl) == 0 and [H.position(k) for k in range(rows)] == [(k + 1) * sl for k in range(rows)]
    H.close()


def _accepted_ranges(H, n):
    return [(a, b) for a in range(n) for b in range(a + 1, n + 1) if H.wpp_check(a, b - a) == 0]


def _all_refusals_are_state(H, n):
    return all(H.wpp_check(a, b - a) in (0, STATE) for a in range(n) for b in range(a + 1, n + 1))


def test_two_pictures_back_to_back(emu, pkg):
    H = Host(emu, 192, 128, 4)                                  # two rows per picture
    fp = i_params(pkg)
    assert H.begin(WPP, 0, fp, pic=0) == 0 and H.begin(WPP, 2, fp, pic=1) == 0
    assert _accepted_ranges(H, 4) == [(0, 2), (0, 4), (2, 4)] and _all_refusals_are_state(H, 4)      # every other range splits a picture
    H.close()


def test_rows_inside_tiles(emu, pkg):
    H = Host(emu, 192, 192, 12)                                 # 3 x 3 CTUs, 2 x 2 tiles: six chains per picture
    fp = i_params(pkg)
    assert H.begin(WPP_TILES, 0, fp, 2, 2, pic=0) == 0 and H.bound_chains() == 6
    assert H.wpp_check(0, 5) == STATE and H.wpp_check(1, 5) == STATE and H.wpp_check(0, 6) == 0
    assert H.begin(WPP_TILES, 6, fp, 2, 2, pic=1) == 0
    assert _accepted_ranges(H, 12) == [(0, 6), (0, 12), (6, 12)] and _all_refusals_are_state(H, 12)
    assert H.compress_wpp(0, 12) == 0                           # two such pictures in a row
    assert H.begin(WPP_TILES, 0, fp, 2, 2) == 0 and H.begin(WPP, 3, fp, pic=1) == 0      # a row picture over the first picture's last three chains
    assert _accepted_ranges(H, 6) == [(3, 6)] and _all_refusals_are_state(H, 6)           # what is left of the first is no picture
    H.close()


def test_the_rows_of_a_p_picture_name_the_same_references(emu, pkg):
    H = Host(emu, 192, 192, 3)
    fp = pkg.engine.ldp_slice(32, 4)
    fp.tmvp = 1
    assert fp.slice_type == 1 and H.begin(WPP_P, 0, fp) == 0

    def name(row, tag=10, pocs=(3, 2), col_pocs=(2, 1), col=20):
        assert H.set_references(row, tag, pocs, 4) == 0 and H.set_collocated_pocs(row, pocs[0], col_pocs) == 0 and H.set_collocated(row, col) == 0

    assert H.wpp_check(0, 3) == STATE and b"without reference" in H.error()
    name(0), name(1)
    assert H.wpp_check(0, 3) == STATE and b"without reference" in H.error()    # row 2 still has none
    name(2)
    assert H.wpp_check(0, 3) == 0                               # identical on all rows
    for row, other in ((1, dict(tag=11)), (2, dict(pocs=(3, 1))), (1, dict(col=21)), (2, dict(col_pocs=(2, 0))), (1, dict(col=-1))):
        name(row, **other)                                      # another plane pointer / POC list / collocated field than row 0
        assert H.wpp_check(0, 3) == STATE and b"different reference pictures or collocated fields" in H.error(), other
        name(row)
        assert H.wpp_check(0, 3) == 0
    H.close()


def test_rebinding_a_middle_chain_breaks_the_picture(emu, pkg):
    H = Host(emu, 192, 192, 3)
    fp = i_params(pkg)
    assert H.begin(WPP, 0, fp) == 0 and H.wpp_check(0, 3) == 0
    assert H.begin(CHAIN, 1, fp) == 0                           # fcu_chain_begin on row 1: a plain chain now
    assert H.wpp_check(0, 3) == STATE and H.wpp_check(0, 1) == STATE and H.wpp_check(2, 1) == STATE
    assert H.begin(WPP, 0, fp) == 0 and H.wpp_check(0, 3) == 0  # bound again
    H.close()


def test_sweep_of_small_pictures(emu, pkg):
    """Every cut of pictures of 1..4 x 1..4 CTUs.  The binder fills as many chains as PictureLayout counts, and where rows are
    chains (a row waits on the chain its descriptor names) the WaveFrontSynchro guard accepts the full range [0, chains) and no
    other sub-range [a, b).  One chain per tile: the chains are independent, fcu_compress_chains takes any sub-range of them and
    fcu_compress_wpp none."""
    Layout = pkg.layout.PictureLayout
    fp = i_params(pkg)
    for W in range(1, 5):
        for Hc in range(1, 5):
            w, h = 64 * W, 64 * Hc
            H = Host(emu, w, h, 16)
            cuts = [(WPP, 0, 0, dict(wpp=True))] + [(SLICES, R, 0, dict(wpp=True, slice_rows=R)) for R in range(1, Hc + 1)]
            cuts += [(WPP_TILES if wpp else TILES, nc, nr, dict(tiles=(nc, nr), wpp=bool(wpp))) for nc in range(1, W + 1) for nr in range(1, Hc + 1) for wpp in (0, 1)]
            for kind, a, b, kw in cuts:
                assert H.begin(kind, 0, fp, a, b) == 0, (W, Hc, kw)
                n = H.bound_chains()
                assert n == Layout(w, h, **kw).chains, (W, Hc, kw)
                assert _accepted_ranges(H, n) == ([(0, n)] if kw["wpp"] else []) and _all_refusals_are_state(H, n), (W, Hc, kw)
                if not kw["wpp"]:
                    assert all(emu.host_emu_chains_check(H.h, s, e - s, 1) == 0 for s in range(n) for e in range(s + 1, n + 1)), (W, Hc, kw)
            H.close()
