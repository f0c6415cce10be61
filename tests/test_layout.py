"""PictureLayout: the argument rules and the derived numbers of a picture cut into chains (host arithmetic, no GPU).
The expected values are written out by hand from the formulas the two drivers held before the layout existed."""
import pytest

# (width, height) -> configuration -> (chains, bind_slice_ctus, sao_slice_ctus, launch_ctus, uses_wpp_launch, slice mode)
ONE, WF = "SliceMode 0 (one slice per picture)", ", WaveFrontSynchro"
CASES = {
    (256, 192): [                                               # 4 x 3 CTUs
        (dict(), (1, 0, 0, 12, False, ONE)),
        (dict(slice_ctus=4), (3, 4, 4, 4, False, "SliceMode 1, SliceArgument 4")),
        (dict(slice_ctus=5), (3, 5, 5, 5, False, "SliceMode 1, SliceArgument 5")),      # slices of 5, 5 and 2 CTUs
        (dict(wpp=True), (3, 0, 0, 12, True, ONE + WF)),
        (dict(wpp=True, slice_rows=2), (3, 0, 8, 12, True, "SliceMode 1, SliceArgument 8" + WF)),      # slices of 2 rows and 1 row
        (dict(tiles=(2, 2)), (4, 0, 0, 12, False, ONE + ", 2 x 2 uniform tiles")),
        (dict(tiles=(3, 1), wpp=True), (9, 0, 0, 12, True, ONE + ", 3 x 1 uniform tiles" + WF)),
    ],
    (320, 128): [                                               # 5 x 2 CTUs
        (dict(), (1, 0, 0, 10, False, ONE)),
        (dict(slice_ctus=4), (3, 4, 4, 4, False, "SliceMode 1, SliceArgument 4")),      # 4, 4 and 2 CTUs
        (dict(slice_ctus=5), (2, 5, 5, 5, False, "SliceMode 1, SliceArgument 5")),
        (dict(wpp=True), (2, 0, 0, 10, True, ONE + WF)),
        (dict(wpp=True, slice_rows=2), (2, 0, 10, 10, True, "SliceMode 1, SliceArgument 10" + WF)),
        (dict(tiles=(2, 2)), (4, 0, 0, 10, False, ONE + ", 2 x 2 uniform tiles")),
        (dict(tiles=(3, 1), wpp=True), (6, 0, 0, 10, True, ONE + ", 3 x 1 uniform tiles" + WF)),
    ],
}


@pytest.mark.parametrize("size", sorted(CASES))
def test_derived_numbers_and_slice_mode(built, pkg, size):
    w_ctu, h_ctu = (size[0] + 63) // 64, (size[1] + 63) // 64
    for kw, want in CASES[size]:
        lo = pkg.layout.PictureLayout(*size, **kw)
        assert (lo.w_ctu, lo.h_ctu, lo.n_ctu) == (w_ctu, h_ctu, w_ctu * h_ctu)
        assert (lo.chains, lo.bind_slice_ctus, lo.sao_slice_ctus, lo.launch_ctus, lo.uses_wpp_launch, lo.describe()) == want, kw
        assert lo.lf_cross_tiles == 1                           # None resolves to HM's default
        if lo.tiles is not None and lo.wpp:                     # one chain per CTU row of every tile
            cb, rb = pkg.engine.tile_grid(w_ctu, h_ctu, *lo.tiles)
            assert lo.chains == sum(rb[r + 1] - rb[r] for r in range(lo.tiles[1]) for _ in range(lo.tiles[0]))


def test_a_slice_as_long_as_the_picture_is_one_slice(pkg):
    for sl in (12, 13, 100):
        lo = pkg.layout.PictureLayout(256, 192, slice_ctus=sl)
        assert (lo.chains, lo.bind_slice_ctus, lo.sao_slice_ctus, lo.launch_ctus, lo.describe()) == (1, 0, 0, 12, ONE)


def test_the_flag_is_kept_as_given(built, pkg):
    for flag in (0, 1):
        assert pkg.layout.PictureLayout(256, 192, tiles=(2, 2), lf_cross_tiles=flag, sao=True).lf_cross_tiles == flag
    assert pkg.layout.PictureLayout(256, 192, tiles=(1, 2), tmvp=True).chains == 2      # TMVP with tile rows only is allowed


@pytest.mark.parametrize("kw, match", [
    (dict(tiles=(2, 2), slice_ctus=4), "tiles need one slice"),
    (dict(tiles=(2, 2), wpp=True, slice_rows=1), "tiles need one slice"),
    (dict(tiles=(2, 2), lf_cross_tiles=2), "lf_cross_tiles .* is 0 or 1"),
    (dict(tiles=(2, 2), sao=True), "sao=True together with tiles needs lf_cross_tiles"),
    (dict(tiles=(2, 1), tmvp=True), "tmvp together with tile columns"),
    (dict(lf_cross_tiles=0), "lf_cross_tiles is the loop filters' flag .* needs tiles"),
    (dict(wpp=True, slice_ctus=8), "wpp needs one slice per picture"),
    (dict(slice_rows=2), "slice_rows .* needs wpp=True"),
    (dict(wpp=True, slice_rows=0), "slice_rows must be at least 1"),
])
def test_every_rule(pkg, kw, match):
    with pytest.raises(ValueError, match="^SomeCaller: " + match):
        pkg.layout.PictureLayout(256, 192, who="SomeCaller", **kw)
    with pytest.raises(ValueError, match="^(?!SomeCaller)" + match.split(" ")[0]):      # no prefix without `who`
        pkg.layout.PictureLayout(256, 192, **kw)


def test_an_empty_tile_is_refused_by_the_grid(built, pkg):
    for tiles in ((5, 1), (1, 4), (0, 1)):
        with pytest.raises(ValueError, match="empty"):
            pkg.layout.PictureLayout(256, 192, tiles=tiles, who="SomeCaller")


def test_the_layout_needs_no_torch():
    import ast
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fast-cu-decision-hevc_amd", "layout.py")).read()
    names = [a.name for n in ast.walk(ast.parse(src)) if isinstance(n, ast.Import) for a in n.names] + \
            [n.module for n in ast.walk(ast.parse(src)) if isinstance(n, ast.ImportFrom)]
    assert names == ["engine"]                                  # tile_grid, host arithmetic of libfcu.so
