"""How one picture is cut into chains: SliceMode 1 slices, WaveFrontSynchro rows, rows inside slices of whole CTU rows,
uniform tiles, rows inside tiles.  `PictureLayout` holds the argument rules of these combinations and the numbers the host
derives from them; `CuEngine.init_picture` / `compress_pictures` / `deblock` / `sao` and the two drivers read it.
Plain host arithmetic: no torch, no GPU, no engine handle, no tensors."""


class PictureLayout:
    """slice_ctus: CTUs per slice (HM's SliceMode 1 / SliceArgument); None or >= the picture = one slice per picture.
    wpp: WaveFrontSynchro -- the CTU rows are chains; slice_rows (with wpp only): slices of slice_rows whole CTU rows.
    tiles=(C, R): one slice cut into C x R uniform tiles, with wpp WaveFrontSynchro inside every tile; lf_cross_tiles (with
    tiles only): LFCrossTileBoundaryFlag of the loop filters, None = 1; sao / tmvp: what the caller runs on such a picture
    (SAO with tiles needs the flag chosen; TMVP cannot cross tile columns).  lf_cross_slices (with slices only: a non-zero
    slice_ctus, or slice_rows): LFCrossSliceBoundaryFlag of the loop filters, None = 1.  who: prefix of the ValueError messages."""

    def __init__(self, width, height, slice_ctus=None, wpp=False, slice_rows=None, tiles=None, lf_cross_tiles=None, sao=False, tmvp=False, who="", *, lf_cross_slices=None):
        def refuse(msg):
            raise ValueError(f"{who}: {msg}" if who else msg)
        self.w_ctu, self.h_ctu = (width + 63) // 64, (height + 63) // 64
        self.n_ctu = self.w_ctu * self.h_ctu
        if tiles is not None:
            if slice_ctus or slice_rows is not None:
                refuse("tiles need one slice per picture (no slice_ctus, no slice_rows)")
            if lf_cross_tiles is not None and lf_cross_tiles not in (0, 1):
                refuse("lf_cross_tiles (LFCrossTileBoundaryFlag) is 0 or 1")
            if sao and lf_cross_tiles is None:
                refuse("sao=True together with tiles needs lf_cross_tiles=0 or 1 (LFCrossTileBoundaryFlag: whether SAO and deblocking reach across the tile boundaries)")
            from .engine import tile_grid                         # host arithmetic of libfcu.so
            tile_grid(self.w_ctu, self.h_ctu, *tiles)             # ValueError for a grid with an empty tile
            if tmvp and tiles[0] > 1:
                refuse("tmvp together with tile columns is not supported (the collocated bottom-right candidate reads across the tile edge)")
        elif lf_cross_tiles is not None:
            refuse("lf_cross_tiles is the loop filters' flag of a picture with tiles and needs tiles=(C, R)")
        if lf_cross_slices is not None:
            if tiles is not None:
                refuse("lf_cross_slices is the loop filters' flag of a picture with slices; tiles need one slice per picture (the tiles' flag: lf_cross_tiles)")
            if lf_cross_slices not in (0, 1):
                refuse("lf_cross_slices (LFCrossSliceBoundaryFlag) is 0 or 1")
            if not slice_ctus and slice_rows is None:
                refuse("lf_cross_slices is the loop filters' flag of a picture with slices and needs slice_ctus, or wpp=True with slice_rows")
        if wpp and slice_ctus:
            refuse("wpp needs one slice per picture (slice_ctus must be None; slices of whole CTU rows: slice_rows)")
        if slice_rows is not None and not wpp:
            refuse("slice_rows cuts a WaveFrontSynchro picture into slices of whole CTU rows and needs wpp=True (without WPP: slice_ctus)")
        if slice_rows is not None and slice_rows < 1:
            refuse("slice_rows must be at least 1")
        self.wpp, self.slice_rows, self.tiles = bool(wpp), slice_rows, tiles
        self.lf_cross_tiles = 1 if lf_cross_tiles is None else lf_cross_tiles
        self.lf_cross_slices = 1 if lf_cross_slices is None else lf_cross_slices
        self.slice_ctus = slice_ctus if slice_ctus else self.n_ctu
        self.n_slices = (self.n_ctu + self.slice_ctus - 1) // self.slice_ctus      # SliceMode 1 slices (1 with wpp and with tiles)
        sliced = self.n_slices > 1
        if tiles is not None:
            self.chains = tiles[0] * (self.h_ctu if wpp else tiles[1])             # fcu_tile_chains
        else:
            self.chains = self.h_ctu if wpp else self.n_slices                     # chains per picture: rows (WPP) or slices
        self.bind_slice_ctus = self.slice_ctus if sliced else 0                    # fcu_frame_params.slice_ctus of fcu_chain_begin
        self.sao_slice_ctus = slice_rows * self.w_ctu if slice_rows is not None else self.bind_slice_ctus      # what fcu_sao and fcu_deblock_slices are told
        self.launch_ctus = self.slice_ctus if sliced else self.n_ctu               # `ctus` of compress_chains: every chain to its end
        self.uses_wpp_launch = self.wpp                                            # compress_wpp instead of compress_chains

    def describe(self):
        """the slice mode as the tools echo it"""
        wf = ", WaveFrontSynchro" if self.wpp else ""
        if self.tiles is not None:
            return f"SliceMode 0 (one slice per picture), {self.tiles[0]} x {self.tiles[1]} uniform tiles" + wf
        if self.slice_rows is not None:
            return f"SliceMode 1, SliceArgument {self.slice_rows * self.w_ctu}" + wf
        return ("SliceMode 0 (one slice per picture)" if self.n_slices == 1 else f"SliceMode 1, SliceArgument {self.slice_ctus}") + wf
