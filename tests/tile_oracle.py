"""Reference for tiles (one slice per picture holding C x R uniform tiles, optionally WaveFrontSynchro inside every tile),
expressed on top of the unchanged oracle (oracle/hmo_py.py) and of tests/wpp_oracle.py.

What HM does (TComPicSym::initTiles; TEncSlice.cpp:1386-1411, 1514-1517, 1718-1727; TComDataCU.cpp:422-440, 1071-1390): the CTUs
are coded in tile-scan order; the first CTU of every tile resets the coder; with WaveFrontSynchro the first CTU of a row OF A TILE
resets and, when the tile is at least two CTUs wide, loads the contexts saved after the second CTU of the tile's row above; a CTU
of another tile is unavailable as a neighbour (intra reference samples, MPMs, split / skip contexts, spatial merge and AMVP
candidates); motion vectors, the search window and motion compensation are not restricted to the tile;
end_of_slice_segment_flag is 1 at the last CTU of the picture only.

The restatement.  A tile of a one-slice picture sees exactly what a picture cropped to that tile sees: CTUs of other tiles are
unavailable in the same way samples outside a picture are, partial CTUs exist only where the tile edge is the picture edge, and
the contexts start from the same tables.  So:

- "crop" mode (I pictures; P pictures whose reference planes are plateaus around the tile boundaries, plateau_planes below): the
  unchanged oracle on each tile's cropped planes -- hmo_py.Encoder(slice_ctus=0) for tile chains, WppOracle for WaveFrontSynchro
  inside tiles -- and the per-CTU records and the reconstruction pasted into picture order.  For a P picture the crop's encoder
  gets the same crop of the reference planes; that is what the whole picture's search reads only when the reference picture
  equals its own edge replication wherever a tile's CTUs can read across the tile edge, which reach_of() lets a test assert on
  the reference's own result.
- "sliced" mode (P pictures cut into tile rows only, all of one height): motion search reads the whole reference picture, so a
  crop is wrong at the top and bottom tile edges; the existing sliced reference is right instead --
  hmo_py.Encoder(slice_ctus = tile_h * W, search_state_per_slice=1) / WppOracle(slice_rows = tile_h): a tile row that spans the
  picture width IS a slice of whole rows as far as resets and neighbours go.

The one difference: the crop's (the slice's) last CTU codes end_of_slice_segment_flag = 1 where the tile's last CTU codes a 0,
except in the last tile.  Terminating bins touch no context, so for the last CTU of every tile but the last the comparison leaves
out the Q15 counter of the coder state after it (and the replay bit count); `excluded` lists those CTUs -- at most one per tile.
Everything else is compared on every CTU.

The search state starts from zero in every tile (the project's convention for units decided side by side); one
hmo_py.Encoder per crop does, and search_state_per_slice=1 does.

Not pinned: this restatement rests on reading the HM lines cited above; no HM run with tiles has recorded its results for
comparison."""
import ctypes as C

import numpy as np

import hmo_py
from wpp_oracle import WppOracle

CTU_BYTES = C.sizeof(hmo_py.Ctu)


def grid(W, H, n_cols, n_rows):
    """TComPicSym::initTiles with uniform spacing: (column boundaries, row boundaries) in CTUs"""
    assert 1 <= n_cols <= W and 1 <= n_rows <= H
    return [i * W // n_cols for i in range(n_cols + 1)], [i * H // n_rows for i in range(n_rows + 1)]


def tile_scan(W, H, n_cols, n_rows):
    """picture addresses of the CTUs in tile-scan order"""
    cb, rb = grid(W, H, n_cols, n_rows)
    return [y * W + x for ty in range(n_rows) for tx in range(n_cols) for y in range(rb[ty], rb[ty + 1]) for x in range(cb[tx], cb[tx + 1])]


def plateau_planes(planes, col_bd, row_bd, M):
    """(Y, U, V) with every row made constant over [B - M, B + M) luma samples around each inner tile column boundary B (CTUs in
    col_bd), then every column over the same span around each inner row boundary: there the picture equals the edge
    replication of either tile's crop"""
    out = [np.ascontiguousarray(p).copy() for p in planes]
    for k, p in enumerate(out):
        sh = 1 if k else 0
        m = M >> sh
        for b in col_bd[1:-1]:
            B = (b * 64) >> sh
            p[:, B - m:B + m] = p[:, B - m:B - m + 1]
        for b in row_bd[1:-1]:
            B = (b * 64) >> sh
            p[B - m:B + m, :] = p[B - m:B - m + 1, :]
    return out


def reach_of(ctus_bytes, search_range):
    """max |mv| / 4 + SearchRange + 5 over the inter partitions of a decided picture (luma samples, rounded up): how far beyond
    its own block a CU's search and interpolation can have read"""
    a = np.frombuffer(ctus_bytes, np.dtype(hmo_py.Ctu))
    inter = a["pred_mode"] == 0
    mv = np.abs(a["mv"].astype(np.int64))[inter]
    return (int(mv.max()) + 3) // 4 + search_range + 5 if mv.size else search_range + 5, int(inter.sum())


def moved_planes(planes, dx, dy):
    """(Y, U, V) whose sample (y, x) is the input's (y + dy, x + dx), the input's border replicated (dx, dy even: chroma moves by
    half): content that moves by (-dx, -dy) luma samples, i.e. a motion vector of (4 dx, 4 dy) quarter samples"""
    out = []
    for k, p in enumerate(planes):
        sx, sy = (dx >> 1, dy >> 1) if k else (dx, dy)
        m = max(abs(sx), abs(sy))
        q = np.pad(p, m, mode="edge")
        out.append(np.ascontiguousarray(q[m + sy:m + sy + p.shape[0], m + sx:m + sx + p.shape[1]]))
    return out


def _zidx(x4, y4):
    return sum((((x4 >> i) & 1) << (2 * i)) | (((y4 >> i) & 1) << (2 * i + 1)) for i in range(4))


def left_edge_evidence(ref, untiled_bytes):
    """What makes the horizontal masking of the motion neighbours visible on a tiled P picture.  Over the 4x4 partitions in the
    first column of every tile that has a tile to its left: (how many are inter AND have an inter left neighbour -- which lies
    in the other tile --, how many of those differ from their twin of the untiled picture in merge_flag / merge_idx / mvp_idx /
    mv / mvd)."""
    dt = np.dtype(hmo_py.Ctu)
    t, u = np.frombuffer(ref.ctus, dt), np.frombuffer(untiled_bytes, dt)
    n_nb = n_diff = 0
    for b in ref.cb[1:-1]:
        for cy in range(ref.H):
            a = cy * ref.W + b
            for j in range(min(16, (ref.h - cy * 64) // 4)):
                p, q = _zidx(0, j), _zidx(15, j)
                if t["pred_mode"][a][p] != 0 or t["pred_mode"][a - 1][q] != 0:
                    continue
                n_nb += 1
                n_diff += any(not np.array_equal(t[k][a][p], u[k][a][p]) for k in ("merge_flag", "merge_idx", "mvp_idx", "mv", "mvd"))
    return n_nb, n_diff


class TileRef:
    """After run(): `ctus` (bytes of the picture's Ctu array, picture order), `rec` (planes before deblocking), `chains` (chain
    order: dicts ctx, frac -- None where the chain ends with a CTU of `excluded` --, mv, n_ctu = CTUs of the chain), `excluded`
    (picture addresses of the last CTU of every tile but the last), `verify` (Verifying counters added up in chain order)."""

    def __init__(self, frame, qp, tiles, wpp=False, mode="crop", decision=None, cabac_b_table=0, ref=None, **enc_kw):
        """decision: None or (state, obf of the PICTURE, sw_skip, sw_term, depth_exception); ref: the reference planes of a P
        picture (whole picture); enc_kw: hmo_py.Encoder's arguments (lambda_override, search_range, fast_search, amp, the tool
        flags)"""
        self.f = [np.ascontiguousarray(a) for a in frame]
        self.h, self.w = self.f[0].shape
        self.W, self.H = (self.w + 63) // 64, (self.h + 63) // 64
        self.qp, self.tiles, self.wpp, self.mode, self.decision, self.btab, self.ref, self.kw = qp, tiles, wpp, mode, decision, cabac_b_table, ref, enc_kw
        self.cb, self.rb = grid(self.W, self.H, *tiles)
        assert mode in ("crop", "sliced")

    def _crop(self, planes, x0, y0, x1, y1):
        return [np.ascontiguousarray(p[(y0 * 64) >> s:(min(y1 * 64, self.h)) >> s, (x0 * 64) >> s:(min(x1 * 64, self.w)) >> s])
                for p, s in zip(planes, (0, 1, 1))]

    def run(self):
        W = self.W
        self.ctus = bytearray(CTU_BYTES * W * self.H)
        self.rec = [np.zeros_like(a) for a in self.f]
        self.chains, self.excluded = [], []
        self.verify = np.zeros((4, 6), np.float64)
        (self._run_sliced if self.mode == "sliced" else self._run_crops)()
        n_tiles = self.tiles[0] * self.tiles[1]
        assert len(self.excluded) == n_tiles - 1                 # at most one CTU per tile, none in the last
        self.ctus = bytes(self.ctus)
        return self

    def _chain(self, state, mv, n_ctu, ends_other_tile):
        self.chains.append(dict(ctx=state[0], frac=None if ends_other_tile else state[1], mv=mv, n_ctu=n_ctu))

    def _run_crops(self):
        C_, R_ = self.tiles
        for ty in range(R_):
            for tx in range(C_):
                x0, x1, y0, y1 = self.cb[tx], self.cb[tx + 1], self.rb[ty], self.rb[ty + 1]
                tw, th = x1 - x0, y1 - y0
                last_tile = ty == R_ - 1 and tx == C_ - 1
                org = self._crop(self.f, x0, y0, x1, y1)
                kw = dict(self.kw)
                if self.ref is not None:
                    kw["ref"] = self._crop(self.ref, x0, y0, x1, y1)
                dec = None
                if self.decision is not None:
                    st_, obf, sk, te, de = self.decision
                    dec = (st_, np.ascontiguousarray(obf[y0 * 16:y1 * 16, x0 * 16:x1 * 16]), sk, te, de)
                if self.wpp:
                    o = WppOracle(*org, self.qp, decision=dec, cabac_b_table=self.btab, **kw).run()
                    enc = o.enc
                    for r in range(th):
                        self._chain(o.row_state[r], o.row_int_mv[r], tw, r == th - 1 and not last_tile)
                    self.verify += o.verify
                else:
                    enc = hmo_py.Encoder(*org, self.qp, slice_ctus=0, cabac_b_table=self.btab, **kw)
                    if dec is not None:
                        enc.set_decision(*dec[:4], depth_exception=dec[4])
                    enc.compress_frame()
                    self._chain(enc.cabac(full=True), enc.test_int_mv(), tw * th, not last_tile)
                    if dec is not None:
                        self.verify += enc.verify_counts()
                assert enc.n_ctu == tw * th
                raw = enc.all_ctus_bytes()
                for k in range(tw * th):
                    a = (y0 + k // tw) * self.W + x0 + k % tw
                    self.ctus[a * CTU_BYTES:(a + 1) * CTU_BYTES] = raw[k * CTU_BYTES:(k + 1) * CTU_BYTES]
                for p, q, s in zip(self.rec, enc.rec, (0, 1, 1)):
                    p[(y0 * 64) >> s:((y0 * 64) >> s) + q.shape[0], (x0 * 64) >> s:((x0 * 64) >> s) + q.shape[1]] = q
                if not last_tile:
                    self.excluded.append((y1 - 1) * self.W + x1 - 1)

    def _run_sliced(self):
        C_, R_ = self.tiles
        assert C_ == 1 and self.decision is None and self.H % R_ == 0     # tile rows of one height: slices of th whole rows
        th, W = self.H // R_, self.W
        kw = dict(self.kw)
        if self.ref is not None:
            kw["ref"] = self.ref
        if self.wpp:
            o = WppOracle(*self.f, self.qp, slice_rows=th, cabac_b_table=self.btab, **kw).run()
            enc = o.enc
            for r in range(self.H):
                self._chain(o.row_state[r], o.row_int_mv[r], W, r % th == th - 1 and r != self.H - 1)
        else:
            enc = hmo_py.Encoder(*self.f, self.qp, slice_ctus=th * W, search_state_per_slice=1, cabac_b_table=self.btab, **kw)
            for a in range(enc.n_ctu):
                enc.compress_ctu(a)
                if (a + 1) % (th * W) == 0:
                    self._chain(enc.cabac(full=True), enc.test_int_mv(), th * W, a + 1 != enc.n_ctu)
        self.ctus[:] = enc.all_ctus_bytes()
        for p, q in zip(self.rec, enc.rec):
            p[...] = q
        self.excluded = [(t + 1) * th * W - 1 for t in range(R_ - 1)]

    def deblocked(self):
        """the assembled picture after TComLoopFilter::loopFilterPic, LFCrossTileBoundaryFlag 1"""
        rec = [p.copy() for p in self.rec]
        hmo_py.deblock_pic(self.ctus, self.w, self.h, rec)
        return rec


def tile_reference(frame, qp, tiles, **kw):
    return TileRef(frame, qp, tiles, **kw).run()


def assert_picture_equal(ref, out_bytes, rec, states, mvs=None, sorted_ctx=None, tag=()):
    """A decided picture against the reference: every fcu_ctu_out field of every CTU (out_bytes: the Ctu array as bytes), the
    reconstruction before deblocking, the coder state after every chain (states[i] = (ctx[176], frac); the Q15 counter left out
    exactly where the chain ends with a CTU of ref.excluded), and the search state after every chain when mvs is given.
    sorted_ctx: an index selecting the contexts to compare (P pictures: search_trace.O_SORTED).  Returns the number of coder
    states whose Q15 counter was left out."""
    dt = np.dtype(hmo_py.Ctu)
    got, want = np.frombuffer(bytes(out_bytes), dt), np.frombuffer(ref.ctus, dt)
    assert len(got) == len(want) == ref.W * ref.H
    for name in dt.names:
        bad = [a for a in range(len(want)) if not np.array_equal(got[name][a], want[name][a])]
        assert not bad, tag + (name, "differs at CTU", bad[:8])
    for p, q in zip(rec, ref.rec):
        assert np.array_equal(np.asarray(p), q), tag + ("reconstruction",)
    assert len(states) == len(ref.chains)
    sel = slice(None) if sorted_ctx is None else sorted_ctx
    skipped = 0
    for i, (c, (ctx, frac)) in enumerate(zip(ref.chains, states)):
        assert np.array_equal(np.asarray(ctx)[sel], c["ctx"][sel]), tag + (i, "contexts after the chain")
        if c["frac"] is None:
            skipped += 1
        else:
            assert frac == c["frac"], tag + (i, "Q15 counter after the chain")
        if mvs is not None:
            assert mvs[i] == c["mv"], tag + (i, "search state after the chain")
    assert skipped <= len(ref.excluded)
    return skipped
