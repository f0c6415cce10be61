"""WaveFrontSynchro (WPP) reference for the tests -- I and P pictures, one slice or slices of whole CTU rows -- expressed on top
of the unchanged oracle (oracle/hmo_py.py).

One slice.  HM's serial `TEncSlice::compressSlice` with `WaveFrontSynchro=1` walks the CTUs of a one-slice picture in raster
order, as without WPP, and changes only the coder state at two points of every row (TEncSlice.cpp:1386-1411, 1514-1517):

- at the first CTU of a row r > 0: `resetEntropy` of m_pppcRDSbacCoder[0][CI_CURR_BEST] -- the context initialisation of the
  slice (an I slice's tables; a P slice's, or the B tables when cabac_init_flag chose them), and `TEncBinCABAC::start` zeroes
  the fractional bit counter (TEncBinCoderCABAC.cpp:69-79), so the Q15 counter is 0, not carried over -- then, when the
  above-right CTU exists (a picture at least two CTUs wide), `loadContexts` of the state saved for the row above, which copies
  the contexts only (`xCopyContextsFrom`, TEncSbac.cpp:1969), not the counter;
- after the second CTU of every row: that state is saved (`m_entropyCodingSyncContextState.loadContexts(CURR_BEST)`).

Slices of whole rows.  HM accepts WaveFrontSynchro and SliceMode 1 at once.  With `SliceArgument` a multiple of the picture
width in CTUs every slice starts at a row start, and compressSlice does, per slice (the slices are independent):

- first CTU of a slice: `resetEntropy` at the start of compressSlice; the CTU is a row start too, so the WaveFrontSynchro branch
  (:1396) resets again; `CUIsFromSameSliceAndTile(pCtuTR)` fails (the above-right CTU belongs to the slice above), so nothing is
  loaded: the row begins from the slice's initial contexts, Q15 counter 0, above neighbours unavailable;
- first CTU of any other row of the slice: as for a one-slice picture -- `resetEntropy`, then, when the picture is at least two
  CTUs wide, `loadContexts` of the state saved after CTU 1 of the row above (contexts only); the row above is in the same
  slice, so its above-right CTU is;
- after CTU 1 of every row: the save.

The search state.  The TZ search's start vectors, `TEncSearch::m_integerMv2Nx2N` (TEncSearch.cpp:3833-3842), are a member of
the encoder that is never reset.  The raster walk carries them from CTU to CTU, across rows, and from picture to picture.  One
`hmo_py.Encoder` per picture walks the rows in raster order, so they carry within a picture by themselves; for a one-slice
picture `set_int_mv` before CTU 0 puts back what the previous picture left.  With slices the oracle's switch
`search_state_per_slice=1` starts the state of every slice from zero -- this project's convention for slices decided side by
side -- and carries it inside a slice.

The class drives `hmo_py.Encoder(..., slice_ctus=0)`, or `(..., slice_ctus=R * W, search_state_per_slice=1)`, CTU by CTU in
raster order and writes the coder state between CTUs through the pointer `hmo_get_cabac` returns: the oracle's next
`hmo_compress_ctu` starts from that slot (oracle/hmo_search.c:1095-1098).  The oracle itself resets the coder and masks the
neighbourhood at the slice starts; neighbour availability is otherwise the picture's, unchanged by WPP.  The class adds only:
the row-start reset (`hmo_cabac_init_tab` with the slice's tables) and the context load for rows that do NOT start a slice, the
save after CTU 1, and the per-row records (coder state, search state, Verifying counters added up in row order, the engine's
convention for row chains).

QP prediction: `getLastCodedQP`'s wavefront-row rule (TComDataCU.cpp:1484) does not matter here, because MaxDeltaQP is 0 (no
CU QP differs from the slice QP).

Not pinned: this restatement rests on reading the HM lines cited above; no HM run with WaveFrontSynchro=1, with or without
SliceMode 1, has recorded its results for comparison.  HM's raster walk would also carry the search state
across a slice boundary; the per-slice zero start departs from it only for a slice whose first CTU is too small for a 64x64 CU.
"""
import ctypes as C

import numpy as np

import hmo_py

NCTX = hmo_py.NCTX
ZERO_MV = [(0, 0)] * 4


class WppOracle:
    """One I or P picture, WPP on; one slice (slice_rows 0) or slices of `slice_rows` whole CTU rows.  After run(): `enc` (the
    hmo_py.Encoder: ctu_arrays, rec, deblock), `row_start[r]` = (ctx[176], frac) the slot held when CTU 0 of row r started
    (None for a row that starts a slice: the reset is inside hmo_compress_ctu), `saved[r]` = the contexts saved after CTU 1 of
    row r, `row_state[r]` = the coder state after the last CTU of row r (what the engine's row chain r ends with),
    `row_int_mv[r]` = m_integerMv2Nx2N after row r, `slice_int_mv[s]` = after the last row of slice s, `int_mv` = after the
    picture, `verify` = the Verifying counters added up row by row, in row order."""

    def __init__(self, Y, U, V, qp, slice_rows=0, int_mv=None, zero_rows=(), decision=None, cabac_b_table=0, rows=None, **enc_kw):
        """int_mv: the search state the previous picture left (one slice only; zero when None); zero_rows: rows that start from
        a zeroed search state instead of the carried one (a deliberate departure from HM, for tests that show the carry
        matters); decision: None or (state, obf, sw_skip, sw_term, depth_exception) as hmo_py.Encoder.set_decision takes them;
        rows: decide only the first `rows` CTU rows (whole slices; bounds the cost on a large picture); enc_kw: hmo_py.Encoder's
        arguments (ref or refs / ref_pocs / poc / col_ref_pocs, col, lambda_override, search_range, fast_search, amp, the tool
        flags)."""
        assert slice_rows >= 0 and (slice_rows == 0 or int_mv is None)
        h, w = Y.shape
        self.W, self.H, self.R = (w + 63) // 64, (h + 63) // 64, slice_rows
        sliced = dict(slice_ctus=slice_rows * self.W, search_state_per_slice=1) if slice_rows else dict(slice_ctus=0)
        self.enc = hmo_py.Encoder(Y, U, V, qp, cabac_b_table=cabac_b_table, **sliced, **enc_kw)
        self.qp = qp
        self.int_mv_in = int_mv
        self.zero_rows = set(zero_rows)
        self.decision = decision
        self.cabac_b_table = cabac_b_table
        self.rows = self.H if rows is None else min(rows, self.H)
        assert self.rows == self.H or not slice_rows or self.rows % slice_rows == 0

    def run(self):
        enc = self.enc
        lib = enc.lib
        lib.hmo_cabac_init_tab.restype = None
        lib.hmo_cabac_init_tab.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        slot = lib.hmo_get_cabac(enc.h)                      # POINTER(Cabac) to [0][CI_CURR_BEST]
        W, H, R = self.W, self.H, self.R or self.H           # one slice: a slice of all rows
        self.row_start, self.saved, self.row_state, self.row_int_mv, self.slice_int_mv = [], [], [], [], []
        self.verify = np.zeros((4, 6), np.float64)
        if self.int_mv_in is not None:
            enc.set_int_mv(self.int_mv_in)
        for r in range(self.rows):
            if self.decision is not None:                    # counters of this row alone (set_decision installs the state and clears them)
                enc.set_decision(*self.decision[:4], depth_exception=self.decision[4])
            if r in self.zero_rows:
                enc.set_int_mv(ZERO_MV)
            for x in range(W):
                if x == 0 and r % R != 0:                    # (a row that starts a slice: the slice's reset inside hmo_compress_ctu)
                    lib.hmo_cabac_init_tab(C.cast(slot, C.c_void_p), enc.p.qp, enc.p.slice_type, self.cabac_b_table)     # resetEntropy
                    if W >= 2:
                        C.memmove(C.addressof(slot.contents.ctx), self.saved[r - 1], NCTX)                            # loadContexts
                if x == 0:
                    self.row_start.append(None if r % R == 0 else (np.ctypeslib.as_array(slot.contents.ctx).copy(), int(slot.contents.frac)))
                enc.compress_ctu(r * W + x)
                if x == 1:
                    self.saved.append(bytes(slot.contents.ctx))
            if W == 1:
                self.saved.append(None)
            self.row_state.append(enc.cabac(full=True))
            self.row_int_mv.append(enc.test_int_mv())
            if r % R == R - 1 or r == H - 1:
                self.slice_int_mv.append(self.row_int_mv[-1])
            if self.decision is not None:
                self.verify += enc.verify_counts()
        self.int_mv = enc.test_int_mv()
        return self


def wpp_oracle(Y, U, V, qp, slice_rows=0, **kw):
    return WppOracle(Y, U, V, qp, slice_rows, **kw).run()


def wpp_p_clip(frames, base_qp, slice_rows=0, ref_pocs=None, n_refs=1, search_range=64, fast_search=1, tmvp=0, amp=0, cabac_b_table=0,
               sao=False, decision=None, zero_start=(), zero_bottom=False):
    """A lowdelay_P clip as LowDelayPDecider(wpp=True[, slice_rows=R]) decides it: every picture (POC 0 an I picture) through
    WppOracle, then deblocking (LFCrossSliceBoundaryFlag 1) and, with `sao`, SAO (told the slice length when sliced), its slice
    switches following m_saoDisabledRate.  One slice: every P picture starts from the search state the picture before left;
    slices: every slice of every picture starts from a zero search state.  ref_pocs(poc, n_refs): RefPicList0
    (lowdelay.ref_pocs) when n_refs > 1; n_refs 1 = the previous picture only.  zero_start: POCs that start from a zeroed
    search state; zero_bottom: the last row of every P picture starts from a zeroed one (both one slice only, both departures
    from HM, for tests).  Returns one dict per picture: poc, o (the reference object), ctus (bytes of the Ctu array),
    rec_unfiltered, rec (after the loop filters), int_mv, ref_pocs, sao."""
    assert not slice_rows or not (zero_start or zero_bottom)
    res, dpb, prev, prev_ctus, int_mv = [], {}, None, None, ZERO_MV
    sao_state = hmo_py.SaoState()
    for poc, f in enumerate(frames):
        stype, qp, lam = hmo_py.ldp_slice(poc, base_qp)
        H, W = (f[0].shape[0] + 63) // 64, (f[0].shape[1] + 63) // 64
        rl = []
        if poc == 0:
            o = wpp_oracle(*f, qp, slice_rows, lambda_override=lam)
        else:
            kw = dict(ref=prev)
            if n_refs > 1:
                rl = ref_pocs(poc, n_refs)
                kw = dict(refs=[dpb[q][0] for q in rl], ref_pocs=rl, poc=poc, col_ref_pocs=dpb[rl[0]][1] or [rl[0] - 1])
            if not slice_rows:
                kw.update(int_mv=ZERO_MV if poc in zero_start else int_mv, zero_rows=(H - 1,) if (zero_bottom and H > 1) else ())
            o = wpp_oracle(*f, qp, slice_rows, cabac_b_table=cabac_b_table, decision=decision, col=prev_ctus if tmvp else None,
                           lambda_override=lam, search_range=search_range, fast_search=fast_search, amp=amp, **kw)
            int_mv = o.int_mv
        prev_ctus = o.enc.all_ctus_bytes()
        rec_unf = [p.copy() for p in o.enc.rec]
        o.enc.deblock()
        rec = [p.copy() for p in o.enc.rec]
        params = None
        if sao:
            layer = hmo_py.ldp_layer(poc)
            sl = dict(slice_ctus=slice_rows * W) if slice_rows else {}
            params, off, _ = hmo_py.sao_picture(f, rec, qp, stype, lam, enabled=sao_state.enabled(layer), **sl)
            sao_state.update(layer, off, o.enc.n_ctu)
        res.append(dict(poc=poc, o=o, ctus=prev_ctus, rec_unfiltered=rec_unf, rec=rec, int_mv=int_mv, ref_pocs=rl, sao=params))
        dpb[poc] = (rec, rl)
        prev = rec
    return res
