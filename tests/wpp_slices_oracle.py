"""WaveFrontSynchro together with SliceMode 1 (slices of whole CTU rows): the reference for the tests, expressed on top of the
unchanged oracle (oracle/hmo_py.py).

HM accepts both switches at once.  With `SliceArgument` a multiple of the picture width in CTUs every slice starts at a row
start, and `TEncSlice::compressSlice` (TEncSlice.cpp:1386-1411, 1514-1517) does, per slice (the slices are independent):

- first CTU of a slice: `resetEntropy` at the start of compressSlice; the CTU is a row start too, so the WaveFrontSynchro branch
  (:1396) resets again; `CUIsFromSameSliceAndTile(pCtuTR)` fails (the above-right CTU belongs to the slice above), so nothing is
  loaded: the row begins from the slice's initial contexts, Q15 counter 0, above neighbours unavailable;
- first CTU of any other row of the slice: as for a one-slice WPP picture (tests/wpp_oracle.py) -- `resetEntropy`, then, when the
  picture is at least two CTUs wide, `loadContexts` of the state saved after CTU 1 of the row above (contexts only); the row
  above is in the same slice, so its above-right CTU is;
- after CTU 1 of every row: the save.

The helper drives `hmo_py.Encoder(..., slice_ctus=R * W, search_state_per_slice=1)` CTU by CTU in raster order.  The oracle itself
resets the coder and masks the neighbourhood at the slice starts and, with that switch, starts the TZ search state
(m_integerMv2Nx2N) of every slice from zero -- this project's convention for slices decided side by side -- and
carries it inside a slice.  The helper adds only: the row-start reset (`hmo_cabac_init_tab` with the slice's tables) and the
context load for rows that do NOT start a slice, the save after CTU 1, and the per-row records (coder state, search state,
Verifying counters added up in row order, the engine's convention for row chains).

Not pinned: this restatement rests on reading the HM lines cited above; no HM run with WaveFrontSynchro=1 and SliceMode 1 has
recorded its results for comparison.  HM's raster walk would also carry the search state across a slice
boundary; the per-slice zero start departs from it only for a slice whose first CTU is too small for a 64x64 CU.
"""
import ctypes as C

import numpy as np

import hmo_py

NCTX = hmo_py.NCTX


class WppSlicesOracle:
    """One I or P picture cut into slices of `slice_rows` whole CTU rows, WPP on.  After run(): `enc` (the hmo_py.Encoder),
    `row_state[r]` = (ctx[176], frac) after the last CTU of row r, `row_int_mv[r]` = the search state after row r,
    `slice_int_mv[s]` = after the last row of slice s, `verify` = the Verifying counters of the rows added up in row order."""

    def __init__(self, Y, U, V, qp, slice_rows, decision=None, cabac_b_table=0, **enc_kw):
        """decision: None or (state, obf, sw_skip, sw_term, depth_exception); enc_kw: hmo_py.Encoder's arguments (ref or refs /
        ref_pocs / poc / col_ref_pocs, col, lambda_override, search_range, fast_search, amp, the tool flags)."""
        assert slice_rows >= 1
        h, w = Y.shape
        self.W, self.H, self.R = (w + 63) // 64, (h + 63) // 64, slice_rows
        self.enc = hmo_py.Encoder(Y, U, V, qp, slice_ctus=slice_rows * self.W, search_state_per_slice=1, cabac_b_table=cabac_b_table, **enc_kw)
        self.cabac_b_table = cabac_b_table
        self.decision = decision

    def run(self, rows=None):
        """rows: decide only the first `rows` CTU rows (whole slices; bounds the cost on a large picture)"""
        enc = self.enc
        lib = enc.lib
        lib.hmo_cabac_init_tab.restype = None
        lib.hmo_cabac_init_tab.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        slot = lib.hmo_get_cabac(enc.h)                      # POINTER(Cabac) to [0][CI_CURR_BEST]
        W, H, R = self.W, self.H, self.R
        self.row_state, self.row_int_mv, self.slice_int_mv, saved = [], [], [], []
        self.verify = np.zeros((4, 6), np.float64)
        assert rows is None or rows % R == 0 or rows >= H
        for r in range(H if rows is None else min(rows, H)):
            if self.decision is not None:                    # counters of this row alone (set_decision clears them)
                enc.set_decision(*self.decision[:4], depth_exception=self.decision[4])
            for x in range(W):
                if x == 0 and r % R != 0:                    # (a row that starts a slice: the slice's reset inside hmo_compress_ctu)
                    lib.hmo_cabac_init_tab(C.cast(slot, C.c_void_p), enc.p.qp, enc.p.slice_type, self.cabac_b_table)     # resetEntropy
                    if W >= 2:
                        C.memmove(C.addressof(slot.contents.ctx), saved[r - 1], NCTX)                                 # loadContexts
                enc.compress_ctu(r * W + x)
                if x == 1:
                    saved.append(bytes(slot.contents.ctx))
            if W == 1:
                saved.append(None)
            self.row_state.append(enc.cabac(full=True))
            self.row_int_mv.append(enc.test_int_mv())
            if r % R == R - 1 or r == H - 1:
                self.slice_int_mv.append(self.row_int_mv[-1])
            if self.decision is not None:
                self.verify += enc.verify_counts()
        return self


def wpp_slices_oracle(Y, U, V, qp, slice_rows, **kw):
    return WppSlicesOracle(Y, U, V, qp, slice_rows, **kw).run()


def wpp_slices_p_clip(frames, base_qp, slice_rows, ref_pocs=None, n_refs=1, search_range=64, fast_search=1, tmvp=0, amp=0, cabac_b_table=0,
                      sao=False, decision=None):
    """A lowdelay_P clip as LowDelayPDecider(wpp=True, slice_rows=R) decides it: every picture (POC 0 an I picture) through
    WppSlicesOracle -- every slice of every picture starts from a zero search state -- then deblocking (LFCrossSliceBoundaryFlag
    1) and, with `sao`, SAO told the slice length, its slice switches following m_saoDisabledRate.  ref_pocs(poc, n_refs):
    RefPicList0 when n_refs > 1; n_refs 1 = the previous picture only.  Returns one dict per picture: poc, o, ctus (bytes of the
    Ctu array), rec_unfiltered, rec (after the loop filters), ref_pocs, sao."""
    res, dpb, prev, prev_ctus = [], {}, None, None
    sao_state = hmo_py.SaoState()
    for poc, f in enumerate(frames):
        stype, qp, lam = hmo_py.ldp_slice(poc, base_qp)
        W = (f[0].shape[1] + 63) // 64
        rl = []
        if poc == 0:
            o = wpp_slices_oracle(*f, qp, slice_rows, lambda_override=lam)
        else:
            kw = dict(ref=prev)
            if n_refs > 1:
                rl = ref_pocs(poc, n_refs)
                kw = dict(refs=[dpb[q][0] for q in rl], ref_pocs=rl, poc=poc, col_ref_pocs=dpb[rl[0]][1] or [rl[0] - 1])
            o = wpp_slices_oracle(*f, qp, slice_rows, cabac_b_table=cabac_b_table, decision=decision, col=prev_ctus if tmvp else None,
                                  lambda_override=lam, search_range=search_range, fast_search=fast_search, amp=amp, **kw)
        prev_ctus = o.enc.all_ctus_bytes()
        rec_unf = [p.copy() for p in o.enc.rec]
        o.enc.deblock()
        rec = [p.copy() for p in o.enc.rec]
        params = None
        if sao:
            layer = hmo_py.ldp_layer(poc)
            params, off, _ = hmo_py.sao_picture(f, rec, qp, stype, lam, enabled=sao_state.enabled(layer), slice_ctus=slice_rows * W)
            sao_state.update(layer, off, o.enc.n_ctu)
        res.append(dict(poc=poc, o=o, ctus=prev_ctus, rec_unfiltered=rec_unf, rec=rec, ref_pocs=rl, sao=params))
        dpb[poc] = (rec, rl)
        prev = rec
    return res
