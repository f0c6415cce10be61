"""WaveFrontSynchro (WPP) reference for P slices (lowdelay_P), expressed on top of the unchanged oracle (oracle/hmo_py.py).

HM's `TEncSlice::compressSlice` with `WaveFrontSynchro=1` walks the CTUs of a one-slice picture in raster order.  It changes
only the coder state at two points of every row, as for I slices (tests/wpp_oracle.py; TEncSlice.cpp:1386-1411, 1514-1517):
at the first CTU of a row r > 0 `resetEntropy` with the P slice's tables (the B tables when cabac_init_flag chose them), then
`loadContexts` of the state saved after the second CTU of the row above.

The TZ search's start vectors, `TEncSearch::m_integerMv2Nx2N` (TEncSearch.cpp:3833-3842), are a member of the encoder that is
never reset.  The raster walk carries them from CTU to CTU, across rows, and from picture to picture.  One `hmo_py.Encoder`
per picture walks the rows in raster order, so they carry within a picture by themselves; `set_int_mv` before CTU 0 puts back
what the previous picture left.

The helper drives `hmo_py.Encoder(..., slice_ctus=0)` CTU by CTU and writes the coder state between CTUs through the pointer
`hmo_get_cabac` returns (oracle/hmo_search.c:1095-1098).

Not pinned: this restatement rests on reading the HM lines cited above; no HM run with WaveFrontSynchro=1 has recorded its
results for comparison.
"""
import ctypes as C

import numpy as np

import hmo_py
from wpp_oracle import wpp_oracle

NCTX = hmo_py.NCTX
ZERO_MV = [(0, 0)] * 4


class WppPOracle:
    """One P picture, one slice, WPP on.  After run(): `enc` (the hmo_py.Encoder), `row_state[r]` = (ctx[176], frac) after the
    last CTU of row r, `row_int_mv[r]` = m_integerMv2Nx2N after row r, `int_mv` = after the picture."""

    def __init__(self, Y, U, V, qp, int_mv=None, cabac_b_table=0, decision=None, zero_rows=(), **enc_kw):
        """int_mv: the search state the previous picture left (zero when None); enc_kw: hmo_py.Encoder's arguments (ref or
        refs / ref_pocs / poc / col_ref_pocs, col, lambda_override, search_range, fast_search, amp, ...); decision: None or
        (state, obf, sw_skip, sw_term, depth_exception); zero_rows: rows that start from a zeroed search state instead of the
        carried one (a deliberate departure from HM, for tests that show the carry matters)."""
        self.enc = hmo_py.Encoder(Y, U, V, qp, slice_ctus=0, cabac_b_table=cabac_b_table, **enc_kw)
        assert self.enc.p.slice_type == hmo_py.SLICE_P
        h, w = Y.shape
        self.W, self.H = (w + 63) // 64, (h + 63) // 64
        self.int_mv_in = list(int_mv) if int_mv is not None else ZERO_MV
        self.cabac_b_table = cabac_b_table
        self.decision = decision
        self.zero_rows = set(zero_rows)

    def run(self):
        enc = self.enc
        lib = enc.lib
        lib.hmo_cabac_init_tab.restype = None
        lib.hmo_cabac_init_tab.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        slot = lib.hmo_get_cabac(enc.h)                      # POINTER(Cabac) to [0][CI_CURR_BEST]
        W, H = self.W, self.H
        if self.decision is not None:
            enc.set_decision(*self.decision[:4], depth_exception=self.decision[4])
        enc.set_int_mv(self.int_mv_in)
        self.row_state, self.row_int_mv, saved = [], [], []
        for r in range(H):
            if r in self.zero_rows:
                enc.set_int_mv(ZERO_MV)
            for x in range(W):
                a = r * W + x
                if x == 0 and r > 0:
                    lib.hmo_cabac_init_tab(C.cast(slot, C.c_void_p), enc.p.qp, hmo_py.SLICE_P, self.cabac_b_table)     # resetEntropy
                    if W >= 2:
                        C.memmove(C.addressof(slot.contents.ctx), saved[r - 1], NCTX)                              # loadContexts
                enc.compress_ctu(a)
                if x == 1:
                    saved.append(bytes(slot.contents.ctx))
            if W == 1:
                saved.append(None)
            self.row_state.append(enc.cabac(full=True))
            self.row_int_mv.append(enc.test_int_mv())
        self.int_mv = enc.test_int_mv()
        return self


def wpp_p_clip(frames, base_qp, ref_pocs=None, n_refs=1, search_range=64, fast_search=1, tmvp=0, amp=0, cabac_b_table=0,
               sao=False, decision=None, zero_start=(), zero_bottom=False):
    """A lowdelay_P clip as LowDelayPDecider(wpp=True) decides it: POC 0 through the I-slice WPP reference, every later picture
    through WppPOracle with the search state the picture before left, then deblocking (and SAO with `sao`, its slice switches
    following m_saoDisabledRate).  ref_pocs(poc, n_refs): RefPicList0 (lowdelay.ref_pocs) when n_refs > 1; n_refs 1 = the
    previous picture only.  zero_start: POCs that start from a zeroed search state; zero_bottom: the last row of every P
    picture starts from a zeroed one (both departures from HM, for tests).  Returns one dict per picture: poc, o (the
    reference object), ctus (bytes of the Ctu array), rec_unfiltered, rec (after the loop filters), int_mv, ref_pocs, sao."""
    res, dpb, prev, prev_ctus, int_mv = [], {}, None, None, ZERO_MV
    sao_state = hmo_py.SaoState()
    for poc, f in enumerate(frames):
        stype, qp, lam = hmo_py.ldp_slice(poc, base_qp)
        rl = []
        if poc == 0:
            o = wpp_oracle(*f, qp, lambda_override=lam)
        else:
            kw = dict(ref=prev)
            if n_refs > 1:
                rl = ref_pocs(poc, n_refs)
                kw = dict(refs=[dpb[q][0] for q in rl], ref_pocs=rl, poc=poc, col_ref_pocs=dpb[rl[0]][1] or [rl[0] - 1])
            H = (f[0].shape[0] + 63) // 64
            o = WppPOracle(*f, qp, int_mv=ZERO_MV if poc in zero_start else int_mv, cabac_b_table=cabac_b_table, decision=decision,
                           zero_rows=(H - 1,) if (zero_bottom and H > 1) else (), col=prev_ctus if tmvp else None, lambda_override=lam,
                           search_range=search_range, fast_search=fast_search, amp=amp, **kw).run()
            int_mv = o.int_mv
        prev_ctus = o.enc.all_ctus_bytes()
        rec_unf = [p.copy() for p in o.enc.rec]
        o.enc.deblock()
        rec = [p.copy() for p in o.enc.rec]
        params = None
        if sao:
            layer = hmo_py.ldp_layer(poc)
            params, off, _ = hmo_py.sao_picture(f, rec, qp, stype, lam, enabled=sao_state.enabled(layer))
            sao_state.update(layer, off, o.enc.n_ctu)
        res.append(dict(poc=poc, o=o, ctus=prev_ctus, rec_unfiltered=rec_unf, rec=rec, int_mv=int_mv, ref_pocs=rl, sao=params))
        dpb[poc] = (rec, rl)
        prev = rec
    return res
