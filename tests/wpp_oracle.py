"""WaveFrontSynchro (WPP) reference for the tests, expressed on top of the unchanged oracle (oracle/hmo_py.py).

HM's serial `TEncSlice::compressSlice` with `WaveFrontSynchro=1` walks the CTUs of a one-slice picture in raster order, as
without WPP, and changes only the coder state at two points of every row (TEncSlice.cpp:1386-1411, 1514-1517):

- at the first CTU of a row r > 0: `resetEntropy` of m_pppcRDSbacCoder[0][CI_CURR_BEST] -- the context initialisation of the
  slice, and `TEncBinCABAC::start` zeroes the fractional bit counter (TEncBinCoderCABAC.cpp:69-79), so the Q15 counter is 0,
  not carried over -- then, when the above-right CTU exists (a picture at least two CTUs wide), `loadContexts` of the state
  saved for the row above, which copies the contexts only (`xCopyContextsFrom`, TEncSbac.cpp:1969), not the counter;
- after the second CTU of every row: that state is saved (`m_entropyCodingSyncContextState.loadContexts(CURR_BEST)`).

The helper drives `hmo_py.Encoder(..., slice_ctus=0)` CTU by CTU in raster order and writes the coder state between CTUs
through the pointer `hmo_get_cabac` returns: the oracle's next `hmo_compress_ctu` starts from that slot
(oracle/hmo_search.c:1095-1098).  Neighbour availability is the one-slice picture's, unchanged by WPP.

QP prediction: `getLastCodedQP`'s wavefront-row rule (TComDataCU.cpp:1484) does not matter here, because MaxDeltaQP is 0 (no
CU QP differs from the slice QP).

Not pinned: this restatement rests on reading the HM lines cited above; no HM run with WaveFrontSynchro=1 has recorded its
results for comparison.
"""
import ctypes as C

import numpy as np

import hmo_py

NCTX = hmo_py.NCTX


def _lib(enc):
    enc.lib.hmo_cabac_init_tab.restype = None
    enc.lib.hmo_cabac_init_tab.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    return enc.lib


class WppOracle:
    """One I picture, one slice, WPP on.  After run(): `enc` (the hmo_py.Encoder: ctu_arrays, rec, deblock),
    `row_start[r]` = (ctx[176], frac) the slot held when CTU 0 of row r > 0 started, `row_state[r]` = the coder state after the
    last CTU of row r (what the engine's row chain r ends with), `saved[r]` = the contexts saved after CTU 1 of row r,
    `verify` = the Verifying counters added up row by row, in row order (the engine's convention for row chains)."""

    def __init__(self, Y, U, V, qp, decision=None, **flags):
        """decision: None, or (state, obf, sw_skip, sw_term, depth_exception) as hmo_py.Encoder.set_decision takes them."""
        self.enc = hmo_py.Encoder(Y, U, V, qp, slice_ctus=0, **flags)
        h, w = Y.shape
        self.W, self.H = (w + 63) // 64, (h + 63) // 64
        self.qp = qp
        self.decision = decision

    def run(self):
        enc = self.enc
        lib = _lib(enc)
        slot = lib.hmo_get_cabac(enc.h)                      # POINTER(Cabac) to [0][CI_CURR_BEST]
        W, H = self.W, self.H
        self.row_start, self.row_state, self.saved = [], [], []
        self.verify = np.zeros((4, 6), np.float64)
        for r in range(H):
            if self.decision is not None:                    # counters of this row alone (set_decision clears them)
                enc.set_decision(*self.decision[:4], depth_exception=self.decision[4])
            for x in range(W):
                a = r * W + x
                if x == 0 and r > 0:
                    lib.hmo_cabac_init_tab(C.cast(slot, C.c_void_p), enc.p.qp, hmo_py.SLICE_I, 0)     # resetEntropy
                    if W >= 2:
                        C.memmove(C.addressof(slot.contents.ctx), self.saved[r - 1], NCTX)           # loadContexts
                if x == 0:                                   # (row 0: the slice start, reset inside hmo_compress_ctu)
                    self.row_start.append(None if r == 0 else (np.ctypeslib.as_array(slot.contents.ctx).copy(), int(slot.contents.frac)))
                enc.compress_ctu(a)
                if x == 1:
                    self.saved.append(bytes(slot.contents.ctx))
            if W == 1:
                self.saved.append(None)
            self.row_state.append(enc.cabac(full=True))
            if self.decision is not None:
                self.verify += enc.verify_counts()
        return self


def wpp_oracle(Y, U, V, qp, decision=None, **flags):
    return WppOracle(Y, U, V, qp, decision=decision, **flags).run()
