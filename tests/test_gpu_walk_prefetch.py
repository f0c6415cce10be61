"""The frames of tests/test_walk_prefetch_emu.py on the device against the oracle: one chain per frame, all chains of a size
in one launch, every TComDataCU array and the reconstruction bit-exact."""
import numpy as np
import pytest

import hmo_py
from test_gpu_parity import _compare_ctu
from walk_prefetch_cases import QPS, SIZES, SOURCES, frame

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("w,h", SIZES)
def test_walk_edge_case_frames_match_oracle(pkg, w, h):
    cases = [(s, qp) for s in SOURCES for qp in QPS]
    frames = [frame(pkg, s, w, h) for s, _ in cases]
    eng = pkg.CuEngine(w, h, max_chains=len(cases))
    for i, (f, (_, qp)) in enumerate(zip(frames, cases)):
        eng.init_chain(i, f, qp=qp)
    eng.compress_chains(0, len(cases), eng.n_ctu)
    eng.sync()
    for i, (f, (s, qp)) in enumerate(zip(frames, cases)):
        ref = hmo_py.Encoder(*f, qp)
        ref.compress_frame()
        for a in range(eng.n_ctu):
            _compare_ctu(eng.ctu_out(i, a), ref.ctu_arrays(a), f"{s} {w}x{h} qp{qp} ctu{a}")
        for p, q in zip(eng.rec_planes(i), ref.rec):
            assert np.array_equal(p, q), f"{s} {w}x{h} qp{qp}: reconstruction"
    eng.destroy()
