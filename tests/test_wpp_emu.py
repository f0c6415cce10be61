"""The engine source's WaveFrontSynchro row chains on the CPU wave emulator (tests/emu/wpp_emu.cpp) against the WPP
reference (tests/wpp_oracle.py): every fcu_ctu_out field, the reconstruction and each row's final coder state."""
import numpy as np
import pytest

import hmo_py
from wpp_oracle import wpp_oracle
from wpp_testlib import TOOLS, assert_ctus_equal, emulate, flags_of, wpp_emu  # noqa: F401 (wpp_emu: the fixture)

CASES = [
    ("mixed", 256, 192, 22, -1, None),
    ("textured", 64, 192, 37, -1, None),    # W = 1: every row starts from the plain reset
    ("smooth", 200, 136, 37, -1, None),     # partial CTUs on both edges
    ("mixed", 136, 72, 22, -1, None),
    ("textured", 200, 136, 22, TOOLS, None),
    ("mixed", 256, 192, 32, -1, "testing"),
    ("mixed", 200, 136, 37, -1, "verifying"),
]


@pytest.mark.parametrize("gen,w,h,qp,tools,state", CASES)
def test_emulated_wpp_rows_are_bit_exact(wpp_emu, pkg, gen, w, h, qp, tools, state):
    Y, U, V = getattr(pkg.synth, gen)(w, h, seed=9)
    decision = None
    if state is not None:
        obf, _ = hmo_py.obf_prepass(Y)
        st = hmo_py.TESTING if state == "testing" else hmo_py.VERIFYING
        decision = (st, obf, (1, 1, 0, 1), (1, 0, 1, 1), 0)
    o = wpp_oracle(Y, U, V, qp, decision=decision, **flags_of(tools))
    e = emulate(wpp_emu, (Y, U, V), qp, tools=tools, decision=decision)       # (checks the row count, runs every row to its end)
    assert len(e["states"]) == o.H
    assert_ctus_equal(o.enc, e["out"])
    for p, q in zip(o.enc.rec, e["rec"]):
        assert np.array_equal(p, q)
    for r in range(o.H):
        assert np.array_equal(e["states"][r][0], o.row_state[r][0]) and e["states"][r][1] == o.row_state[r][1], r
    if state == "verifying":
        assert np.array_equal(e["verify"], o.verify)
        assert e["verify"][:, :4].sum() > 0
