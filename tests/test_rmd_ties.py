"""RMD candidate list under ties.  The reference keeps CandCostList with a sorted insert and a strict '<' (xUpdateCandList,
TEncSearch.cpp:5345-5370): among equal costs the lower mode number comes first.  The engine ranks the 35 modes in parallel, so
the order of equal costs is a property it has to state rather than inherit.  These pictures make most costs equal: on a flat
picture every mode predicts the source exactly (SATD 0 for all 35), and on a picture of flat 16x16 tiles the same holds for
every PU that lies inside a tile whose neighbours are not reconstructed differently -- only the mode bits (MPM or not)
separate the costs, and all non-MPM modes tie.  Engine source on the CPU emulator == oracle, for every PU of every CTU."""
import numpy as np
import pytest

import emu_py
import hmo_py


def _flat(w, h, seed):
    return (np.full((h, w), 128, np.uint8), np.full((h // 2, w // 2), 128, np.uint8), np.full((h // 2, w // 2), 128, np.uint8))


def _tiles(w, h, seed):
    rng = np.random.default_rng(seed)
    lv = lambda hh, ww, t: np.kron(rng.integers(16, 240, size=((hh + t - 1) // t, (ww + t - 1) // t)), np.ones((t, t), dtype=np.int64))[:hh, :ww].astype(np.uint8)
    return (np.ascontiguousarray(lv(h, w, 16)), np.ascontiguousarray(lv(h // 2, w // 2, 8)), np.ascontiguousarray(lv(h // 2, w // 2, 8)))


@pytest.mark.parametrize("gen,w,h,qp", [(_flat, 128, 64, 32), (_tiles, 128, 128, 32), (_tiles, 136, 72, 22)])
def test_rmd_list_order_under_ties_equals_oracle(built, gen, w, h, qp):
    f = gen(w, h, 11)
    o, e = hmo_py.Encoder(*f, qp), emu_py.EmuEncoder(*f, qp)
    to, te = o.enable_pu_trace(), e.enable_pu_trace()
    o.compress_frame()
    e.compress_frame()
    assert to.shape == te.shape and np.array_equal(to["valid"], te["valid"])
    n_pu = n_tied = 0
    for a in range(to.shape[0]):
        for p in range(to.shape[1]):
            ro, re = to[a][p], te[a][p]
            if not ro["valid"]:
                continue
            n_pu += 1
            assert ro["n_rd"] == re["n_rd"] and ro["n_rmd"] == re["n_rmd"], (a, p)
            assert np.array_equal(ro["rd_mode"][:ro["n_rd"]], re["rd_mode"][:re["n_rd"]]), (a, p, ro["rd_mode"], re["rd_mode"])
            assert ro["rmd_cost"][:ro["n_rmd"]].tobytes() == re["rmd_cost"][:re["n_rmd"]].tobytes(), (a, p)
            assert ro["best_mode"] == re["best_mode"], (a, p)
            c = ro["rmd_cost"][:ro["n_rmd"]]
            n_tied += int((np.diff(c) == 0).any())
    assert n_pu == int(to["valid"].sum()) and n_pu >= hmo_py.PUS_PER_CTU
    # the fixture does what it is for: in most PUs at least two survivors have the same cost
    assert n_tied * 2 > n_pu, (n_tied, n_pu)
    assert to.tobytes() == te.tobytes()
