"""Reference of the risk-table model (fcu_risk_train, fcu_risk_predict, fcu_risk_table) in plain numpy with Python integers, written
from the definitions in include/fcu.h over host copies of CU traces and key arrays.  It shares nothing with the kernel source: the
samples come from a walk over every block of every CTU (cu_trace_ref.nodes), the sums are Python integers in dictionaries."""
import math

import numpy as np

import cu_trace_ref
import maps_ref

BINS = 257
Q_MAX = (1 << 40) - 1
SPLIT, NOT_SPLIT, ABSENT, FORCED = 1, 0, -1, 2
MODEL = np.dtype([("risk", np.int64, (4, BINS, 2)), ("count", np.uint32, (4, BINS, 2))])      # fcu_risk_model
assert MODEL.itemsize == 24672


def q_of(j0, j1):
    """floor(|j0 - j1| * 256) clamped to 2^40 - 1; whatever is not < 2^40 (NaN, infinity) gives 2^40 - 1"""
    s = abs(float(j0) - float(j1)) * 256.0
    if not s < float(1 << 40):
        return Q_MAX
    return min(int(math.floor(s)), Q_MAX)


def samples(trace, keys, w, h):
    """[(depth, key, split_won, q, label element)] of one picture: the records with valid, split_tried and whole_tried of the
    blocks that lie wholly inside the picture, key = keys[element]; keys >= BINS included (the caller drops them)"""
    trace = np.asarray(trace).reshape(-1, cu_trace_ref.CUS_PER_CTU)
    out = []
    for a, t, d, x, y, idx, whole in cu_trace_ref.nodes(w, h):
        r = trace[a, t]
        if whole and r["valid"] and r["split_tried"] and r["whole_tried"]:
            out.append((d, int(keys[idx]), 1 if r["split_won"] else 0, q_of(r["j0"], r["j1"]), idx))
    return out


def train(traces, keys, w, h, model=None):
    """(model, dropped) of a batch: model = a copy of `model` (or zeros) with the batch added"""
    risk, count, dropped = {}, {}, 0
    for tr, ky in zip(traces, keys):
        for d, x, truth, q, _ in samples(tr, ky, w, h):
            if x >= BINS:
                dropped += 1
                continue
            risk[d, x, truth] = risk.get((d, x, truth), 0) + q
            count[d, x, truth] = count.get((d, x, truth), 0) + 1
    out = np.zeros((), MODEL) if model is None else np.array(model, MODEL).reshape(()).copy()
    for k, v in risk.items():
        tot = int(out["risk"][k]) + v
        assert tot < 1 << 63
        out["risk"][k] = tot
    for k, v in count.items():
        out["count"][k] = int(out["count"][k]) + v
    return out, dropped


def table(model, min_count):
    """int8 [4, BINS]: NOT_SPLIT iff risk[..][1] < risk[..][0], else SPLIT; ABSENT below min_count samples"""
    out = np.zeros((4, BINS), np.int8)
    model = np.asarray(model).reshape(())
    for d in range(4):
        for x in range(BINS):
            r0, r1 = int(model["risk"][d, x, 0]), int(model["risk"][d, x, 1])
            n = int(model["count"][d, x, 0]) + int(model["count"][d, x, 1])
            out[d, x] = ABSENT if n < min_count else (NOT_SPLIT if r1 < r0 else SPLIT)
    return out


def predict(keys, model, min_count, w, h):
    """int8 [NL]: FORCED on a block of depth < 3 the picture edge cuts, ABSENT for a key >= BINS, else the table's label"""
    tab = table(model, min_count)
    out, o = [], 0
    for d, (bh, bw) in enumerate(maps_ref.level_shapes(w, h)):
        s = 64 >> d
        for by in range(bh):
            for bx in range(bw):
                x = int(keys[o])
                whole = bx * s + s <= w and by * s + s <= h
                out.append(FORCED if d < 3 and not whole else (ABSENT if x >= BINS else int(tab[d, x])))
                o += 1
    assert o == len(keys)
    return np.array(out, np.int8)


def loss(trace, labels, w, h):
    """(FPLoss + FNLoss of a label array against a trace in doubles, scored samples): cu_trace_ref.score over all depths"""
    _, pic = cu_trace_ref.score(trace, labels, w, h)
    return float(pic["v"][:, 4:].sum()), int(pic["scored"].sum()) + int(pic["open"].sum())
