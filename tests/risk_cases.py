"""Inputs of the risk-table tests, shared by the emulator tests (test_risk.py) and the GPU tests (test_gpu_risk.py): seeded synthetic
CU traces and key arrays for the picture sizes of maps_cases, with the numpy reference (risk_ref.py) computed once per case.  The
builder asserts that every edge the tests rely on is present, so no test passes by leaving one out."""
import functools

import numpy as np

import cu_trace_ref
import labels_ref
import maps_cases
import risk_ref

SIZES = maps_cases.SIZES
MIN_COUNTS = (0, 1, 3)
KEY_TIE, KEY_EMPTY, KEY_TWO = 200, 150, 210                  # depth-3 bins no random key reaches (random depth-3 keys are 0..4)
BIG = 2.0 ** 40 / 256.0


def picture(w, h, seed, index=0):
    """(trace [n_ctu, 85] of CU_TRACE, keys uint16 [NL]) of one synthetic picture.  Every record is random -- also those of blocks
    outside or cut by the picture, which no kernel may count.  Where the picture has at least 12 whole 8x8 blocks, the edges:
    records with valid 0 / split_tried 0 / whole_tried 0 (j0 = FCU_MAX_DOUBLE), j0 == j1, |j0 - j1| below 1/256, a difference
    above 2^40 / 256 and a NaN (both clamped); key 256 at depth 0, keys >= 257, the bin KEY_TIE whose two risks tie, the bin
    KEY_EMPTY no sample has but a block asks for, and the bin KEY_TWO + index with exactly two samples."""
    rng = np.random.default_rng(seed)
    n_ctu = ((w + 63) // 64) * ((h + 63) // 64)
    NL = labels_ref.label_count(w, h)
    tr = np.zeros((n_ctu, 85), cu_trace_ref.CU_TRACE)
    tr["valid"] = rng.random((n_ctu, 85)) < 0.9
    tr["split_tried"] = rng.random((n_ctu, 85)) < 0.85
    tr["whole_tried"] = rng.random((n_ctu, 85)) < 0.9
    tr["split_won"] = (rng.random((n_ctu, 85)) < 0.5) & (tr["split_tried"] != 0)
    tr["j0"] = np.where(tr["whole_tried"] != 0, rng.random((n_ctu, 85)) * 1e5, cu_trace_ref.MAX_DOUBLE)
    tr["j1"] = np.where(tr["split_tried"] != 0, rng.random((n_ctu, 85)) * 1e5, 0.0)
    keys = np.zeros(NL, np.uint16)
    nodes = list(cu_trace_ref.nodes(w, h))
    for a, t, d, x, y, idx, whole in nodes:
        keys[idx] = rng.integers(0, (256 >> (2 * d)) + 1)
        if rng.random() < 0.06:
            keys[idx] = rng.choice([257, 258, 300, 4096, 65535])
    d3 = [n for n in nodes if n[2] == 3 and n[6]]
    if len(d3) < 12:
        return tr, keys
    pick = [d3[i] for i in rng.permutation(len(d3))[:12]]

    def put(n, key=None, **f):
        a, t, d, x, y, idx, whole = n
        rec = dict(valid=1, split_tried=1, whole_tried=1, split_won=0, j0=100.0, j1=50.0)
        rec.update(f)
        for k, v in rec.items():
            tr[k][a, t] = v
        if key is not None:
            keys[idx] = key
    put(pick[0], valid=0)
    put(pick[1], split_tried=0, j1=0.0)
    put(pick[2], whole_tried=0, j0=cu_trace_ref.MAX_DOUBLE, key=KEY_EMPTY)      # no sample: the bin stays empty, the block asks for it
    put(pick[3], j0=1234.5, j1=1234.5, key=1)
    put(pick[4], j0=77.0, j1=77.0 + 1.0 / 1024.0, split_won=1, key=2)
    put(pick[5], j0=3.0 * BIG, j1=1.0, key=3)
    put(pick[6], j0=float("nan"), j1=1.0, split_won=1, key=4)
    put(pick[7], j0=500.25, j1=100.0, split_won=0, key=KEY_TIE)
    put(pick[8], j0=100.0, j1=500.25, split_won=1, key=KEY_TIE)
    put(pick[9], j0=9.0, j1=1.0, split_won=0, key=KEY_TWO + index)
    put(pick[10], j0=2.0, j1=7.5, split_won=1, key=KEY_TWO + index)
    put(pick[11], key=300)                                     # a sample that is dropped
    d0 = [n for n in nodes if n[2] == 0 and n[6]]
    if d0:
        put(d0[0], key=256, j0=10.0, j1=4.0, split_won=1)
    return tr, keys


def assert_edges(w, h, traces, keys, model, dropped):
    """every edge of the issue is in the batch (pictures with at least 12 whole 8x8 blocks)"""
    smp = [s for tr, ky in zip(traces, keys) for s in risk_ref.samples(tr, ky, w, h)]
    elem = {(i, s[4]) for i, (tr, ky) in enumerate(zip(traces, keys)) for s in risk_ref.samples(tr, ky, w, h)}
    whole = [(i, n) for i in range(len(traces)) for n in cu_trace_ref.nodes(w, h) if n[6]]
    rec = lambda i, n: traces[i][n[0], n[1]]
    for field in ("valid", "split_tried", "whole_tried"):
        hit = [(i, n) for i, n in whole if not rec(i, n)[field] and all(rec(i, n)[f] for f in ("valid", "split_tried", "whole_tried") if f != field)]
        assert hit and not any((i, n[5]) in elem for i, n in hit), field
    assert any(not rec(i, n)["whole_tried"] and rec(i, n)["j0"] == cu_trace_ref.MAX_DOUBLE for i, n in whole)
    diffs = [(rec(i, n)["j0"], rec(i, n)["j1"]) for i, n in whole if (i, n[5]) in elem]
    assert any(a == b for a, b in diffs) and any(0 < abs(a - b) < 1 / 256 for a, b in diffs) and any(abs(a - b) > BIG for a, b in diffs) and any(a != a for a, b in diffs)
    assert any(s[3] == 0 for s in smp) and any(s[3] == risk_ref.Q_MAX for s in smp)
    assert any(s[0] == 0 and s[1] == 256 for s in smp) or not any(n[2] == 0 for _, n in whole)
    assert dropped > 0 and any(s[1] >= 257 for s in smp)
    r, c = model["risk"], model["count"]
    assert r[3, KEY_TIE, 0] == r[3, KEY_TIE, 1] > 0 and c[3, KEY_TIE].sum() >= 2
    assert c[3, KEY_EMPTY].sum() == 0 and any(ky[n[5]] == KEY_EMPTY for (i, n), ky in ((p, keys[p[0]]) for p in whole) if n[2] == 3)
    assert any(c[3, KEY_TWO + i].sum() == 2 for i in range(len(traces)))      # exactly min_count - 1 samples for min_count 3; KEY_EMPTY for 1


@functools.lru_cache(maxsize=None)
def case(w, h, n_pics=1, seed=7):
    """(traces, keys, reference model, dropped, {min_count: [labels per picture]}) -- computed once, never modified"""
    pics = [picture(w, h, seed + 11 * i, i) for i in range(n_pics)]
    traces, keys = [p[0] for p in pics], [p[1] for p in pics]
    model, dropped = risk_ref.train(traces, keys, w, h)
    if w * h >= 64 * 64:
        assert_edges(w, h, traces, keys, model, dropped)
    labels = {m: [risk_ref.predict(k, model, m, w, h) for k in keys] for m in MIN_COUNTS}
    for a in traces + keys + [model] + [q for v in labels.values() for q in v]:
        a.setflags(write=False)
    return traces, keys, model, dropped, labels
