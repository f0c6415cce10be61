"""Inputs of the many-CTU tests (test_big_pictures.py on the emulators, test_gpu_big_pictures.py through the C ABI): pictures past
the sizes at which the picture-level kernels take a second trip of their record walk (report_pic, match_pic, score_pic) or run into the cap on their grid (risk_train / risk_add),
as small in pixels as those thresholds allow -- one CTU row, 8 samples high.  Seeded synthetic records, traces, labels and keys
(nothing is decided), the numpy references computed once per case and set read-only.

Every builder asserts, from the constants tests/emu/big_emu.cpp exports (the kernels' own enums), that the path it is named
after is really crossed: a retuned constant makes the case fail, it does not quietly stop covering the path.

What the strip cannot give: a block of depth 0..2 is never wholly inside a picture 8 samples high, so the samples of
fcu_label_score and fcu_risk_train are all of depth 3 here (the sums of the other depths are zero on both sides), and the tail
CTU (8 samples wide) holds one whole 8x8 block and four 4x4 partitions."""
import ctypes as C
import functools
import os

import numpy as np

import cu_trace_ref
import labels_ref
import maps_cases
import maps_ref
import report_cases
import report_ref
import risk_cases
import risk_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEIGHT = 8
# CTUs -> width.  128: whole CTUs, the last size with one trip of the 128-record walks; 129: the tail CTU 16 wide, so that the width
# stays a multiple of 16 (the report's wide loads); 130: the tail CTU 8 wide, the width no multiple of 16
WIDTHS = {128: 64 * 128, 129: 64 * 128 + 16, 130: 64 * 129 + 8}
MANY = 130
RISK_PICS, RISK_SPLIT = 16, 3                                # 16 x 130 = 2080 units; accumulate as 3 + 13 pictures
KEY_LATE = 240                                               # a depth-3 bin nothing else reaches: the sample of a wave's third unit


def _pkg():
    import __graft_entry__ as g
    return g.load_package()


@functools.lru_cache(maxsize=None)
def _emu():
    return C.CDLL(os.path.join(ROOT, "tests", "emu", "libbig_emu.so"))


def size(n_ctu):
    w = WIDTHS[n_ctu]
    assert (w + 63) // 64 == n_ctu and w % 8 == 0
    return w, HEIGHT


def thresholds():
    """the constants of the kernels, as tests/emu/big_emu.cpp exports them from the kernel source"""
    L = _emu()
    return {"report_trip": L.big_emu_report_pic_trip(), "match_trip": L.big_emu_match_pic_trip(), "score_ahead": L.big_emu_score_ahead(),
            "score_ctus": L.big_emu_score_ctus(), "risk_slots": L.big_emu_risk_max_slots(), "risk_group_units": L.big_emu_risk_group_units(),
            "risk_waves": L.big_emu_risk_waves(), "risk_pred_threads": L.big_emu_risk_pred_threads()}


def assert_trips(trip, what):
    """the three sizes against a walk of `trip` records per trip: 128 CTUs = one full trip and no more, 129 and 130 a second trip
    that is partial (the r < n_ctu guard with the tail in a later trip)"""
    assert sorted(WIDTHS) == [trip, trip + 1, trip + 2], (what, trip)
    for n in WIDTHS:
        trips, tail = (n + trip - 1) // trip, n % trip
        assert (trips == 1 and tail == 0) if n == trip else (trips >= 2 and 0 < tail < trip), (what, n, trip)


# ---- the picture report
def report_records(w, h, seed):
    """report_cases.records, then the first four partitions of every CTU (z = 0..3: the top-left 8x8 block, inside every CTU of
    the strip) set so that all sixteen dwords of the CTU's report record are non-zero -- report_pic sums dword by dword, so a
    record that is dropped, doubled or read from another place moves every sum"""
    e = _pkg().engine
    rng = np.random.default_rng(seed + 77)
    r = report_cases.records(w, h, seed)
    n = r.shape[0]
    off = {k: getattr(e.CtuOut, k).offset for k in ("depth", "part_size", "pred_mode", "skip", "merge_flag", "cbf")}
    z = np.arange(4)
    r[:, off["depth"] + z] = np.stack([rng.integers(1, 3, n), np.full(n, 3), rng.integers(0, 4, n), rng.integers(0, 4, n)], 1)      # (depth 1 | 2), depth 3
    r[:, off["part_size"] + z] = np.stack([rng.integers(1, 3, n), rng.integers(3, 5, n), rng.integers(5, 7, n), np.full(n, 7)], 1)   # (1 | 2), (3 | 4), (5 | 6), 7
    r[:, off["pred_mode"] + z] = rng.integers(0, 2, (n, 4))
    for k, key in enumerate(("skip", "merge_flag")):
        r[:, off[key] + z] = rng.integers(0, 2, (n, 4))
        r[np.arange(n), off[key] + rng.integers(0, 4, n)] = 1 + 2 * k
    for k in range(3):
        r[:, off["cbf"] + 256 * k + z] = rng.integers(0, 8, (n, 4))
        r[np.arange(n), off["cbf"] + 256 * k + rng.integers(0, 4, n)] = 1 + 2 * k
    return r


@functools.lru_cache(maxsize=None)
def report_case(n_ctu, seed):
    """(org, rec, records, reference picture report, reference CTU records) as report_cases.case gives them"""
    assert_trips(thresholds()["report_trip"], "report_pic")
    w, h = size(n_ctu)
    org, rec = report_cases.planes(w, h, seed)
    r = report_records(w, h, seed + 1000)
    pic, ctu = report_ref.picture_report(_pkg(), org, rec, r)
    assert len(ctu) == n_ctu and (ctu.view(np.uint32).reshape(n_ctu, 16) != 0).all()
    assert int(pic["bits"]) > (1 << 32) and all(int(v) > 0 for v in pic["part_size_part"])
    for a in org + rec + [r, ctu]:
        a.setflags(write=False)
    return org, rec, r, pic, ctu


# ---- the split match
def match_records(w, h, seed, base=None, redraw=None):
    """fcu_ctu_out records whose depth and part_size entries are random over the values the labels tell apart (no valid quadtree is
    needed: the match reads one entry per node).  base / redraw: a copy of `base` with the CTUs of `redraw` drawn again"""
    e = _pkg().engine
    rng = np.random.default_rng(seed)
    n_ctu = ((w + 63) // 64) * ((h + 63) // 64)
    r = np.zeros((n_ctu, e.CTU_OUT_BYTES), np.uint8) if base is None else base.copy()
    rows = np.arange(n_ctu) if redraw is None else np.asarray(redraw)
    d, p = e.CtuOut.depth.offset, e.CtuOut.part_size.offset
    r[rows, d:d + 256] = rng.integers(0, 4, (len(rows), 256))
    r[rows, p:p + 256] = rng.choice([0, 1, 2, 3, 3, 3], (len(rows), 256))
    return r


@functools.lru_cache(maxsize=None)
def match_case(n_ctu, seed):
    """(records A, records B, reference of A against B, the CTUs in which B differs): B = A with a seeded third of the CTUs drawn
    again, the first record, the last one and the first record of the second trip among them"""
    trip = thresholds()["match_trip"]
    assert_trips(trip, "match_pic")
    w, h = size(n_ctu)
    a = match_records(w, h, seed)
    rng = np.random.default_rng(seed + 1)
    third = set(int(i) for i in rng.choice(n_ctu, n_ctu // 3, replace=False)) | {0, n_ctu - 1} | ({trip} if n_ctu > trip else {trip - 1})
    third = sorted(third)
    b = match_records(w, h, seed + 2, base=a, redraw=third)
    assert [i for i in range(n_ctu) if not np.array_equal(a[i], b[i])] == third
    want = maps_ref.split_match(_pkg(), a, b, w, h)
    assert 0 < want["part_equal"] < want["part_total"] == (w // 4) * (h // 4) and want["node"][3].all() and want["only_a"][3] and want["only_b"][3]
    for q in (a, b):
        q.setflags(write=False)
    return a, b, want, third


# ---- the label score and the trace maps
def score_picture(w, h, seed):
    """(trace [n_ctu, 85], labels int8 [NL]).  Every record and every label is random -- also those of blocks outside or cut by the
    picture, which no kernel may count; the costs are finite, so that no sum ends as an infinity.  Then the whole 8x8 blocks of a
    CTU are dealt, in turn, to TP, FP, TN, FN and `open`, so that every CTU but the tail one (one whole block) has a non-zero
    entry in every field score_pic sums at depth 3 -- both loss sums among them"""
    rng = np.random.default_rng(seed + 5)
    n_ctu = ((w + 63) // 64) * ((h + 63) // 64)
    NL = labels_ref.label_count(w, h)
    tr = np.zeros((n_ctu, 85), cu_trace_ref.CU_TRACE)
    tr["valid"] = rng.random((n_ctu, 85)) < 0.9
    tr["split_tried"] = rng.random((n_ctu, 85)) < 0.85
    tr["whole_tried"] = rng.random((n_ctu, 85)) < 0.9
    tr["split_won"] = (rng.random((n_ctu, 85)) < 0.5) & (tr["split_tried"] != 0)
    tr["j0"], tr["j1"] = rng.random((n_ctu, 85)) * 1e5, rng.random((n_ctu, 85)) * 1e5
    lab = rng.choice(np.array([labels_ref.SPLIT, labels_ref.NOT_SPLIT, labels_ref.ABSENT, labels_ref.FORCED, 7], np.int8), NL, p=[0.4, 0.4, 0.08, 0.08, 0.04])
    turn = {}
    for a, t, d, x, y, idx, whole in cu_trace_ref.nodes(w, h):
        if d != 3 or not whole:
            continue
        k = turn.get(a, 0)
        turn[a] = k + 1
        if k >= 5:
            continue                                           # (the others stay random)
        won, v = ((1, labels_ref.SPLIT), (0, labels_ref.SPLIT), (0, labels_ref.NOT_SPLIT), (1, labels_ref.NOT_SPLIT), (int(rng.integers(0, 2)), labels_ref.ABSENT))[k]
        tr["valid"][a, t], tr["split_tried"][a, t], tr["split_won"][a, t] = 1, 1, won
        tr["j0"][a, t], tr["j1"][a, t] = rng.random(2) * 1e5
        lab[idx] = v
    return tr, lab


def reversed_sums(ctu):
    """the picture's loss sums with the CTU records added in reversed raster order (one after the other from 0.0)"""
    out = np.zeros((4, 2), np.float64)
    for a in range(len(ctu) - 1, -1, -1):
        for d in range(4):
            for k in range(2):
                out[d, k] = np.float64(out[d, k]) + np.float64(ctu["loss"][a, d, k])
    return out


@functools.lru_cache(maxsize=None)
def score_case(n_ctu=MANY, seed=31):
    """(traces [2], labels [2], reference CTU records [2], reference picture records [2], reference maps [2]) of two pictures with
    different content.  The walk of score_pic is long enough for its order to show: the same per-CTU sums added in reversed order
    give another double"""
    th = thresholds()
    w, h = size(n_ctu)
    assert n_ctu > 2 * th["score_ahead"] and n_ctu % th["score_ahead"] != 0 and n_ctu % th["score_ctus"] != 0      # many trips, a partial last one; a partial last workgroup
    pics = [score_picture(w, h, seed + 7 * i) for i in range(2)]
    traces, labels = [p[0] for p in pics], [p[1] for p in pics]
    ref = [cu_trace_ref.score(t, q, w, h) for t, q in zip(traces, labels)]
    for ctu, pic in ref:
        body = ctu[:-1]                                        # every CTU but the tail one
        assert (body["n"][:, 3] > 0).all() and (body["open"][:, 3] > 0).all() and (body["loss"][:, 3] > 0).all()
        assert int(ctu["n"][-1, 3].sum()) + int(ctu["open"][-1, 3]) == 1
        assert not ctu["n"][:, :3].any() and not ctu["loss"][:, :3].any()      # (no whole block above depth 3 in the strip)
        assert (reversed_sums(ctu)[3] != pic["v"][3, 4:]).any(), "the case does not tell the order of the sum: pick another seed"
    maps = [cu_trace_ref.maps(t, w, h) for t in traces]
    assert traces[0].tobytes() != traces[1].tobytes() and labels[0].tobytes() != labels[1].tobytes()
    for a in traces + labels + [q for r in ref for q in r] + [q for m in maps for q in m]:
        a.setflags(write=False)
    return traces, labels, [r[0] for r in ref], [r[1] for r in ref], maps


# ---- the decision maps and the N_OBF maps
def maps_case(seed=11):
    """maps_cases.case at 130 CTUs; the plans of risk_predict / nobf_blocks give level 3 more workgroups than any smaller case"""
    w, h = size(MANY)
    shapes = maps_ref.level_shapes(w, h)
    per = thresholds()["risk_pred_threads"]
    assert (shapes[3][0] * shapes[3][1] + per - 1) // per > 3 and (shapes[2][0] * shapes[2][1]) % per != 0
    return maps_cases.case(w, h, seed)


# ---- the risk-table model
def risk_plan(n_units):
    """(workgroups of risk_train, {units a wave takes: number of such waves}) from the exported constants"""
    th = thresholds()
    groups = min(th["risk_slots"], max(1, (n_units + th["risk_group_units"] - 1) // th["risk_group_units"]))
    assert groups == _emu().big_emu_risk_train_groups(n_units)
    stride, waves = groups * th["risk_waves"], {}
    for first in range(stride):
        k = len(range(first, n_units, stride))
        waves[k] = waves.get(k, 0) + 1
    return groups, waves


@functools.lru_cache(maxsize=None)
def risk_case(seed=7):
    """(traces [16], keys [16], reference model, dropped, {min_count: [labels per picture]}, the late sample's unit) of 16 pictures
    of the 130-CTU strip: the cap on the workgroups of risk_train binds, some waves take three units and some two.  Every picture
    carries the edge records of risk_cases.picture (checked on the first and the last alone); the last CTU of the last picture --
    a unit only a wave's third step reaches -- holds the one sample of the bin KEY_LATE, with a difference above 2^40 / 256"""
    th = thresholds()
    w, h = size(MANY)
    n_units = MANY * RISK_PICS
    groups, waves = risk_plan(n_units)
    assert groups == th["risk_slots"] and n_units > th["risk_slots"] * th["risk_group_units"], "the cap on the slots does not bind"
    assert set(waves) == {2, 3} and waves[2] > 0 and waves[3] > 0, waves
    for part in (RISK_SPLIT, RISK_PICS - RISK_SPLIT):          # the two calls of the accumulate split stay below the cap
        assert 1 < risk_plan(MANY * part)[0] < th["risk_slots"]
    pics = [risk_cases.picture(w, h, seed + 11 * i, i) for i in range(RISK_PICS)]
    traces, keys = [p[0] for p in pics], [p[1] for p in pics]
    late = [n for n in cu_trace_ref.nodes(w, h) if n[0] == MANY - 1 and n[2] == 3 and n[6]][-1]
    unit = (RISK_PICS - 1) * MANY + late[0]
    assert unit >= 2 * groups * th["risk_waves"], "no wave reaches the late sample in its third step"
    for k, v in dict(valid=1, split_tried=1, whole_tried=1, split_won=1, j0=3.0 * risk_cases.BIG, j1=1.0).items():
        traces[-1][k][late[0], late[1]] = v
    keys[-1][late[5]] = KEY_LATE
    for i in (0, RISK_PICS - 1):                               # (assert_edges looks for picture k's two-sample bin at position k of its batch)
        risk_cases.assert_edges(w, h, [traces[i]] * (i + 1), [keys[i]] * (i + 1), *risk_ref.train([traces[i]], [keys[i]], w, h))
    model, dropped = risk_ref.train(traces, keys, w, h)
    assert model["count"][3, KEY_LATE].tolist() == [0, 1] and model["risk"][3, KEY_LATE].tolist() == [0, risk_ref.Q_MAX]
    assert not model["count"][:3].any() and dropped > RISK_PICS
    labels = {m: [risk_ref.predict(k, model, m, w, h) for k in keys] for m in (1, 3)}
    for a in traces + keys + [model] + [q for v in labels.values() for q in v]:
        a.setflags(write=False)
    return traces, keys, model, dropped, labels, unit
