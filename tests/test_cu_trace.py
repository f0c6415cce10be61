"""The CU trace (fcu_chain_set_cu_trace), fcu_label_score and fcu_trace_maps on the emulator: the engine source with a trace bound
and the two kernels compiled for the CPU (tests/emu/cu_trace_emu.cpp).  The oracle has no trace; the records are pinned through what
it publishes -- its Verifying counters on OBF maps that single out one CU, and total_cost of pruned decisions.
tests/test_gpu_cu_trace.py repeats the core through the C ABI."""
import ctypes as C

import numpy as np
import pytest

import cu_trace_ref as ref
import hmo_py
import labels_ref
import maps_ref
from cu_trace_testlib import (ALL_OFF, ALL_ON, ERR_ARG, ERR_STATE, OK, PICS, assert_cu_pinned, assert_losses_close, emu_trace, emulate, inputs, n_ctus, oracle,  # noqa: F401
                              score_labels, single_cu_obf, trace_emu, whole_cus)

SCORE_PICS = ("i128", "cut")


# ---- the kernels through the emulator driver
def emu_score(lib, pic, traces, labels, stale=0x5C):
    """cu_trace_emu_score over n pictures of one size into buffers filled with `stale`: (per-CTU records [n, n_ctu], records [n])"""
    w, h = PICS[pic][:2]
    n, nc = len(traces), n_ctus(pic)
    tr = [np.ascontiguousarray(t) for t in traces]
    lb = [np.ascontiguousarray(q, np.int8) for q in labels]
    tp, lp = (C.c_void_p * n)(*[t.ctypes.data for t in tr]), (C.c_void_p * n)(*[q.ctypes.data for q in lb])
    ctu = np.frombuffer(bytes([stale]) * (n * nc * 128), np.uint8).copy().view(ref.CTU_SCORE).reshape(n, nc)
    rec = np.frombuffer(bytes([stale]) * (n * 224), np.uint8).copy().view(ref.PIC_SCORE)
    assert lib.cu_trace_emu_score(w, h, n, tp, lp, rec.ctypes.data, ctu.ctypes.data) == OK, lib.cu_trace_emu_last_error()
    return ctu, rec


def emu_maps(lib, pic, traces, shift=0, stale=0x33, want=(1, 1, 1)):
    """cu_trace_emu_maps with the label base moved by `shift` bytes and stale bytes under every output: (labels, j0, j1) [n, NL]"""
    w, h = PICS[pic][:2]
    n, NL = len(traces), labels_ref.label_count(w, h)
    tr = [np.ascontiguousarray(t) for t in traces]
    tp = (C.c_void_p * n)(*[t.ctypes.data for t in tr])
    bl = np.full(n * NL + shift + 8, stale, np.uint8)
    bj = [np.frombuffer(bytes([stale]) * (8 * (n * NL + 2)), np.uint8).copy().view(np.float64) for _ in range(2)]
    rc = lib.cu_trace_emu_maps(w, h, n, tp, bl.ctypes.data + shift if want[0] else None, bj[0].ctypes.data + 8 if want[1] else None, bj[1].ctypes.data + 8 if want[2] else None)
    assert rc == OK, lib.cu_trace_emu_last_error()
    assert np.all(bl[:shift] == stale) and np.all(bl[shift + n * NL:] == stale)      # nothing written outside
    for q in bj:
        assert np.all(q.view(np.uint8)[:8] == stale) and np.all(q.view(np.uint8)[-8:] == stale)
    return bl[shift:shift + n * NL].view(np.int8).reshape(n, NL).copy(), bj[0][1:-1].reshape(n, NL).copy(), bj[1][1:-1].reshape(n, NL).copy()


# ---- 1. the trace is a side output
@pytest.mark.parametrize("pic", ["i128", "cut", "p"])
def test_nothing_else_moves(trace_emu, pkg, pic):
    """with a trace bound, fcu_ctu_out, the reconstruction, the context states and the Verifying counters are byte for byte those
    without it -- Verifying on the random OBF map, and Testing with every switch on (where the depth-3 branch that zeroes J1 now runs
    because a trace is bound)"""
    w, h = PICS[pic][:2]
    obf = labels_ref.obf_maps(w, h)["random"]
    for state, dec in ((hmo_py.VERIFYING, None), (hmo_py.TESTING, (ALL_ON, ALL_ON, 0))):
        a = emulate(trace_emu, pkg, pic, state=state, obf=obf, decision=dec, trace=False)
        b = emulate(trace_emu, pkg, pic, state=state, obf=obf, decision=dec, trace=True)
        assert a["out"] == b["out"] and all(np.array_equal(p, q) for p, q in zip(a["rec"], b["rec"])), (pic, state)
        assert all(np.array_equal(s[0], t[0]) and s[1] == t[1] for s, t in zip(a["states"], b["states"])), (pic, state)
        assert a["verify"].tobytes() == b["verify"].tobytes() and (state != hmo_py.VERIFYING or a["verify"][:, :4].sum() > 0)
        assert b["trace"]["valid"].sum() > 0 and not b["trace"]["pad"].any()
    ex = oracle(pkg, pic)
    got = np.frombuffer(emu_trace(pkg, pic)["out"], np.dtype(hmo_py.Ctu))
    assert np.array_equal(got["total_cost"], ex["total_cost"]) and np.array_equal(got["depth"], np.frombuffer(ex["ctus"], np.dtype(hmo_py.Ctu))["depth"])


def test_the_trace_copy_stays_clear_of_everything_else(trace_emu):
    """fcu_chain_set_cu_trace uploads one pointer: its byte range is the end of the GPU descriptor, directly behind the label fields,
    and overlaps no other range a setter copies on its own, nor position, coder state, counters or search state; the copy of
    fcu_chain_set_decision, which runs to the end, covers it (the host descriptor holds the pointer too)"""
    r = (C.c_size_t * 24)()
    trace_emu.cu_trace_emu_ranges(r)
    rng = {n: (r[2 * i], r[2 * i + 1]) for i, n in enumerate(("cu_trace", "labels", "decision", "pu_trace", "col", "int_mv", "list0", "range", "ref"))}
    ver, state, next_ctu, end = (r[18], r[19]), (r[20], r[21]), r[22], r[23]
    off, ln = rng["cu_trace"]
    assert ln == 8 and off == rng["labels"][0] + rng["labels"][1] and off + ln == end
    for name in ("labels", "pu_trace", "col", "int_mv", "list0", "range", "ref"):
        o, l = rng[name]
        assert o + l <= off, name
    assert ver[0] + ver[1] <= off and state[0] + state[1] <= off and next_ctu + 8 <= off
    assert rng["decision"][0] < off and rng["decision"][0] + rng["decision"][1] >= off + ln


def test_index_and_layouts(trace_emu, built, pkg):
    lib = trace_emu
    assert [lib.cu_trace_emu_sizeof(k) for k in range(3)] == [24, 128, 224] == [ref.CU_TRACE.itemsize, ref.CTU_SCORE.itemsize, ref.PIC_SCORE.itemsize]
    e = pkg.engine
    assert (e.CU_TRACE_DTYPE, e.CTU_SCORE_DTYPE, e.PIC_SCORE_DTYPE) == (ref.CU_TRACE, ref.CTU_SCORE, ref.PIC_SCORE) and e.CUS_PER_CTU == 85
    L = C.CDLL(pkg.lib_path())
    assert [L.fcu_abi_sizeof(k) for k in (13, 14, 15, 16)] == [24, 128, 224, -1]
    seen = set()
    for d in range(4):
        for j in range(4 ** d):
            z = j << (8 - 2 * d)
            assert lib.cu_trace_emu_index(d, z) == ref.cu_index(d, z) == L.fcu_cu_index(d, z) == L.fcu_pu_index(d, 0, z) == (0, 1, 5, 21)[d] + j
            seen.add(ref.cu_index(d, z))
    assert seen == set(range(85))


# ---- 2. every record against the oracle
def _pin(pkg, pic, cus, tr):
    for a, t, d, x, y, idx in cus:
        r = tr[a, t]
        assert r["valid"] == 1, (pic, a, t)
        v = oracle(pkg, pic, hmo_py.VERIFYING, single_cu_obf(pic, d, x, y, not r["split_won"]))["verify"]
        assert_cu_pinned(v, r, d, (pic, a, t, d, x, y))


def test_every_cu_of_a_ctu_one_at_a_time_against_the_oracle(trace_emu, pkg):
    """64x64 I picture, 85 CUs.  For CU B with split_won 0 the oracle runs in Verifying on an OBF map that is positive on B's cells
    only: B is the one false positive of its depth, and FPLoss of that depth is |J0 - J1| of B's record exactly (one term added
    to 0.0).  For split_won 1 the complementary map makes B the one false negative.  This pins split_won and |J0 - J1| of all 85
    records independently"""
    tr = emu_trace(pkg, "one")["trace"]
    assert tr["valid"].all() and tr["split_tried"].all() and tr["whole_tried"].all() and 0 < tr["split_won"].sum() < 85
    _pin(pkg, "one", whole_cus("one"), tr)


@pytest.mark.parametrize("pic", ["cut", "p"])
def test_sampled_cus_of_a_cut_picture_and_of_a_p_picture_against_the_oracle(trace_emu, pkg, pic):
    """a seeded sample of 40 whole CUs; the cut picture never records a CU the edge cuts; the P picture has depth-3 CUs whose NxN
    was not tried (the best inter candidate has no residual): split_tried 0, J1 0.0, split_won 0 -- which the oracle's Verifying
    state counts with J1 = 0, so the pin holds for them as well"""
    tr = emu_trace(pkg, pic)["trace"]
    cus = whole_cus(pic)
    w, h = PICS[pic][:2]
    whole = {(a, t) for a, t, *_ in cus}
    for a in range(tr.shape[0]):
        for t in range(85):
            assert tr[a, t]["valid"] == ((a, t) in whole), (pic, a, t)
            if not tr[a, t]["valid"]:
                assert tr[a, t].tobytes() == bytes(24)          # cleared, never written
    untried = [c for c in cus if not tr[c[0], c[1]]["split_tried"]]
    assert all(c[2] == 3 and tr[c[0], c[1]]["j1"] == 0.0 and not tr[c[0], c[1]]["split_won"] for c in untried)
    assert bool(untried) == PICS[pic][3]
    rng = np.random.default_rng(2040)
    first = [c for c in cus if c[2] == 0][:2] + untried[:3]       # a depth-0 CU and an untried one are in every sample
    rest = [c for c in cus if c not in first]
    pick = first + [rest[i] for i in sorted(rng.choice(len(rest), 40 - len(first), replace=False))]
    assert {c[2] for c in pick} == {0, 1, 2, 3}
    _pin(pkg, pic, pick, tr)


@pytest.mark.parametrize("pic", SCORE_PICS)
def test_absolute_costs_at_depth_0(trace_emu, pkg, pic):
    """slices of one CTU: every CTU starts from the reset state whatever the CTUs before it decided.  Oracle in Testing on an all-zero
    OBF map with only sw_terminate[0] on: every whole CTU stays one CU, total_cost = J0 of its depth-0 record.  All-positive map with
    only sw_skip2nx2n[0] on: the whole-CU check is skipped, total_cost = J1.  Exhaustive: total_cost = split_won ? J1 : J0."""
    w, h = PICS[pic][:2]
    tr = emu_trace(pkg, pic, 0, 1)["trace"]
    zero, pos = np.zeros((h // 4, w // 4), np.int16), np.full((h // 4, w // 4), 3, np.int16)
    j0 = oracle(pkg, pic, hmo_py.TESTING, zero, ALL_OFF, (1, 0, 0, 0), slice_ctus=1)["total_cost"]
    j1 = oracle(pkg, pic, hmo_py.TESTING, pos, (1, 0, 0, 0), ALL_OFF, slice_ctus=1)["total_cost"]
    ex = oracle(pkg, pic, slice_ctus=1)["total_cost"]
    whole = [a for a, t, d, *_ in whole_cus(pic) if d == 0]
    assert whole and (pic != "cut" or len(whole) < n_ctus(pic))
    for a in whole:
        r = tr[a, 0]
        assert r["valid"] and r["whole_tried"] and r["split_tried"]
        assert r["j0"] == j0[a] and r["j1"] == j1[a] and ex[a] == (r["j1"] if r["split_won"] else r["j0"]), (pic, a, r, j0[a], j1[a], ex[a])


def test_a_picture_decided_twice_into_the_same_array_gives_the_same_bytes(trace_emu, pkg):
    first = emu_trace(pkg, "cut")["trace"]
    buf = first.copy()
    buf["valid"] = 7                                            # what an earlier, different picture might have left
    again = emulate(trace_emu, pkg, "cut", trace_buf=buf)["trace"]
    assert again.tobytes() == first.tobytes()


# ---- 3. the score
def _score_cases(pkg, pic):
    w, h = PICS[pic][:2]
    f, _ = inputs(pkg, pic)
    maps = dict(labels_ref.obf_maps(w, h))
    maps["prepass"] = hmo_py.obf_prepass(f[0])[0]
    return {k: np.ascontiguousarray(maps[k], np.int16) for k in ("positive", "zero", "prepass")}


@pytest.mark.parametrize("pic", SCORE_PICS)
def test_score_has_the_oracles_verifying_counters_without_deciding_again(trace_emu, pkg, pic):
    """labels an OBF map expresses (all positive, all zero, the pre-pass's own map) against the Training picture's trace: the oracle's
    Verifying counts exactly, its loss sums within 1e-9 relative (another order of the same non-negative terms); per CTU and per
    picture byte for byte the numpy reference"""
    w, h = PICS[pic][:2]
    tr = emu_trace(pkg, pic)["trace"]
    for name, obf in _score_cases(pkg, pic).items():
        lab = labels_ref.obf_labels(obf, w, h)
        ctu, rec = emu_score(trace_emu, pic, [tr], [lab])
        want = oracle(pkg, pic, hmo_py.VERIFYING, obf)["verify"]
        assert np.array_equal(rec["v"][0][:, :4], want[:, :4]) and want[:, :4].sum() > 0, (pic, name, rec["v"][0], want)
        assert_losses_close(rec["v"][0][:, 4:], want[:, 4:], (pic, name))
        assert np.array_equal(rec["scored"][0], want[:, :4].sum(axis=1)) and not rec["open"][0].any()
        rc, rp = ref.score(tr, lab, w, h)
        assert ctu[0].tobytes() == rc.tobytes() and rec[0].tobytes() == rp.tobytes(), (pic, name)


@pytest.mark.parametrize("pic", SCORE_PICS)
def test_score_losses_are_bit_for_bit_the_engines_when_every_chain_is_one_ctu(trace_emu, pkg, pic):
    """slice_ctus = 1: one chain per CTU.  The engine's own Verifying run adds a chain's terms depth by depth in z-order and the
    chains in order -- the order of the two kernels -- so all six counters are equal as bytes"""
    w, h = PICS[pic][:2]
    tr = emu_trace(pkg, pic, 0, 1)["trace"]
    for name in ("random", "positive"):
        lab = score_labels(pic, name)
        own = emulate(trace_emu, pkg, pic, 0, 1, state=hmo_py.VERIFYING, labels=lab, trace=False)["verify"]
        _, rec = emu_score(trace_emu, pic, [tr], [lab])
        assert rec["v"][0].tobytes() == own.tobytes() and own[:, 4:].sum() > 0, (pic, name, rec["v"][0], own)


def test_score_of_a_p_picture_leaves_out_what_was_not_tried(trace_emu, pkg):
    """a P picture has depth-3 CUs whose NxN was never tried.  The engine's (and the oracle's) Verifying state counts them, with
    J1 = 0; they are no sample of a split decision and the score takes only records with split_tried: depths 0..2 equal the oracle's
    counters, depth 3 is short by exactly those CUs, all of which the oracle counts as not split"""
    pic = "p"
    w, h = PICS[pic][:2]
    tr = emu_trace(pkg, pic)["trace"]
    untried = int((tr["valid"] & (tr["split_tried"] == 0)).sum())
    for name in ("positive", "zero"):
        obf = labels_ref.obf_maps(w, h)[name]
        lab = labels_ref.obf_labels(obf, w, h)
        ctu, rec = emu_score(trace_emu, pic, [tr], [lab])
        want = oracle(pkg, pic, hmo_py.VERIFYING, obf)["verify"]
        assert np.array_equal(rec["v"][0][:3, :4], want[:3, :4])
        assert_losses_close(rec["v"][0][:3, 4:], want[:3, 4:])
        k = 1 if name == "positive" else 2                      # predicted split -> FP, predicted whole -> TN
        short = want[3, :4] - rec["v"][0][3, :4]
        assert short[k] == untried > 0 and short.sum() == untried
        rc, rp = ref.score(tr, lab, w, h)
        assert ctu[0].tobytes() == rc.tobytes() and rec[0].tobytes() == rp.tobytes()


def test_score_of_two_pictures_open_labels_and_a_repeated_call(trace_emu, pkg):
    """two pictures in one call; labels with ABSENT, FORCED and a stray value go to `open` and nowhere else; a repeated call into
    buffers filled with other stale bytes gives identical bytes"""
    pic = "cut"
    w, h = PICS[pic][:2]
    t0, t1 = emu_trace(pkg, pic)["trace"], emu_trace(pkg, pic, 0, 1)["trace"]
    assert t0.tobytes() != t1.tobytes()
    lab0 = score_labels(pic, "random")
    lab1 = lab0.copy()
    rng = np.random.default_rng(5)
    hit = rng.random(lab1.size)
    lab1[hit < 0.15], lab1[(hit >= 0.15) & (hit < 0.3)], lab1[(hit >= 0.3) & (hit < 0.45)] = labels_ref.ABSENT, labels_ref.FORCED, 7
    lab1[0], lab1[1] = 7, labels_ref.ABSENT                     # (the two whole depth-0 CUs)
    ctu, rec = emu_score(trace_emu, pic, [t0, t1], [lab0, lab1])
    for i, (t, q) in enumerate(((t0, lab0), (t1, lab1))):
        rc, rp = ref.score(t, q, w, h)
        assert ctu[i].tobytes() == rc.tobytes() and rec[i].tobytes() == rp.tobytes(), i
    assert not rec["open"][0].any() and rec["open"][1].all()
    samples = np.array([sum(1 for a, t, d, *_ in whole_cus(pic) if d == dd and t1[a, t]["split_tried"]) for dd in range(4)])
    assert np.array_equal(rec["open"][1] + rec["scored"][1], samples)
    ctu2, rec2 = emu_score(trace_emu, pic, [t0, t1], [lab0, lab1], stale=0xC4)
    assert ctu2.tobytes() == ctu.tobytes() and rec2.tobytes() == rec.tobytes()


# ---- 4. the maps
@pytest.mark.parametrize("pic", ["i128", "cut", "p"])
def test_maps_of_an_exhaustive_picture(trace_emu, pkg, pic):
    """wherever fcu_decision_maps labels the chosen tree 0 or 1 the trace label says the same; FORCED is equal; on an exhaustive I
    picture no wholly-inside block is ABSENT (P: only depth-3 blocks whose NxN was not tried); byte for byte the numpy reference, at
    an odd base address as well, two pictures in a batch, each output on its own"""
    w, h = PICS[pic][:2]
    e = emu_trace(pkg, pic)
    tr = e["trace"]
    rec = np.frombuffer(e["out"], np.uint8)
    tree = labels_ref.flatten(maps_ref.picture_maps(pkg, rec, w, h, (), labels=True)["labels"])
    lab, j0, j1 = emu_maps(trace_emu, pic, [tr, tr[::-1].copy()])
    want = ref.maps(tr, w, h)
    for got, wnt in zip((lab[0], j0[0], j1[0]), want):
        assert got.tobytes() == wnt.tobytes()
    for got, wnt in zip((lab[1], j0[1], j1[1]), ref.maps(tr[::-1], w, h)):
        assert got.tobytes() == wnt.tobytes()
    on_tree = (tree == 0) | (tree == 1)
    untried = lab[0] == labels_ref.ABSENT
    assert np.array_equal(lab[0][on_tree & ~untried], tree[on_tree & ~untried]) and np.array_equal(lab[0] == labels_ref.FORCED, tree == labels_ref.FORCED)
    lv = maps_ref.split_levels(lab[0], w, h)
    for d in range(4):
        absent = lv[d][labels_ref.whole_mask(w, h, d)] == labels_ref.ABSENT
        assert not absent.any() or (PICS[pic][3] and d == 3)
    sampled = (lab[0] == 0) | (lab[0] == 1)                     # the discarded CUs are labelled too
    assert sampled[tree == labels_ref.ABSENT].sum() == (tree == labels_ref.ABSENT).sum() - (untried & (tree == labels_ref.ABSENT)).sum()
    assert not PICS[pic][3] or sampled.sum() > on_tree.sum()
    assert np.all(j0[0][lab[0] < 0] == 0) and np.all(j1[0][lab[0] == labels_ref.FORCED] == 0) and np.all(j0[0][(lab[0] == 0) | (lab[0] == 1)] > 0)
    odd = emu_maps(trace_emu, pic, [tr], shift=1, stale=0xC4)
    assert odd[0][0].tobytes() == lab[0].tobytes() and odd[1][0].tobytes() == j0[0].tobytes()
    only = emu_maps(trace_emu, pic, [tr], want=(0, 0, 1))
    assert only[2][0].tobytes() == j1[0].tobytes()


def test_maps_of_a_testing_state_picture(trace_emu, pkg):
    """the picture decided again in Testing with its own replayed labels and every switch on: the blocks below a terminated CU are
    ABSENT (never recorded), a terminated CU itself was not divided (split_tried 0: ABSENT as a sample, but valid with its J0), and
    the skipped whole-CU checks have whole_tried 0 and J0 = FCU_MAX_DOUBLE"""
    pic = "cut"
    w, h = PICS[pic][:2]
    full = emu_trace(pkg, pic)
    rec = np.frombuffer(full["out"], np.uint8)
    tree = labels_ref.raster_labels(maps_ref.raster(pkg, rec, w, h, "depth"), maps_ref.raster(pkg, rec, w, h, "part_size"), w, h)
    e = emulate(trace_emu, pkg, pic, state=hmo_py.TESTING, labels=tree, decision=(ALL_ON, ALL_ON, 0))
    tr = e["trace"]
    lab, j0, j1 = emu_maps(trace_emu, pic, [tr])
    for got, wnt in zip((lab[0], j0[0], j1[0]), ref.maps(tr, w, h)):
        assert got.tobytes() == wnt.tobytes()
    n_term = n_skip = 0
    for a, t, d, x, y, idx in whole_cus(pic):
        r, v = tr[a, t], int(tree[idx])
        assert r["valid"] == (v != labels_ref.ABSENT), (a, t, v)  # visited exactly the chosen tree
        if v == labels_ref.NOT_SPLIT:                           # TerminateCU: not divided / NxN not tried
            assert not r["split_tried"] and r["j1"] == 0.0 and not r["split_won"] and r["whole_tried"] and r["j0"] < ref.MAX_DOUBLE
            assert lab[0][idx] == labels_ref.ABSENT and j0[0][idx] == 0.0
            n_term += 1
        elif v == labels_ref.SPLIT:                             # Skip2Nx2N: the whole-CU check skipped
            assert r["split_tried"] and not r["whole_tried"] and r["j0"] == ref.MAX_DOUBLE and r["split_won"] and lab[0][idx] == labels_ref.SPLIT
            assert j0[0][idx] == ref.MAX_DOUBLE and j1[0][idx] == r["j1"] > 0
            n_skip += 1
        else:
            assert lab[0][idx] == labels_ref.ABSENT and r.tobytes() == bytes(24)
    assert n_term > 0 and n_skip > 0


# ---- 5. what the entry points refuse
def test_guards(trace_emu, pkg):
    lib = trace_emu
    buf = np.zeros(2 * 85, ref.CU_TRACE)
    got = C.c_void_p()
    hd = lib.cu_trace_emu_host(128, 64, 2)
    try:                                                      # nothing bound
        assert lib.cu_trace_emu_set_trace_one(hd, 2, buf.ctypes.data, None) == ERR_ARG and lib.cu_trace_emu_set_trace_one(hd, -1, buf.ctypes.data, None) == ERR_ARG
        assert lib.cu_trace_emu_set_trace_one(hd, 0, buf.ctypes.data, C.byref(got)) == ERR_STATE and b"fcu_chain_set_cu_trace" in lib.cu_trace_emu_last_error()
        assert b"not bound" in lib.cu_trace_emu_last_error() and not got.value
    finally:
        lib.cu_trace_emu_destroy(hd)
    f = [np.ascontiguousarray(q) for q in pkg.synth.mixed(128, 64, seed=9)]
    rec = [np.zeros_like(q) for q in f]
    out = (hmo_py.Ctu * 2)()
    hd = lib.cu_trace_emu_create(0, 128, 64, 32, 1, 0, *[q.ctypes.data for q in f], *[q.ctypes.data for q in rec], C.addressof(out), 0, 0.0, 0, 0, None, None, 0)
    try:
        assert lib.cu_trace_emu_set_trace_one(hd, 1, None, C.byref(got)) == OK and not got.value          # a chain starts without a trace
        assert lib.cu_trace_emu_set_trace_one(hd, 0, buf.ctypes.data, C.byref(got)) == OK and got.value == buf.ctypes.data
        assert lib.cu_trace_emu_set_trace_one(hd, 1, None, C.byref(got)) == OK and not got.value          # chain 0 alone
        assert lib.cu_trace_emu_set_trace_one(hd, 0, buf.ctypes.data + 4, C.byref(got)) == ERR_ARG and b"multiple of 8" in lib.cu_trace_emu_last_error()
        assert got.value == buf.ctypes.data
        assert lib.cu_trace_emu_set_trace_one(hd, 0, None, C.byref(got)) == OK and not got.value          # NULL stops
    finally:
        lib.cu_trace_emu_destroy(hd)
    tr, lab = np.zeros((2, 85), ref.CU_TRACE), np.zeros(labels_ref.label_count(128, 64), np.int8)
    one, none = (C.c_void_p * 1)(tr.ctypes.data), (C.c_void_p * 1)(None)
    labs = (C.c_void_p * 1)(lab.ctypes.data)
    rec1, ctu = np.zeros(1, ref.PIC_SCORE), np.zeros(2, ref.CTU_SCORE)
    for args, word in (((0, one, labs, rec1.ctypes.data), b"n_pics"), ((1, None, labs, rec1.ctypes.data), b"dev_trace is null"), ((1, one, None, rec1.ctypes.data), b"dev_labels is null"),
                       ((1, none, labs, rec1.ctypes.data), b"dev_trace[0]"), ((1, one, none, rec1.ctypes.data), b"dev_labels[0]"), ((1, one, labs, None), b"host_scores")):
        assert lib.cu_trace_emu_score(128, 64, *args, ctu.ctypes.data) == ERR_ARG and word in lib.cu_trace_emu_last_error(), word
    j = np.zeros(lab.size + 1, np.float64)
    for args, word in (((0, one, lab.ctypes.data, None, None), b"n_pics"), ((1, None, lab.ctypes.data, None, None), b"dev_trace is null"), ((1, none, lab.ctypes.data, None, None), b"dev_trace[0]"),
                       ((1, one, None, None, None), b"no output"), ((1, one, None, j.ctypes.data + 4, None), b"multiples of 8")):
        assert lib.cu_trace_emu_maps(128, 64, *args) == ERR_ARG and word in lib.cu_trace_emu_last_error(), word
