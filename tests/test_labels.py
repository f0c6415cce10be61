"""Caller-supplied split labels on the emulator (fcu_chain_set_labels, fcu_labels_from_rasters; the same engine and kernel source
compiled for the CPU, tests/emu/labels_emu.cpp) against the unchanged oracle: a label array an OBF map can express has a bit-exact
reference in hmo_set_decision with that OBF map.  tests/test_gpu_labels.py repeats the cases through the C ABI."""
import ctypes as C

import numpy as np
import pytest

import hmo_py
import labels_ref
import maps_ref
from labels_testlib import (CASE_QPS, CASES, DECISIONS, ALL_ON, ERR_ARG, ERR_STATE, OBF_NAMES, OK, assert_verify_equal, emulate, labels_emu,  # noqa: F401
                            obf_map, reference, sorted_ctx)
from tile_oracle import assert_picture_equal

I_CASE_QPS = [(c, q) for c, q in CASE_QPS if not CASES[c][5]]


def test_the_random_maps_make_both_labels_fire_at_every_depth():
    """the premise of the cases: among the CUs a Testing-state search visits, Skip2Nx2N and TerminateCU both occur at every depth;
    the labels hold FORCED exactly on the cut blocks and nothing but SPLIT / NOT_SPLIT elsewhere"""
    for case in CASES:
        w, h = CASES[case][:2]
        obf = obf_map(case, "random")
        assert all(v == {0, 1} for v in labels_ref.reached_labels(obf, w, h)), case
        lv = maps_ref.split_levels(labels_ref.obf_labels(obf, w, h), w, h)
        for d in range(4):
            whole = labels_ref.whole_mask(w, h, d)
            assert np.all(lv[d][~whole] == labels_ref.FORCED) and np.all(np.isin(lv[d][whole], (0, 1)))
    assert any(not labels_ref.whole_mask(136, 72, d).all() for d in range(3))


@pytest.mark.parametrize("obf_name", OBF_NAMES)
@pytest.mark.parametrize("case,qp", CASE_QPS)
def test_testing_state_from_labels_equals_the_oracle_on_the_obf_map(labels_emu, pkg, case, qp, obf_name):
    """labels bound and NO OBF map, Testing state: every fcu_ctu_out field, the reconstruction and the coder state after every
    chain equal the oracle's run of hmo_set_decision with the OBF map the labels were derived from -- all switches on and two
    seeded per-depth patterns, each with depth_exception 0 and 1"""
    w, h = CASES[case][:2]
    lab = labels_ref.obf_labels(obf_map(case, obf_name), w, h)
    trials = set()
    for dec in DECISIONS:
        ref = reference(pkg, case, qp, hmo_py.TESTING, obf_name, dec)
        e = emulate(labels_emu, pkg, case, qp, hmo_py.TESTING, labels=lab, decision=dec)
        assert_picture_equal(ref, e["out"], e["rec"], e["states"], sorted_ctx=sorted_ctx(case), tag=(case, qp, obf_name, dec))
        trials.add(e["trials"])
    if obf_name == "random":
        assert len(trials) > 1                               # the decisions differ in what they prune


@pytest.mark.parametrize("obf_name", OBF_NAMES)
@pytest.mark.parametrize("case,qp", CASE_QPS)
def test_verifying_state_counts_the_labels_as_the_oracle_counts_the_obf_map(labels_emu, pkg, case, qp, obf_name):
    """Verifying: the exhaustive decision, and g_iVerResult -- TP / FP / TN / FN exact, the RD-loss sums as doubles"""
    w, h = CASES[case][:2]
    lab = labels_ref.obf_labels(obf_map(case, obf_name), w, h)
    ref = reference(pkg, case, qp, hmo_py.VERIFYING, obf_name)
    e = emulate(labels_emu, pkg, case, qp, hmo_py.VERIFYING, labels=lab)
    assert_picture_equal(ref, e["out"], e["rec"], e["states"], sorted_ctx=sorted_ctx(case), tag=(case, qp, obf_name))
    assert ref.verify[:, :4].sum() > 0
    assert_verify_equal(e["verify"], ref.verify, (case, qp, obf_name))


@pytest.mark.parametrize("case,qp", CASE_QPS)
def test_labels_take_the_place_of_a_bound_obf_map(labels_emu, pkg, case, qp):
    """the order fcu.h names first: fcu_chain_set_decision with an OBF map, then the labels -- which decide, not the map (the
    all-positive map is bound, the labels say what the random map says)"""
    w, h = CASES[case][:2]
    lab = labels_ref.obf_labels(obf_map(case, "random"), w, h)
    dec = DECISIONS[0]
    ref = reference(pkg, case, qp, hmo_py.TESTING, "random", dec)
    e = emulate(labels_emu, pkg, case, qp, hmo_py.TESTING, labels=lab, obf=obf_map(case, "positive"), decision=dec)
    assert_picture_equal(ref, e["out"], e["rec"], e["states"], sorted_ctx=sorted_ctx(case), tag=(case, qp))


@pytest.mark.parametrize("code", [labels_ref.ABSENT, labels_ref.FORCED, 77])
@pytest.mark.parametrize("case,qp", CASE_QPS)
def test_no_prediction_is_the_exhaustive_search(labels_emu, pkg, case, qp, code):
    """an array of nothing but "no prediction" codes: Testing with all switches on gives the Training-state result bit for bit, and
    Verifying counts nothing"""
    w, h = CASES[case][:2]
    lab = np.full(labels_ref.label_count(w, h), code, np.int8)
    ref = reference(pkg, case, qp, hmo_py.TRAINING)
    for state in (hmo_py.TESTING, hmo_py.VERIFYING):
        e = emulate(labels_emu, pkg, case, qp, state, labels=lab, decision=(ALL_ON, ALL_ON, 0))
        assert_picture_equal(ref, e["out"], e["rec"], e["states"], sorted_ctx=sorted_ctx(case), tag=(case, qp, code, state))
        assert not e["verify"].any()


def _records(pkg, out_bytes):
    return np.frombuffer(out_bytes, np.uint8)


def decision_labels(pkg, out_bytes, w, h):
    """the labels of a decided picture as fcu_decision_maps writes them, by tests/maps_ref.py"""
    rec = _records(pkg, out_bytes)
    return labels_ref.raster_labels(maps_ref.raster(pkg, rec, w, h, "depth"), maps_ref.raster(pkg, rec, w, h, "part_size"), w, h)


def assert_replay_equal(ref, e, tag):
    """a replayed picture against the exhaustive reference: everything assert_picture_equal compares except total_bits and
    total_cost of the records, which may differ by the rounding of the split flags' bit counts (see the test below): at most one
    bit per split flag coded on the chosen tree, 21 nodes of levels 0..2 per CTU"""
    dt = np.dtype(hmo_py.Ctu)
    got, want = np.frombuffer(e["out"], dt).copy(), np.frombuffer(ref.ctus, dt)
    assert np.all(np.abs(got["total_bits"].astype(np.int64) - want["total_bits"].astype(np.int64)) <= 21), tag
    got["total_bits"], got["total_cost"] = want["total_bits"], want["total_cost"]
    assert_picture_equal(ref, got.tobytes(), e["rec"], e["states"], tag=tag)


@pytest.mark.parametrize("case,qp", I_CASE_QPS)
def test_replay_of_an_i_pictures_own_labels_gives_the_exhaustive_decision(labels_emu, pkg, case, qp):
    """Decide exhaustively, take the labels of the chosen tree, decide again in Testing with all switches on: the reconstruction, the
    coder state after every chain and every record field except total_bits / total_cost equal the ORACLE's exhaustive run.  Every
    candidate of a CU starts from the same [D][CI_CURR_BEST] snapshot, so not evaluating the loser changes neither the winner nor
    the state handed on; at depth 3 SPLIT is NxN.  The pruned search is cheaper.
    Narrowed from "every record field": the search counts a CU's split flag on the go-on coder as the last candidate EVALUATED
    left it (TEncCu.cpp:1380-1386 resets the bit counter but loads nothing), and resetBits keeps the Q15 remainder of that coder.
    A loser that is no longer evaluated leaves another remainder, so the whole-bit count of a split flag can round the other way
    by one: total_bits of a record moves by a few bits (measured on these pictures: -1 .. +2 per CTU) and total_cost with it.  The
    decision does not move: with its own labels every split on the tree is forced, and no mode decision inside a CU reads a split
    flag's cost.  (Not claimed for P pictures: a pruned search no longer advances the carried TZ start vectors.)"""
    w, h = CASES[case][:2]
    ref = reference(pkg, case, qp, hmo_py.TRAINING)
    full = emulate(labels_emu, pkg, case, qp, hmo_py.TRAINING)
    assert_picture_equal(ref, full["out"], full["rec"], full["states"], tag=(case, qp, "exhaustive"))
    lab = decision_labels(pkg, full["out"], w, h)
    e = emulate(labels_emu, pkg, case, qp, hmo_py.TESTING, labels=lab, decision=(ALL_ON, ALL_ON, 0))
    assert_replay_equal(ref, e, (case, qp, "replay"))
    assert e["trials"] < full["trials"]


# ---- fcu_labels_from_rasters
def _from_rasters(lib, w, h, depth, part, n_pics=1, shift=0, stale=0x33):
    """the emulated kernel with all three bases moved by `shift` bytes and stale bytes underneath the output"""
    NL = labels_ref.label_count(w, h)
    plane = (h // 4) * (w // 4)
    bd, bp, bo = (np.full(n * n_pics + shift + 8, stale, np.uint8) for n in (plane, plane, NL))
    bd[shift:shift + plane * n_pics] = np.asarray(depth, np.uint8).reshape(-1)
    if part is not None:
        bp[shift:shift + plane * n_pics] = np.asarray(part, np.int8).reshape(-1).view(np.uint8)
    rc = lib.labels_emu_from_rasters(w, h, n_pics, bd.ctypes.data + shift, None if part is None else bp.ctypes.data + shift, bo.ctypes.data + shift)
    assert rc == OK, lib.labels_emu_last_error()
    assert np.all(bo[:shift] == stale) and np.all(bo[shift + NL * n_pics:] == stale)      # nothing written outside
    return bo[shift:shift + NL * n_pics].view(np.int8).reshape(n_pics, NL).copy()


@pytest.mark.parametrize("shift", [0, 1, 2])
@pytest.mark.parametrize("w,h", [(256, 128), (136, 72)])
def test_labels_from_the_rasters_of_a_decided_picture(labels_emu, pkg, w, h, shift):
    """depth / part_size maps of a decided picture -> the labels fcu_decision_maps writes for it (tests/maps_ref.py), at every
    base alignment, two pictures in a batch; a second call over other stale bytes gives identical bytes; without part_size
    level 3 is NOT_SPLIT"""
    e = hmo_py.Encoder(*pkg.synth.mixed(w, h, seed=4), 37)
    e.compress_frame()
    rec = _records(pkg, e.all_ctus_bytes())
    depth, part = maps_ref.raster(pkg, rec, w, h, "depth"), maps_ref.raster(pkg, rec, w, h, "part_size")
    want = flat = labels_ref.flatten(maps_ref.picture_maps(pkg, rec, w, h, (), labels=True)["labels"])
    codes = {int(v) for v in np.unique(flat)}
    assert codes >= {0, 1} and (labels_ref.FORCED in codes) == bool(w % 64 or h % 64)
    depth2 = np.roll(depth, 16, axis=1)                       # a second picture: the first one moved by a CTU column
    got = _from_rasters(labels_emu, w, h, np.stack([depth, depth2]), np.stack([part, part]), n_pics=2, shift=shift)
    assert np.array_equal(got[0], want) and np.array_equal(got[0], labels_ref.raster_labels(depth, part, w, h))
    assert np.array_equal(got[1], labels_ref.raster_labels(depth2, part, w, h))
    again = _from_rasters(labels_emu, w, h, np.stack([depth, depth2]), np.stack([part, part]), n_pics=2, shift=shift, stale=0xC4)
    assert np.array_equal(again, got)
    no_ps = _from_rasters(labels_emu, w, h, depth, None, shift=shift)[0]
    assert np.array_equal(no_ps, labels_ref.raster_labels(depth, None, w, h))
    lv = maps_ref.split_levels(no_ps, w, h)
    assert not (lv[3] == labels_ref.SPLIT).any() and (maps_ref.split_levels(want, w, h)[3] == labels_ref.SPLIT).any()


def test_labels_from_rasters_refuses_what_the_header_says(labels_emu):
    d, o = np.zeros(32 * 16, np.uint8), np.zeros(200, np.int8)
    assert labels_emu.labels_emu_from_rasters(128, 64, 0, d.ctypes.data, None, o.ctypes.data) == ERR_ARG
    assert labels_emu.labels_emu_from_rasters(128, 64, 1, None, None, o.ctypes.data) == ERR_ARG and b"dev_depth" in labels_emu.labels_emu_last_error()
    assert labels_emu.labels_emu_from_rasters(128, 64, 1, d.ctypes.data, None, None) == ERR_ARG and b"dev_labels" in labels_emu.labels_emu_last_error()


# ---- the host rules (HostState of fcu_host.h: what fcu_chain_set_labels / fcu_chain_set_decision / fcu_label_count apply)
@pytest.mark.parametrize("w,h", [(128, 128), (136, 72), (3840, 2160), (8, 8)])
def test_label_count_of_whole_and_cut_pictures(labels_emu, w, h):
    hd = labels_emu.labels_emu_host(w, h, 1)
    try:
        want = sum(-(-w // s) * -(-h // s) for s in (64, 32, 16, 8))
        assert labels_emu.labels_emu_count(hd) == want == labels_ref.label_count(w, h)
    finally:
        labels_emu.labels_emu_destroy(hd)


def test_guards_of_set_labels_and_set_decision(labels_emu, pkg):
    lib = labels_emu
    lab, obf = np.zeros(labels_ref.label_count(128, 128), np.int8), np.zeros((32, 32), np.int16)
    hd = lib.labels_emu_host(128, 128, 2)
    try:                                                      # nothing bound
        assert lib.labels_emu_set_labels_one(hd, 2, lab.ctypes.data) == ERR_ARG and lib.labels_emu_set_labels_one(hd, -1, lab.ctypes.data) == ERR_ARG
        assert lib.labels_emu_set_labels_one(hd, 0, lab.ctypes.data) == ERR_STATE and b"not bound" in lib.labels_emu_last_error()
        assert lib.labels_emu_set_decision_one(hd, 0, hmo_py.TESTING, None) == ERR_ARG      # (as before: the map is asked for first)
        assert lib.labels_emu_set_decision_one(hd, 0, hmo_py.TESTING, obf.ctypes.data) == ERR_STATE
    finally:
        lib.labels_emu_destroy(hd)
    f = [np.ascontiguousarray(q) for q in pkg.synth.mixed(128, 128, seed=9)]
    rec = [np.zeros_like(q) for q in f]
    out = (hmo_py.Ctu * 4)()
    hd = lib.labels_emu_create(0, 128, 128, 32, 2, 0, *[q.ctypes.data for q in f], *[q.ctypes.data for q in rec], C.addressof(out), 0, 0.0, 0, 0, None, None, 0)
    try:
        nine = (C.c_int * 9)()
        assert lib.labels_emu_n(hd) == 2 and lib.labels_emu_chain(hd, 0, nine) == 0
        for state in (hmo_py.VERIFYING, hmo_py.TESTING):     # neither an OBF map nor labels
            assert lib.labels_emu_set_decision_one(hd, 0, state, None) == ERR_ARG and b"OBF map" in lib.labels_emu_last_error()
        assert lib.labels_emu_set_labels_one(hd, 0, None) == OK                              # unbinding what is not bound, in Training
        assert lib.labels_emu_set_labels_one(hd, 0, lab.ctypes.data) == OK
        assert lib.labels_emu_chain(hd, 0, nine) == 1 and lib.labels_emu_chain(hd, 1, (C.c_int * 9)()) == 0      # chain 0 alone
        assert list(nine)[:8] == [0, 4, 20, 84, 2, 4, 8, 16]                                 # level offsets and row lengths of 128 x 128
        assert lib.labels_emu_set_decision_one(hd, 0, hmo_py.TESTING, None) == OK            # labels bound: no map needed
        assert lib.labels_emu_chain(hd, 0, nine) == 1 and nine[8] == hmo_py.TESTING          # the decision left the binding alone
        assert lib.labels_emu_set_decision_one(hd, 1, hmo_py.TESTING, None) == ERR_ARG       # the other chain has none
        assert lib.labels_emu_set_labels_one(hd, 0, None) == ERR_STATE and b"cannot lose its labels" in lib.labels_emu_last_error()
        assert lib.labels_emu_chain(hd, 0, nine) == 1
        assert lib.labels_emu_set_decision_one(hd, 0, hmo_py.TESTING, obf.ctypes.data) == OK  # with a map underneath the labels may go
        assert lib.labels_emu_set_labels_one(hd, 0, None) == OK and lib.labels_emu_chain(hd, 0, nine) == 0
        assert lib.labels_emu_set_decision_one(hd, 0, hmo_py.TRAINING, None) == OK
    finally:
        lib.labels_emu_destroy(hd)


def test_the_label_copy_stays_clear_of_the_search_state(labels_emu):
    """fcu_chain_set_labels uploads the label fields alone: its byte range lies behind the device-only search state (int_mv_r), which
    the copy of fcu_chain_set_decision still covers -- the new fields sit at the end of that range and are mirrored
    in the host descriptor"""
    r = (C.c_size_t * 6)()
    labels_emu.labels_emu_ranges(r)
    lab_off, lab_len, dec_off, dec_len, mv_off, mv_len = list(r)
    assert lab_len == 8 + 8 * 4 and lab_off >= mv_off + mv_len
    assert dec_off < mv_off and dec_off + dec_len >= lab_off + lab_len
