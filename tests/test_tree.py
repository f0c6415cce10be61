"""The key tree on the emulator and the host functions: the kernel bodies of fcu_feature_bins, fcu_tree_keys and fcu_tree_hist
(csrc/fcu_tree.h) compiled for the CPU (tests/emu/tree_emu.cpp) and fcu_tree_split / fcu_tree_train's level loop against the
plain-numpy reference (tests/tree_ref.py).  Every comparison is an equality.  tests/test_gpu_tree.py repeats the device cases
through the C ABI."""
import ctypes as C

import numpy as np
import pytest

import hmo_py
import features_ref
import labels_ref
import risk_ref
import tree_cases
import tree_ref
from cu_trace_testlib import PICS, emu_trace, inputs, trace_emu  # noqa: F401
from test_risk import emu_train, load_emu as load_risk_emu

OK, ERR_ARG = 0, -2
_P = C.c_void_p
SIGNATURES = {"bins": ([C.c_int] * 4 + [_P] * 3, C.c_int), "keys": ([C.c_int] * 4 + [_P, _P, C.c_int, _P], C.c_int),
              "hist": ([C.c_int] * 5 + [_P] * 5 + [C.c_int, _P], C.c_int), "split": ([_P, _P, C.c_int, C.c_int, C.c_int, _P], C.c_int),
              "train": ([C.c_int] * 6 + [_P] * 3, C.c_int), "edges_check": ([_P, C.c_int], C.c_int), "last_error": ([], C.c_char_p),
              "sizeof": ([], C.c_int), "label_count": ([C.c_int] * 2, C.c_int)}


@pytest.fixture(scope="session")
def tree_emu(built):
    lib = tree_cases.emu()
    for name, (argtypes, restype) in SIGNATURES.items():
        f = getattr(lib, "tree_emu_" + name)
        f.argtypes, f.restype = argtypes, restype
    return lib


def ptrs(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def emu_bins(lib, w, h, X, E, mask, offset=0):
    """tree_emu_bins over poisoned bytes, the output `offset` bytes into its buffer; nothing outside is written"""
    X, E = np.ascontiguousarray(X, np.float32), np.ascontiguousarray(E, np.float32)
    out = np.full(X.size + 64, 0xA5, np.uint8)
    assert lib.tree_emu_bins(w, h, X.shape[0], mask, X.ctypes.data, E.ctypes.data, out.ctypes.data + offset) == OK, lib.tree_emu_last_error()
    assert np.all(out[:offset] == 0xA5) and np.all(out[offset + X.size:] == 0xA5)
    return out[offset:offset + X.size].reshape(X.shape).copy()


def emu_keys(lib, w, h, B, tree, levels, mask=3):
    B = np.ascontiguousarray(B, np.uint8)
    n = B.shape[0]
    out = np.full(n * B.shape[1] + 8, 0xA5A5, np.uint16)
    t = np.array(tree).reshape(())
    assert lib.tree_emu_keys(w, h, n, mask, B.ctypes.data, t.ctypes.data, levels, out.ctypes.data + 8) == OK, lib.tree_emu_last_error()
    assert np.all(out[:4] == 0xA5A5) and np.all(out[4 + n * B.shape[1]:] == 0xA5A5)
    return out[4:4 + n * B.shape[1]].reshape(n, B.shape[1]).copy()


def emu_hist(lib, w, h, traces, bins, nodes, level, mask=3, hist=None, accumulate=0):
    tr, bn = [np.ascontiguousarray(t) for t in traces], [np.ascontiguousarray(b) for b in bins]
    nd = [np.ascontiguousarray(k) for k in nodes] if nodes is not None else None
    shape = (4, 1 << level, bn[0].shape[1], 32, 2)
    risk, count = hist if hist is not None else (np.full(shape, -0x5A5A5A5A5A5A5A5B, np.int64), np.full(shape, 0xA5A5A5A5, np.uint32))
    dropped = C.c_uint32(0xDEAD)
    assert lib.tree_emu_hist(w, h, len(tr), mask, level, ptrs(tr), ptrs(bn), ptrs(nd) if nd else None, risk.ctypes.data, count.ctypes.data, accumulate, C.byref(dropped)) == OK, lib.tree_emu_last_error()
    return risk, count, dropped.value


def test_layout(tree_emu, built, pkg):
    e = pkg.engine
    assert tree_emu.tree_emu_sizeof() == 376 == tree_ref.TREE.itemsize == C.sizeof(e.KeyTree)
    L = C.CDLL(pkg.lib_path())
    assert L.fcu_abi_sizeof(18) == 376 and L.fcu_abi_sizeof(19) == -1
    t = e.KeyTree(3)
    assert bytes(t) == tree_ref.new_tree(3).tobytes()


# ---- 1. bins
@pytest.mark.parametrize("size", tree_cases.BIN_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("sets", sorted(tree_cases.SETS))
def test_bins_equal_the_reference(tree_emu, size, sets):
    """two pictures (the second one the first one's rows reversed inside every level would need new edges: it is the same picture
    twice, which checks the picture stride), F = 130, 16 and 146, the output at an even and at an odd byte"""
    w, h = size
    X, E, B = tree_cases.bins_case(w, h)
    mask, cols = tree_cases.SETS[sets]
    Xs, Es = np.ascontiguousarray(np.stack([X[:, cols], X[:, cols]])), np.ascontiguousarray(E[:, cols])
    for offset in (0, 1):
        got = emu_bins(tree_emu, w, h, Xs, Es, mask, offset)
        assert got[0].tobytes() == np.ascontiguousarray(B[:, cols]).tobytes() and got[1].tobytes() == got[0].tobytes(), offset


def test_bins_of_nan_and_infinity(tree_emu):
    w, h = 64, 64
    X, E, _ = tree_cases.bins_case(w, h)
    X = X.copy()
    X[0, 0], X[1, 1], X[2, 2] = np.nan, np.inf, -np.inf
    got = emu_bins(tree_emu, w, h, X[None], E, 3)[0]
    assert got.tobytes() == tree_ref.bins(X, E, w, h).tobytes() and got[0, 0] == 0 and got[1, 1] == 31 and got[2, 2] == 0


def test_edges_check(tree_emu):
    E = tree_cases.bins_case(64, 64)[1]
    assert tree_emu.tree_emu_edges_check(np.ascontiguousarray(E).ctypes.data, 3) == OK
    for bad, d, f, k in ((np.nan, 0, 0, 0), (np.inf, 3, 145, 30), (-1e30, 1, 7, 5)):
        e = E.copy()
        e[d, f, k] = bad
        assert tree_emu.tree_emu_edges_check(e.ctypes.data, 3) == ERR_ARG and ("host_edges[%d][%d]" % (d, f)).encode() in tree_emu.tree_emu_last_error()
    assert tree_emu.tree_emu_edges_check(None, 3) == ERR_ARG and tree_emu.tree_emu_edges_check(E.ctypes.data, 0) == ERR_ARG


# ---- 2. keys
@pytest.mark.parametrize("levels,walk", [(0, 0), (1, 1), (3, 3), (5, 5), (5, 2), (3, 0)])
def test_keys_equal_the_numpy_walk(tree_emu, levels, walk):
    w, h = 208, 136
    B, t, K = tree_cases.keys_case(w, h, levels, walk)
    got = emu_keys(tree_emu, w, h, np.stack([B, B[::-1]]), t, walk)
    assert got[0].tobytes() == K.tobytes() and got[1].tobytes() == tree_ref.keys(B[::-1], t, walk, w, h).tobytes()
    assert got.max() < 1 << walk


# ---- 3. histograms
@pytest.mark.parametrize("level", tree_cases.HIST_LEVELS)
@pytest.mark.parametrize("size,F", [((208, 136), 146), ((64, 64), 16)], ids=["208x136-146", "64x64-16"])
def test_hist_equals_add_at(tree_emu, size, F, level):
    """byte-equal histograms and `dropped` over poisoned bytes, a repeated call, and [A, B] == A then B with accumulate"""
    w, h = size
    mask = 3 if F == 146 else 2
    traces, bins, nodes, risk, count, dropped = tree_cases.hist_case(w, h, 2, level, F)
    r, c, d = emu_hist(tree_emu, w, h, traces, bins, nodes, level, mask)
    assert r.tobytes() == risk.tobytes() and c.tobytes() == count.tobytes() and d == dropped
    r2, c2, d2 = emu_hist(tree_emu, w, h, traces, bins, nodes, level, mask, hist=(r, c))
    assert r2.tobytes() == risk.tobytes() and c2.tobytes() == count.tobytes() and d2 == dropped
    a = emu_hist(tree_emu, w, h, traces[:1], bins[:1], nodes[:1] if nodes else None, level, mask)
    b = emu_hist(tree_emu, w, h, traces[1:], bins[1:], nodes[1:] if nodes else None, level, mask, hist=a[:2], accumulate=1)
    assert b[0].tobytes() == risk.tobytes() and b[1].tobytes() == count.tobytes() and a[2] + b[2] == dropped


@pytest.mark.parametrize("level", (0, 2))
def test_hist_summed_over_bins_is_the_risk_model_on_the_nodes(tree_emu, level):
    """the cross-check with fcu_risk_train: for every column, node n's cells summed over the bins are the model's bin n"""
    w, h = 208, 136
    traces, bins, nodes, risk, count, dropped = tree_cases.hist_case(w, h, 2, level)
    keys = nodes if nodes else [np.zeros(b.shape[0], np.uint16) for b in bins]
    model, _ = emu_train(load_risk_emu(), w, h, traces, keys)
    r, c, _ = emu_hist(tree_emu, w, h, traces, bins, nodes, level)
    mr, mc = model["risk"].reshape(4, 257, 2), model["count"].reshape(4, 257, 2)
    assert mc[:, :1 << level].sum() > 0                       # (nodes past the level are the model's further bins, and dropped here)
    for f in range(r.shape[2]):
        assert np.array_equal(r[:, :, f].sum(axis=2), mr[:, :1 << level]) and np.array_equal(c[:, :, f].sum(axis=2), mc[:, :1 << level]), f


# ---- 4. the split choice (host only)
def _split(lib, risk, count, level, min_count, tree=None):
    t = np.array(tree_ref.new_tree(5) if tree is None else tree).reshape(())
    r, c = np.ascontiguousarray(risk, np.int64), np.ascontiguousarray(count, np.uint32)
    return lib.tree_emu_split(r.ctypes.data, c.ctypes.data, r.shape[2], level, min_count, t.ctypes.data), t


def _hand(F=3, level=0):
    return np.zeros((4, 1 << level, F, 32, 2), np.int64), np.zeros((4, 1 << level, F, 32, 2), np.uint32)


def _put(r, c, d, n, rows):
    """rows: (bins per column, truth, q) of single samples"""
    for bins, t, q in rows:
        for f, b in enumerate(bins):
            r[d, n, f, b, t] += q
            c[d, n, f, b, t] += 1


def test_split_hand_tables(tree_emu):
    r, c = _hand()
    # depth 0: columns 1 and 2 separate perfectly, column 1 at thresholds 4..8, column 2 at 0: the tie goes to f = 1, b = 4
    _put(r, c, 0, 0, [((0, 4, 0), 0, 10), ((0, 4, 0), 0, 7), ((0, 9, 1), 1, 5), ((0, 9, 1), 1, 3)])
    # depth 1: no gain -- every sample has truth 1, min(R) = 0 already
    _put(r, c, 1, 0, [((1, 2, 3), 1, 9), ((5, 6, 7), 1, 4)])
    # depth 2: no samples.  depth 3: the only separating threshold leaves one sample on the left: refused by min_count 2, taken by 1
    _put(r, c, 3, 0, [((3, 0, 0), 0, 8), ((9, 0, 0), 1, 6), ((9, 0, 0), 1, 2), ((9, 0, 0), 0, 1)])
    rc, t = _split(tree_emu, r, c, 0, 1)
    assert rc == OK and list(t["feature"][:, 0]) == [1, -1, -1, 0] and list(t["thr"][:, 0]) == [4, 0, 0, 3]
    want = tree_ref.split(r, c, 0, 1, tree_ref.new_tree(5))
    assert t.tobytes() == want.tobytes()
    rc, t2 = _split(tree_emu, r, c, 0, 2)
    assert rc == OK and list(t2["feature"][:, 0]) == [1, -1, -1, -1] and t2.tobytes() == tree_ref.split(r, c, 0, 2, tree_ref.new_tree(5)).tobytes()
    # min_count on the right child: mirror depth 3
    r3, c3 = _hand()
    _put(r3, c3, 3, 0, [((3, 0, 0), 0, 8), ((3, 0, 0), 0, 2), ((3, 0, 0), 1, 1), ((9, 0, 0), 1, 6)])
    assert _split(tree_emu, r3, c3, 0, 2)[1]["feature"][3, 0] == -1 and _split(tree_emu, r3, c3, 0, 1)[1]["feature"][3, 0] == 0
    # only the nodes of the level are written; the rest of the tree stays
    keep = tree_cases.hand_tree(5, 3, 9)
    rc, t4 = _split(tree_emu, r, c, 0, 1, keep)
    assert rc == OK and np.array_equal(t4["feature"][:, 1:], keep["feature"][:, 1:]) and np.array_equal(t4["thr"][:, 1:], keep["thr"][:, 1:]) and t4["levels"] == 5
    # inconsistent totals: a histogram of another shape
    bad = r.copy()
    bad[0, 0, 2, 5, 1] += 1
    rc, _ = _split(tree_emu, bad, c, 0, 1)
    assert rc == ERR_ARG and b"totals" in tree_emu.tree_emu_last_error()
    with pytest.raises(ValueError):
        tree_ref.split(bad, c, 0, 1, tree_ref.new_tree(5))
    for args, word in (((None, c.ctypes.data, 3, 0, 1, t.ctypes.data), b"host_risk"), ((r.ctypes.data, None, 3, 0, 1, t.ctypes.data), b"host_count"), ((r.ctypes.data, c.ctypes.data, 0, 0, 1, t.ctypes.data), b"F is"),
                       ((r.ctypes.data, c.ctypes.data, 3, 5, 1, t.ctypes.data), b"level"), ((r.ctypes.data, c.ctypes.data, 3, 0, -1, t.ctypes.data), b"min_count"), ((r.ctypes.data, c.ctypes.data, 3, 0, 1, None), b"tree is null")):
        assert tree_emu.tree_emu_split(*args) == ERR_ARG and word in tree_emu.tree_emu_last_error(), word


def test_split_through_the_library_needs_no_gpu(pkg, built):
    r, c = _hand()
    _put(r, c, 0, 0, [((0, 4, 0), 0, 10), ((0, 9, 1), 1, 5)])
    t = pkg.engine.tree_split(r, c, 0, pkg.engine.KeyTree(1))
    assert bytes(t) == tree_ref.split(r, c, 0, 1, tree_ref.new_tree(1)).tobytes()
    bad = r.copy()
    bad[0, 0, 1, 0, 0] += 1
    with pytest.raises(pkg.engine.FcuError, match="totals"):
        pkg.engine.tree_split(bad, c, 0, pkg.engine.KeyTree(1))


# ---- 5. planted rules
def emu_tree_train(lib, w, h, traces, bins, levels, min_count=1, mask=3):
    tr, bn = [np.ascontiguousarray(t) for t in traces], [np.ascontiguousarray(b) for b in bins]
    t = np.frombuffer(b"\xA5" * 376, np.uint8).copy().view(tree_ref.TREE)
    assert lib.tree_emu_train(w, h, len(tr), mask, levels, min_count, ptrs(tr), ptrs(bn), t.ctypes.data) == OK, lib.tree_emu_last_error()
    return t[0]


@pytest.mark.parametrize("rule", ["one", "two"])
def test_planted_rule_is_found(tree_emu, rule):
    w, h = tree_cases.PLANTED_SIZE[rule]
    tr, B, nobf_keys, tree, K = tree_cases.planted_case(rule)
    got = emu_tree_train(tree_emu, w, h, [tr], [B], int(tree["levels"]))
    assert got.tobytes() == tree.tobytes()
    keys = emu_keys(tree_emu, w, h, B[None], got, int(got["levels"]))[0]
    assert keys.tobytes() == K.tobytes()
    model, dropped = emu_train(load_risk_emu(), w, h, [tr], [keys])
    assert dropped == 0 and sum(tree_ref.table_loss(model)) == 0


# ---- 6. monotone on a real picture
def test_real_picture_training_loss_never_increases(tree_emu, pkg):
    """128 x 64, decided exhaustively with a trace (the emulated engine); features of the reference, the driver's default edges"""
    import torch
    w, h = PICS["i128"][:2]
    tr = emu_trace(pkg, "i128")["trace"]
    Y = np.ascontiguousarray(inputs(pkg, "i128")[0][0])
    X = features_ref.feature_maps(Y, ("tmv", "soc"), np.ascontiguousarray(hmo_py.obf_prepass(Y)[1], np.float64)).astype(np.float32)
    E = pkg.engine.feature_edges(torch.as_tensor(X[None]), w, h).numpy()
    E2 = pkg.engine.feature_edges(torch.as_tensor(X[None]), w, h).numpy()
    assert E.tobytes() == E2.tobytes() and E.shape == (4, 146, 31) and np.isfinite(E).all() and np.all(np.diff(E, axis=2) >= 0)
    assert tree_emu.tree_emu_edges_check(np.ascontiguousarray(E).ctypes.data, 3) == OK
    B = emu_bins(tree_emu, w, h, X[None], E, 3)[0]
    assert B.tobytes() == tree_ref.bins(X, E, w, h).tobytes()
    tree5 = tree_ref.train([tr], [B], 5, 1, w, h)
    prev = None
    for levels in range(6):
        t = emu_tree_train(tree_emu, w, h, [tr], [B], levels)
        want = tree_ref.new_tree(levels)
        n = (1 << levels) - 1
        want["feature"][:, :n], want["thr"][:, :n] = tree5["feature"][:, :n], tree5["thr"][:, :n]      # training is greedy: a prefix
        assert t.tobytes() == want.tobytes(), levels
        keys = emu_keys(tree_emu, w, h, B[None], t, levels)[0]
        model, dropped = emu_train(load_risk_emu(), w, h, [tr], [keys])
        model = model.reshape(())
        loss = tree_ref.table_loss(model)
        print("levels %d: loss per depth %s" % (levels, loss))
        if levels == 0:
            assert loss == [int(min(model["risk"][d, 0, 0], model["risk"][d, 0, 1])) for d in range(4)]
        else:
            assert all(a <= b for a, b in zip(loss, prev)), (levels, loss, prev)
        prev = loss
    assert dropped == 0


# ---- 7. loops and caps
@pytest.mark.parametrize("level", (0, 4))
def test_strips_cross_the_chunk_cap_and_the_fold_trip(tree_emu, level):
    w, h = tree_cases.STRIP
    traces, bins, nodes, risk, count, dropped = tree_cases.strip_case(level)
    r, c, d = emu_hist(tree_emu, w, h, traces, bins, nodes, level)
    assert r.tobytes() == risk.tobytes() and c.tobytes() == count.tobytes() and d == dropped
    assert count[:3].sum() == 0 and count[3].sum() > 0


def test_strip_bins_and_keys_take_several_workgroups(tree_emu):
    w, h = tree_cases.STRIP
    tree_cases.strip_case(0)                                  # (asserts the row counts against the enums)
    NL = labels_ref.label_count(w, h)
    rng = np.random.default_rng(4)
    X = rng.integers(-40, 40, (2, NL, 16)).astype(np.float32)
    E = np.sort(rng.integers(-40, 40, (4, 16, 31)), axis=2).astype(np.float32)
    B = emu_bins(tree_emu, w, h, X, E, 2, offset=1)
    assert all(B[i].tobytes() == tree_ref.bins(X[i], E, w, h).tobytes() for i in range(2))
    t = tree_cases.hand_tree(5, 16, 77)
    K = emu_keys(tree_emu, w, h, B, t, 5, mask=2)
    assert all(K[i].tobytes() == tree_ref.keys(B[i], t, 5, w, h).tobytes() for i in range(2))


@pytest.mark.parametrize("level", (0, 4))
def test_every_depth_has_samples(tree_emu, level):
    traces, bins, nodes, risk, count, dropped = tree_cases.all_depths_case(level)
    r, c, d = emu_hist(tree_emu, 192, 128, traces, bins, nodes, level)
    assert r.tobytes() == risk.tobytes() and c.tobytes() == count.tobytes() and d == dropped


# ---- 8. argument rules and the driver's option rules
def test_refusals_name_their_argument(tree_emu):
    w, h = 64, 64
    NL = labels_ref.label_count(w, h)
    traces, bins, nodes, _, _, _ = tree_cases.hist_case(w, h, 2, 2, 16)
    X, E, B = np.zeros((NL, 16), np.float32), np.zeros((4, 16, 31), np.float32), np.ascontiguousarray(bins[0])
    out8, out16 = np.zeros(NL * 16 + 8, np.uint8), np.zeros(NL + 8, np.uint16)
    L, xp, ep, op = tree_emu, X.ctypes.data, E.ctypes.data, out8.ctypes.data
    for args, word in (((0, 2, xp, ep, op), b"n_pics"), ((1, 4, xp, ep, op), b"sets"), ((1, 0, xp, ep, op), b"sets"), ((1, 2, None, ep, op), b"dev_features is null"),
                       ((1, 2, xp + 2, ep, op), b"dev_features starts"), ((1, 2, xp, None, op), b"dev_edges is null"), ((1, 2, xp, ep, None), b"dev_bins is null"),
                       (((1 << 22) // NL + 1, 2, xp, ep, op), b"2^22")):
        assert L.tree_emu_bins(w, h, *args) == ERR_ARG and word in L.tree_emu_last_error(), word
    t = np.array(tree_cases.hand_tree(3, 16, 1)).reshape(())
    bad_f, bad_t, bad_l = t.copy(), t.copy(), t.copy()
    bad_f["feature"][2, 5], bad_t["thr"][1, 1], bad_l["levels"] = 16, 31, 6
    bp, tp, kp = B.ctypes.data, t.ctypes.data, out16.ctypes.data
    for args, word in (((0, 2, bp, tp, 3, kp), b"n_pics"), ((1, 8, bp, tp, 3, kp), b"sets"), ((1, 2, None, tp, 3, kp), b"dev_bins is null"), ((1, 2, bp, None, 3, kp), b"host_tree is null"),
                       ((1, 2, bp, bad_f.ctypes.data, 3, kp), b"feature"), ((1, 2, bp, bad_t.ctypes.data, 3, kp), b"thr"), ((1, 2, bp, bad_l.ctypes.data, 3, kp), b"levels"),
                       ((1, 2, bp, tp, 4, kp), b"levels is 0"), ((1, 2, bp, tp, -1, kp), b"levels is 0"), ((1, 2, bp, tp, 3, None), b"dev_keys is null"), ((1, 2, bp, tp, 3, kp + 1), b"even byte")):
        assert L.tree_emu_keys(w, h, *args) == ERR_ARG and word in L.tree_emu_last_error(), word
    tr, bn, nd, none = ptrs([np.ascontiguousarray(traces[0])]), ptrs([B]), ptrs([np.ascontiguousarray(nodes[0])]), (C.c_void_p * 1)(None)
    r, c = np.zeros((4, 4, 16, 32, 2), np.int64), np.zeros((4, 4, 16, 32, 2), np.uint32)
    rp, cp = r.ctypes.data, c.ctypes.data
    for args, word in (((0, 2, 2, tr, bn, nd, rp, cp, 0), b"n_pics"), ((1, 5, 2, tr, bn, nd, rp, cp, 0), b"sets"), ((1, 2, 5, tr, bn, nd, rp, cp, 0), b"level is"), ((1, 2, -1, tr, bn, nd, rp, cp, 0), b"level is"),
                       ((1, 2, 2, None, bn, nd, rp, cp, 0), b"dev_trace is null"), ((1, 2, 2, tr, None, nd, rp, cp, 0), b"dev_bins is null"), ((1, 2, 2, tr, bn, None, rp, cp, 0), b"dev_nodes is null"),
                       ((1, 2, 2, none, bn, nd, rp, cp, 0), b"dev_trace[0]"), ((1, 2, 2, tr, none, nd, rp, cp, 0), b"dev_bins[0]"), ((1, 2, 2, tr, bn, none, rp, cp, 0), b"dev_nodes[0]"),
                       ((1, 2, 2, tr, bn, nd, None, cp, 0), b"dev_risk is null"), ((1, 2, 2, tr, bn, nd, rp + 4, cp, 0), b"dev_risk starts"), ((1, 2, 2, tr, bn, nd, rp, None, 0), b"dev_count is null"),
                       ((1, 2, 2, tr, bn, nd, rp, cp + 2, 0), b"dev_count starts"), ((1, 2, 2, tr, bn, nd, rp, cp, 2), b"accumulate")):
        assert L.tree_emu_hist(w, h, *args, None) == ERR_ARG and word in L.tree_emu_last_error(), word
    assert L.tree_emu_hist(w, h, 1, 2, 0, tr, bn, None, rp, cp, 0, None) == OK                       # no nodes at level 0
    for args, word in (((0, 2, 2, 1, tr, bn, tp), b"n_pics"), ((1, 0, 2, 1, tr, bn, tp), b"sets"), ((1, 2, 6, 1, tr, bn, tp), b"levels is"), ((1, 2, 2, -1, tr, bn, tp), b"min_count"),
                       ((1, 2, 2, 1, None, bn, tp), b"dev_trace is null"), ((1, 2, 2, 1, tr, none, tp), b"dev_bins[0]"), ((1, 2, 2, 1, tr, bn, None), b"host_tree is null")):
        assert L.tree_emu_train(w, h, *args) == ERR_ARG and word in L.tree_emu_last_error(), word


def test_sequence_decider_option_rules(pkg):
    S = pkg.sequence.SequenceDecider
    for kw in (dict(risk={"tree": {"levels": 6}}), dict(risk={"tree": {"levels": -1}}), dict(risk={"tree": {"levels": 2, "depth": 3}}), dict(risk={"tree": 3}),
               dict(risk={"tree": {"levels": 2}, "key": lambda *a: None}), dict(risk={"tree": {"levels": 2, "min_count": -1}}), dict(risk={"tree": {"levels": 2, "sets": ("dct",)}}),
               dict(risk={"tree": {"levels": 2}}, fast=False)):
        with pytest.raises(ValueError, match="risk"):
            S(64, 64, 32, **kw)
