"""Inputs of the key-tree tests, shared by the emulator tests (test_tree.py) and the GPU tests (test_gpu_tree.py), with the numpy
reference (tree_ref.py) computed once per case and set read-only.  Every builder asserts that the edge or the path it is named
after is really in the case -- the tiling from the enums tests/emu/tree_emu.cpp exports out of the kernel source -- so that no test
passes by leaving one out and a retuned constant fails the case instead of quietly shrinking what it covers."""
import ctypes as C
import functools
import os

import numpy as np

import cu_trace_ref
import features_cases
import labels_ref
import risk_cases
import risk_ref
import tree_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN_SIZES = [(208, 136), (72, 200), (64, 64)]               # (208, 136) and (72, 200): right and bottom CTUs partial, zero rows
SETS = {"tmv": (1, slice(0, 130)), "soc": (2, slice(130, 146)), "both": (3, slice(0, 146))}
HIST_LEVELS = (0, 2, 4)
STRIP = (64 * 129 + 8, 8)                                    # 130 CTUs in one row, 8 samples high: the strip of big_cases
STRIP_PICS = 16
# the two-level rule needs more depth-0 samples (one per CTU) than the one-level rule for the greedy root to be the planted one
PLANTED_SIZE = {"one": (512, 256), "two": (1024, 512)}


@functools.lru_cache(maxsize=None)
def emu():
    return C.CDLL(os.path.join(ROOT, "tests", "emu", "libtree_emu.so"))


def enums():
    L = emu()
    return {k: getattr(L, "tree_emu_" + k)() for k in ("threads", "bin_rows", "lds_cols", "chunk", "max_chunks", "fold_ahead", "fold_threads")}


def hist_plan(w, h, n_pics, F, level):
    out = (C.c_int * 12)()
    emu().tree_emu_hist_plan(w, h, n_pics, F, level, out)
    v = list(out)
    return {"tile": v[0], "n_tiles": v[1], "blocks": v[2:6], "chunk_off": v[6:11], "groups": v[11]}


def readonly(*arrays):
    for a in arrays:
        a.setflags(write=False)


# ---- 1. bins
def hand_edges(X, w, h, seed=5):
    """float32 [4, 146, 31] for the reference features X [NL, 146]: per (level, column) values taken from the column's own samples
    (edges exactly on samples), every third column with each edge repeated, and the constant column soc_0 with 31 equal edges"""
    rng = np.random.default_rng(seed)
    E = np.zeros((4, X.shape[1], tree_ref.BINS - 1), np.float32)
    for d, (o, n) in enumerate(tree_ref.level_rows(w, h)):
        for f in range(X.shape[1]):
            v = np.sort(X[o:o + n, f])
            e = v[np.sort(rng.integers(0, n, tree_ref.BINS - 1))]
            if f % 3 == 1:
                e = np.repeat(e[::2], 2)[:tree_ref.BINS - 1]
            E[d, f] = e
    return E


@functools.lru_cache(maxsize=None)
def bins_case(w, h):
    """(X float32 [NL, 146], edges [4, 146, 31], reference bins uint8 [NL, 146])"""
    X = np.array(features_cases.case(w, h, "textured")[3], np.float32)
    E = hand_edges(X, w, h)
    B = tree_ref.bins(X, E, w, h)
    assert np.all(np.diff(E, axis=2) >= 0) and np.isfinite(E).all()
    assert (np.diff(E, axis=2) == 0).any() and np.all(E[:, 130] == E[:, 130, :1])                      # repeated edges; a constant column
    assert any((X[:, f, None] == E[d, f][None, :]).any() for d in range(4) for f in (0, 7, 131))     # values exactly on edges
    if w % 64 or h % 64:
        assert (X == 0).all(axis=1).any()                                                             # zero rows of cut blocks
    assert B.max() == tree_ref.BINS - 1 and B.min() == 0
    readonly(X, E, B)
    return X, E, B


# ---- 2. keys
def hand_tree(levels, F, seed):
    """a seeded tree of `levels` levels with about a quarter of its nodes unsplit"""
    rng = np.random.default_rng(seed)
    t = tree_ref.new_tree(levels)
    t["feature"] = np.where(rng.random((4, tree_ref.NODES)) < 0.25, -1, rng.integers(0, F, (4, tree_ref.NODES)))
    t["thr"] = rng.integers(0, tree_ref.BINS - 1, (4, tree_ref.NODES))
    if levels:
        t["feature"][:, 0] = np.array([3, -1, F - 1, 0])[:4]       # a root that is not split at depth 1; the last column at depth 2
    return t


@functools.lru_cache(maxsize=None)
def keys_case(w, h, levels, walk):
    """(bins [NL, 146], tree of `levels` levels, reference keys of a walk of `walk` <= levels steps)"""
    B = bins_case(w, h)[2]
    t = hand_tree(levels, B.shape[1], 100 + levels)
    K = tree_ref.keys(B, t, walk, w, h)
    if walk >= 3:
        assert len(np.unique(K)) > 2 and (t["feature"][:, :(1 << walk) - 1] == -1).any()
    readonly(t, K)
    return B, t, K


# ---- 3. histograms
def random_bins(NL, F, seed):
    return np.random.default_rng(seed).integers(0, tree_ref.BINS, (NL, F)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def hist_case(w, h, n_pics, level, F=146, seed=3):
    """(traces, bins, nodes or None, reference risk, count, dropped): the seeded synthetic traces of risk_cases (valid, untried and
    whole_tried == 0 records, q at the clamp), random bins, random node indices of which a few lie past the level"""
    NL = labels_ref.label_count(w, h)
    traces = [risk_cases.picture(w, h, seed + 11 * i, i)[0] for i in range(n_pics)]
    bins = [random_bins(NL, F, seed + 100 + i) for i in range(n_pics)]
    rng = np.random.default_rng(seed + 7)
    nodes = None
    if level:
        nodes = [rng.integers(0, 1 << level, NL).astype(np.uint16) for _ in range(n_pics)]
        for k in nodes:
            k[rng.random(NL) < 0.05] = (1 << level) + rng.integers(0, 3)
    risk, count, dropped = tree_ref.hist(traces, bins, nodes, level, w, h)
    smp = [s for i, tr in enumerate(traces) for s in risk_ref.samples(tr, np.zeros(NL, np.uint16), w, h)]
    if w * h >= 128 * 64:
        assert any(s[3] == risk_ref.Q_MAX for s in smp) and (dropped > 0) == (level > 0)
        assert len(smp) < sum(1 for n in cu_trace_ref.nodes(w, h) if n[6]) * n_pics          # some records are no samples
    readonly(risk, count, *traces, *bins, *(nodes or []))
    return traces, bins, nodes, risk, count, dropped


# ---- 5. planted rules
@functools.lru_cache(maxsize=None)
def planted_case(rule, F=146, seed=17):
    """(trace, bins, N_OBF-like keys, reference tree) of one picture whose every record is a sample with a random q and
    rule "one": split_won = bin of column 37 > 12; rule "two": bin of column 3 > 15 and bin of column 140 > 10, at every depth.
    The other columns are random.  The builder asserts what the tests rely on."""
    w, h = PLANTED_SIZE[rule]
    rng = np.random.default_rng(seed)
    NL = labels_ref.label_count(w, h)
    n_ctu = ((w + 63) // 64) * ((h + 63) // 64)
    B = random_bins(NL, F, seed + 1)
    tr = np.zeros((n_ctu, 85), cu_trace_ref.CU_TRACE)
    tr["valid"], tr["split_tried"], tr["whole_tried"] = 1, 1, 1
    tr["j0"], tr["j1"] = rng.random((n_ctu, 85)) * 1e4 + 1.0, 0.0
    for a, t, d, x, y, idx, whole in cu_trace_ref.nodes(w, h):
        tr["split_won"][a, t] = (B[idx, 37] > 12) if rule == "one" else (B[idx, 3] > 15 and B[idx, 140] > 10)
    keys = np.array([rng.integers(0, (256 >> (2 * d)) + 1) for d, (o, n) in enumerate(tree_ref.level_rows(w, h)) for _ in range(n)], np.uint16)
    levels = 1 if rule == "one" else 2
    tree = tree_ref.train([tr], [B], levels, 1, w, h)
    if rule == "one":
        assert (tree["feature"][:, 0] == 37).all() and (tree["thr"][:, 0] == 12).all()
    else:
        assert (tree["feature"][:, 0] == 3).all() and (tree["thr"][:, 0] == 15).all() and (tree["feature"][:, 1] == -1).all()
        assert (tree["feature"][:, 2] == 140).all() and (tree["thr"][:, 2] == 10).all()
    K = tree_ref.keys(B, tree, levels, w, h)
    on_tree, on_nobf = risk_ref.train([tr], [K], w, h)[0], risk_ref.train([tr], [keys], w, h)[0]
    assert sum(tree_ref.table_loss(on_tree)) == 0 and all(x > 0 for x in tree_ref.table_loss(on_nobf))
    readonly(tr, B, keys, tree, K)
    return tr, B, keys, tree, K


# ---- 7. loops and caps
@functools.lru_cache(maxsize=None)
def strip_case(level, F=146, seed=29):
    """STRIP_PICS strips of 130 CTUs: (traces, bins, nodes, reference risk, count, dropped).  A strip has only depth-3 samples.
    Asserted from the kernels' enums: depth 3 has more chunks than the cap on workgroups per depth (so a workgroup takes a second
    and a third chunk, the last one partial), the slots of a depth are more than one trip of the fold, a level of one strip is more
    than one workgroup of feat_bins and of tree_keys with a partial last one, and the last column tile is partial."""
    w, h = STRIP
    E, P = enums(), hist_plan(w, h, STRIP_PICS, F, level)
    rows3 = tree_ref.level_rows(w, h)[3][1]
    chunks3 = -(-P["blocks"][3] // E["chunk"])
    assert P["blocks"][3] == rows3 * STRIP_PICS and chunks3 >= 2 * E["max_chunks"] + 1 and P["blocks"][3] % E["chunk"] != 0
    assert P["chunk_off"][4] - P["chunk_off"][3] == E["max_chunks"] > E["fold_ahead"]
    assert E["chunk"] // E["threads"] >= 2 and rows3 > E["bin_rows"] and rows3 % E["bin_rows"] and rows3 > E["threads"] and rows3 % E["threads"]
    assert P["tile"] == E["lds_cols"] >> level and F % P["tile"] != 0 and P["n_tiles"] >= 2 and P["groups"] == P["chunk_off"][4] * P["n_tiles"]
    return hist_case(w, h, STRIP_PICS, level, F, seed)


@functools.lru_cache(maxsize=None)
def all_depths_case(level, seed=31):
    """three 192 x 128 pictures: every depth has samples, each depth in the workgroups of several column tiles"""
    P = hist_plan(192, 128, 3, 146, level)
    assert all(b > 0 for b in P["blocks"]) and P["n_tiles"] >= 2
    case = hist_case(192, 128, 3, level, 146, seed)
    assert all(case[4][d].sum() > 0 for d in range(4))
    return case
