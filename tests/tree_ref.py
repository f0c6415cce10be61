"""Reference of the key tree (fcu_feature_bins, fcu_tree_keys, fcu_tree_hist, fcu_tree_split, fcu_tree_train) in plain numpy with
Python integers, written from the definitions in include/fcu.h.  It shares nothing with the kernel source: bins are counted edge by
edge, the samples come from risk_ref.samples (a walk over every block of every CTU), the histograms from np.add.at, the split choice
from Python integers."""
import numpy as np

import maps_ref
import risk_ref

BINS, MAX_LEVELS, NODES = 32, 5, 31
TREE = np.dtype([("levels", np.int32), ("feature", np.int16, (4, NODES)), ("thr", np.uint8, (4, NODES))])      # fcu_key_tree
assert TREE.itemsize == 376


def new_tree(levels=0):
    t = np.zeros((), TREE)
    t["levels"], t["feature"][...] = levels, -1
    return t


def level_rows(w, h):
    """[(first row, rows)] of level d = 0..3 in the NL layout"""
    out, o = [], 0
    for bh, bw in maps_ref.level_shapes(w, h):
        out.append((o, bh * bw))
        o += bh * bw
    return out


def bins(X, edges, w, h):
    """uint8 [NL, F]: per element the number of edges e of its (level, column) with e <= x"""
    X, edges = np.asarray(X, np.float32), np.asarray(edges, np.float32)
    out = np.zeros(X.shape, np.uint8)
    for d, (o, n) in enumerate(level_rows(w, h)):
        with np.errstate(invalid="ignore"):
            out[o:o + n] = (edges[d][None, :, :] <= X[o:o + n, :, None]).sum(axis=2)
    return out


def keys(b, tree, levels, w, h):
    """uint16 [NL]: the walk of `levels` steps per row"""
    out = np.zeros(b.shape[0], np.uint16)
    for d, (o, n) in enumerate(level_rows(w, h)):
        for r in range(o, o + n):
            i = 0
            for _ in range(levels):
                f = int(tree["feature"][d, i])
                i = 2 * i + 1 + (1 if f >= 0 and int(b[r, f]) > int(tree["thr"][d, i]) else 0)
            out[r] = i - ((1 << levels) - 1)
    return out


def hist(traces, bins_list, nodes_list, level, w, h, risk=None, count=None):
    """(risk int64, count uint32 [4, 2^level, F, 32, 2], dropped) of a batch, added to risk / count when given"""
    F = bins_list[0].shape[1]
    shape = (4, 1 << level, F, BINS, 2)
    risk = np.zeros(shape, np.int64) if risk is None else np.array(risk, np.int64)
    count = np.zeros(shape, np.int64) if count is None else np.array(count, np.int64)
    dropped, cols = 0, np.arange(F)
    for i, (tr, b) in enumerate(zip(traces, bins_list)):
        nodes = np.zeros(b.shape[0], np.uint16) if nodes_list is None else nodes_list[i]
        for d, node, truth, q, idx in risk_ref.samples(tr, nodes, w, h):
            if node >= 1 << level:
                dropped += 1
                continue
            np.add.at(risk, (d, node, cols, b[idx].astype(np.intp), truth), q)
            np.add.at(count, (d, node, cols, b[idx].astype(np.intp), truth), 1)
    assert count.max(initial=0) < 1 << 32
    return risk, count.astype(np.uint32), dropped


def split(risk, count, level, min_count, tree):
    """fills the nodes of `level` of `tree` in place; ValueError where fcu_tree_split gives FCU_ERR_ARG"""
    F = risk.shape[2]
    need = max(1, min_count)
    tot_r, tot_n = risk.astype(object).sum(axis=3), count.astype(object).sum(axis=3)      # [4, nodes, F, 2]
    if (tot_r != tot_r[:, :, :1]).any() or (tot_n != tot_n[:, :, :1]).any():
        raise ValueError("inconsistent totals")
    for d in range(4):
        for n in range(1 << level):
            R = [int(tot_r[d, n, 0, t]) for t in range(2)]
            NT = int(tot_n[d, n, 0].sum())
            best, bf, bb = min(R), -1, 0
            for f in range(F):
                L, NL = [0, 0], 0
                for b in range(BINS - 1):
                    L[0] += int(risk[d, n, f, b, 0])
                    L[1] += int(risk[d, n, f, b, 1])
                    NL += int(count[d, n, f, b].sum())
                    if NL < need or NT - NL < need:
                        continue
                    loss = min(L) + min(R[0] - L[0], R[1] - L[1])
                    if loss < best:
                        best, bf, bb = loss, f, b
            i = (1 << level) - 1 + n
            tree["feature"][d, i], tree["thr"][d, i] = bf, bb
    return tree


def train(traces, bins_list, levels, min_count, w, h):
    tree = new_tree(levels)
    for l in range(levels):
        nodes = [keys(b, tree, l, w, h) for b in bins_list] if l else None
        r, c, _ = hist(traces, bins_list, nodes, l, w, h)
        split(r, c, l, min_count, tree)
    return tree


def table_loss(model):
    """per depth the integer training loss of the risk table: the sum over bins of min(risk[0], risk[1])"""
    m = np.asarray(model).reshape(())
    return [int(np.minimum(m["risk"][d, :, 0], m["risk"][d, :, 1]).astype(object).sum()) for d in range(4)]
