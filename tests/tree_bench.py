"""Times the key-tree kernels at 4K on one MI355X and writes profiles/tree_bench.json (python tests/tree_bench.py --out ...).
One and sixteen pictures, F = 146, medians of --reps runs with min and max, after a warm-up call of everything.  Kernel times are
the library's own stream events (timed=True): feat_bins, tree_hist and tree_fold at levels 0 and 4, tree_keys at 5 levels, and all
kernels of fcu_tree_train at 5 levels added up, with the call's wall time (which includes the copies of the histograms to the host
and the split choice) next to it.  Per kernel the ALGORITHMIC bytes (from the shapes) over the kernel time and their share of the
HBM rate an MI355X sustains (cu_trace_bench.HBM_SUSTAINED).  The host path the kernels replace is timed on the same data: features
and traces copied to the host, np.searchsorted per (level, column), np.add.at for the level-0 histograms.  Synthetic traces and
luma planes: the times do not depend on the values, but for the LDS adds of tree_hist, which random bins spread evenly."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cu_trace_bench import HBM_SUSTAINED, node_elements  # noqa: E402


def host_path(X, E, tr, idx, whole, rows):
    """bins by np.searchsorted and the level-0 histograms by np.add.at for one picture's host copies"""
    B = np.zeros(X.shape, np.uint8)
    for d, (o, n) in enumerate(rows):
        for f in range(X.shape[1]):
            B[o:o + n, f] = np.searchsorted(E[d, f], X[o:o + n, f], side="right")
    depth = np.repeat(np.arange(4), (1, 4, 16, 64))[None, :]
    smp = whole & (tr["valid"] != 0) & (tr["split_tried"] != 0) & (tr["whole_tried"] != 0)
    s = np.abs(tr["j0"] - tr["j1"]) * 256.0
    q = np.where(s < 2.0 ** 40, np.floor(np.where(s < 2.0 ** 40, s, 0.0)), 2.0 ** 40 - 1).astype(np.int64)
    risk, count = np.zeros((4, X.shape[1], 32, 2), np.int64), np.zeros((4, X.shape[1], 32, 2), np.int64)
    d_s, t_s, q_s, b_s = np.broadcast_to(depth, smp.shape)[smp], (tr["split_won"] != 0)[smp].astype(np.intp), q[smp], B[idx[smp]]
    cols = np.arange(X.shape[1])[None, :]
    np.add.at(risk, (d_s[:, None], cols, b_s, t_s[:, None]), q_s[:, None])
    np.add.at(count, (d_s[:, None], cols, b_s, t_s[:, None]), 1)
    return B, risk, count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pics", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    e = pkg.engine
    w, h, F = 3840, 2160, 146
    dev = torch.device("cuda", 0)
    q = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}
    res = {"width": w, "height": h, "F": F, "device": torch.cuda.get_device_name(0), "hbm_sustained_Bps": HBM_SUSTAINED, "reps": args.reps, "batches": []}
    eng = pkg.CuEngine(w, h, max_chains=1)
    n_ctu, NL = eng.n_ctu, eng.label_count()
    rng = np.random.default_rng(7)
    idx, whole, nl = node_elements(w, h)
    assert nl == NL
    rows, o = [], 0
    for bh, bw in e.map_level_shapes(w, h):
        rows.append((o, bh * bw))
        o += bh * bw
    n_max = max(args.pics)
    host_tr = np.zeros((n_max, n_ctu, 85), e.CU_TRACE_DTYPE)
    host_tr["j0"], host_tr["j1"] = rng.random(host_tr.shape) * 1e5, rng.random(host_tr.shape) * 1e5
    host_tr["valid"], host_tr["split_tried"], host_tr["whole_tried"] = whole[None], whole[None], whole[None]
    host_tr["split_won"] = rng.integers(0, 2, host_tr.shape) * whole[None]
    traces = [torch.as_tensor(host_tr[i].view(np.uint8).reshape(-1)).to(dev) for i in range(n_max)]
    lumas = [torch.as_tensor(rng.integers(0, 256, (h, w)).astype(np.uint8)).to(dev) for _ in range(n_max)]
    X_all = eng.feature_maps(lumas, yc=np.full((n_max, 16), 2.0))
    for n in args.pics:
        tb, X = traces[:n], X_all[:n].contiguous()
        E = e.feature_edges(X, w, h)
        B = eng.feature_bins(X, E)                             # warm-up of every call + the checks against the host path
        tree = eng.tree_train(tb, B, 5)
        nodes4 = eng.tree_keys(B, tree, 4)
        r0, c0, _ = eng.tree_hist(tb, B, 0)
        h4 = eng.tree_hist(tb, B, 4, nodes=nodes4)[:2]
        hB, hr, hc = host_path(X[0].cpu().numpy(), E.cpu().numpy(), host_tr[0], idx, whole, rows)
        assert np.array_equal(hB, B[0].cpu().numpy())
        if n == 1:
            assert np.array_equal(hr, r0.cpu().numpy()[:, 0]) and np.array_equal(hc, c0.cpu().numpy()[:, 0].astype(np.int64))
        kb, kk, kh0, kf0, kh4, kf4, kt, wt, host = [], [], [], [], [], [], [], [], []
        for _ in range(args.reps):
            kb.append(eng.feature_bins(X, E, out=B, timed=True)[1])
            kk.append(eng.tree_keys(B, tree, 5, timed=True)[1])
            ms = eng.tree_hist(tb, B, 0, hist=(r0, c0), timed=True)[3]
            kh0.append(ms[0]), kf0.append(ms[1])
            ms = eng.tree_hist(tb, B, 4, nodes=nodes4, hist=h4, timed=True)[3]
            kh4.append(ms[0]), kf4.append(ms[1])
            t0 = time.perf_counter()
            kt.append(eng.tree_train(tb, B, 5, timed=True)[1])
            wt.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            hX, hE = X.cpu().numpy(), E.cpu().numpy()
            for i, t in enumerate(tb):
                host_path(hX[i], hE, eng.cu_trace_array(t), idx, whole, rows)
            host.append((time.perf_counter() - t0) * 1e3)
        slot = 12 * 4096 + 8
        blocks = [rows[d][1] * n for d in range(4)]
        chunks = sum(min(8, -(-b // 1024)) for b in blocks)
        hist_bytes = lambda level: (n * NL * (-(-F // (64 >> level))) * 26 + n * NL * F) + chunks * (-(-F // (64 >> level))) * slot
        fold_bytes = lambda level: chunks * (-(-F // (64 >> level))) * slot + 4 * (1 << level) * F * 64 * 12
        rate = lambda b, ms: {"bytes": b, "Bps": b / (np.median(ms) * 1e-3), "share_of_hbm": b / (np.median(ms) * 1e-3) / HBM_SUSTAINED}
        res["batches"].append({"n_pics": n, "rows": n * NL, "hist_chunk_workgroups": chunks,
                               "feat_bins_ms": q(kb), "feat_bins": rate(n * NL * F * 5, kb),
                               "tree_keys_5_ms": q(kk), "tree_keys_5": rate(n * NL * 7, kk),
                               "tree_hist_0_ms": q(kh0), "tree_hist_0": rate(hist_bytes(0), kh0), "tree_fold_0_ms": q(kf0), "tree_fold_0": rate(fold_bytes(0), kf0),
                               "tree_hist_4_ms": q(kh4), "tree_hist_4": rate(hist_bytes(4), kh4), "tree_fold_4_ms": q(kf4), "tree_fold_4": rate(fold_bytes(4), kf4),
                               "tree_train_5_kernels_ms": q(kt), "tree_train_5_call_ms": q(wt),
                               "host_bins_and_level0_hist_ms": q(host)})
    eng.destroy()
    doc = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
