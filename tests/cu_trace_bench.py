#!/usr/bin/env python3
"""Time of the CU trace and of what is made of it (fcu_label_score, fcu_trace_maps) on 4K pictures -- a measurement script, not a
test.  Writes one JSON document (--out) and prints it.

  engine     34 slice chains of one CTU row of a 3840x2160 I picture each, the first --ctus CTUs of every row, decided with no
             trace bound and with one: the cost of binding a trace, as a ratio on the same work (medians of --reps launches after a
             warm-up launch, min and max next to them).  bench.py, which binds no trace, is the figure for the engine as it ships.
  score      fcu_label_score of 1 and 16 pictures: both kernels from the call's own events and the call on the host clock.  The
             path it replaces is a Verifying decision of the picture: its time is ESTIMATED from the rows above (60 CTUs at the
             measured time per CTU of a row chain, all rows side by side) -- an estimate, not a measurement of a whole picture.
  maps       fcu_trace_maps (labels + J0 + J1) of 1 and 16 pictures against the path it replaces: the trace copied to the host and
             the three arrays formed in numpy (array operations, no loops).
Traces of the kernel runs are synthetic (random records, every CU valid); one result of every shape is checked against the host
path before anything is timed.  Per kernel the ALGORITHMIC bytes (from the shapes) over the kernel time and their share of the
HBM rate an MI355X sustains (6.3 TB/s)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_SUSTAINED = 6.3e12


def node_elements(w, h):
    """[n_ctu, 85] element of the label layout of every node (-1: the block starts outside the picture) and [n_ctu, 85] whole"""
    w_ctu, h_ctu = (w + 63) // 64, (h + 63) // 64
    idx, whole, off = np.full((w_ctu * h_ctu, 85), -1, np.int64), np.zeros((w_ctu * h_ctu, 85), bool), 0
    cx, cy = np.meshgrid(np.arange(w_ctu), np.arange(h_ctu))
    cx, cy = cx.reshape(-1), cy.reshape(-1)
    for d in range(4):
        s, bw, bh = 64 >> d, (w + (64 >> d) - 1) // (64 >> d), (h + (64 >> d) - 1) // (64 >> d)
        for j in range(4 ** d):
            nx = sum(((j >> (2 * b)) & 1) << b for b in range(d))
            ny = sum(((j >> (2 * b + 1)) & 1) << b for b in range(d))
            x, y = cx * 64 + nx * s, cy * 64 + ny * s
            t = (0, 1, 5, 21)[d] + j
            inside = (x < w) & (y < h)
            idx[:, t] = np.where(inside, off + (y // s) * bw + x // s, -1)
            whole[:, t] = (x + s <= w) & (y + s <= h)
        off += bw * bh
    return idx, whole, off


def host_maps(tr, idx, whole, NL):
    """the path fcu_trace_maps replaces, on a host copy of one picture's trace"""
    lab, j0, j1 = np.zeros(NL, np.int8), np.zeros(NL, np.float64), np.zeros(NL, np.float64)
    m = idx >= 0
    kept = whole & (tr["valid"] != 0) & (tr["split_tried"] != 0)
    depth_lt3 = np.arange(85)[None, :] < 21
    v = np.where(~whole & depth_lt3, 2, np.where(kept, tr["split_won"].astype(np.int8), -1)).astype(np.int8)
    lab[idx[m]] = v[m]
    j0[idx[m]] = np.where(kept, tr["j0"], 0.0)[m]
    j1[idx[m]] = np.where(kept, tr["j1"], 0.0)[m]
    return lab, j0, j1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pics", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ctus", type=int, default=3, help="CTUs of every row chain the engine legs decide")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    e = pkg.engine
    w, h, qp = 3840, 2160, 32
    dev = torch.device("cuda", 0)
    q = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}
    res = {"width": w, "height": h, "device": torch.cuda.get_device_name(0), "hbm_sustained_Bps": HBM_SUSTAINED, "engine": {}, "score": [], "maps": []}

    # ---- the engine with and without a trace
    lo = pkg.layout.PictureLayout(w, h, slice_ctus=60)
    eng = pkg.CuEngine(w, h, max_chains=lo.chains)
    n_ctu, NL = eng.n_ctu, eng.label_count()
    frame = pkg.synth.mixed(w, h, seed=3)
    labels = torch.ones(NL, dtype=torch.int8, device=dev)

    def launch(trace, state):
        n, _, _ = eng.init_picture(0, frame, qp, lo)
        if trace is not None:
            for k in range(n):
                eng.enable_cu_trace(k, trace)
        if state != e.TRAINING:
            eng.set_labels(range(n), labels)
            for k in range(n):
                eng.set_decision(k, state)
        eng.sync()
        t0 = time.perf_counter()
        eng.compress_chains(0, n, args.ctus)
        eng.sync()
        return (time.perf_counter() - t0) * 1e3
    trace = torch.zeros(n_ctu * e.CUS_PER_CTU * e.CU_TRACE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    legs = {"training_no_trace": (None, e.TRAINING), "training_trace": (trace, e.TRAINING), "verifying_no_trace": (None, e.VERIFYING)}
    times = {k: [] for k in legs}
    for rep in range(args.reps + 1):                          # the legs alternate; the first round is the warm-up
        for k, (t, s) in legs.items():
            ms = launch(t, s)
            if rep:
                times[k].append(ms)
    res["engine"] = {"chains": lo.chains, "ctus_per_chain": args.ctus, **{k + "_ms": q(v) for k, v in times.items()}}
    res["engine"]["trace_over_no_trace"] = res["engine"]["training_trace_ms"]["median"] / res["engine"]["training_no_trace_ms"]["median"]
    per_ctu = res["engine"]["verifying_no_trace_ms"]["median"] / args.ctus
    res["engine"]["verifying_picture_ms_ESTIMATE"] = per_ctu * 60
    res["engine"]["estimate_note"] = "60 CTUs of a row at the measured time per CTU of a row chain, 34 rows side by side; not a measured picture"

    # ---- the kernels on synthetic traces
    rng = np.random.default_rng(7)
    idx, whole, nl = node_elements(w, h)
    assert nl == NL
    n_max = max(args.pics)
    host_tr = np.zeros((n_max, n_ctu, 85), e.CU_TRACE_DTYPE)
    host_tr["j0"], host_tr["j1"] = rng.integers(1, 1 << 20, host_tr.shape).astype(np.float64), rng.integers(1, 1 << 20, host_tr.shape).astype(np.float64)
    host_tr["valid"], host_tr["split_tried"], host_tr["whole_tried"] = whole[None], whole[None], whole[None]
    host_tr["split_won"] = rng.integers(0, 2, host_tr.shape) * whole[None]
    traces = [torch.as_tensor(host_tr[i].view(np.uint8).reshape(-1)).to(dev) for i in range(n_max)]
    labs = torch.as_tensor(rng.integers(0, 2, (n_max, NL)).astype(np.int8)).to(dev)
    for n in args.pics:
        tb, lb = traces[:n], labs[:n]
        rec = eng.label_score(tb, lb)                          # warm-up + check of the counts against numpy
        v = labs[0].cpu().numpy()[np.where(idx >= 0, idx, 0)]
        for d, (a, b) in enumerate(((0, 1), (1, 5), (5, 21), (21, 85))):
            sel = whole[:, a:b]
            assert rec["v"][0][d, 0] == ((v[:, a:b] == 1) & (host_tr[0]["split_won"][:, a:b] == 1) & sel).sum()
        k1, k2, call = [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            _, ms = eng.label_score(tb, lb, timed=True)
            call.append((time.perf_counter() - t0) * 1e3), k1.append(ms[0]), k2.append(ms[1])
        nbytes = n * n_ctu * (85 * 24 + 85 + 128)
        res["score"].append({"n_pics": n, "score_ctu_ms": q(k1), "score_pic_ms": q(k2), "call_ms": q(call), "score_ctu_bytes": nbytes, "score_pic_bytes": n * n_ctu * 128,
                             "score_ctu_Bps": nbytes / (np.median(k1) * 1e-3), "score_ctu_share_of_hbm": nbytes / (np.median(k1) * 1e-3) / HBM_SUSTAINED,
                             "replaces_verifying_decision_ms_ESTIMATE": n * res["engine"]["verifying_picture_ms_ESTIMATE"]})
        m = eng.trace_maps(tb, labels=True, costs=True)        # warm-up + check
        want = host_maps(host_tr[0], idx, whole, NL)
        for got, wnt in zip((m["labels"][0], m["j0"][0], m["j1"][0]), want):
            assert np.array_equal(got.cpu().numpy(), wnt)
        km, call, host = [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            _, ms = eng.trace_maps(tb, labels=True, costs=True, timed=True)
            call.append((time.perf_counter() - t0) * 1e3), km.append(ms)
            t0 = time.perf_counter()
            for t in tb:
                host_maps(eng.cu_trace_array(t), idx, whole, NL)
            host.append((time.perf_counter() - t0) * 1e3)
        nbytes = n * (n_ctu * 85 * 24 + NL * 17)
        res["maps"].append({"n_pics": n, "trace_ctu_ms": q(km), "call_ms": q(call), "host_path_ms": q(host), "bytes": nbytes, "Bps": nbytes / (np.median(km) * 1e-3),
                            "share_of_hbm": nbytes / (np.median(km) * 1e-3) / HBM_SUSTAINED})
    eng.destroy()
    doc = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
