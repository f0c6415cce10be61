#!/usr/bin/env python3
"""Time of the risk-table model (fcu_risk_train, fcu_risk_predict, fcu_nobf_maps) on 4K pictures -- a measurement script, not a test.
Writes one JSON document (--out) and prints it.

  train     risk_train + risk_add of 1 and 16 pictures from the call's own events, and the call on the host clock; next to it, in
            the same session and on the same batch, fcu_trace_maps (labels + J0 + J1), which reads the same records.
  predict   risk_predict of the same batch; nobf: fcu_nobf_maps (no event of its own: the call on the host clock and a pair of
            stream events around it, both including the copy of the pointer array).
  host      the path the train call replaces: traces and keys copied to the host, the samples selected and the tables formed with
            numpy (array operations, integer np.add.at, no loops).
Traces are synthetic (random records, every whole CU a sample; keys = the N_OBF maps of random OBF maps); one result of every
shape is checked against the host path before anything is timed.  Medians of --reps repetitions after a warm-up, min and max
next to them.  Per kernel the ALGORITHMIC bytes (from the shapes) over the kernel time and their share of the HBM rate an MI355X
sustains (6.3 TB/s)."""
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


def host_train(tr, keys, idx, whole):
    """the tables of one picture's host copies: (risk int64 [4 * 257 * 2], count int64 [...], dropped)"""
    depth = np.repeat(np.arange(4), (1, 4, 16, 64))[None, :]
    smp = whole & (tr["valid"] != 0) & (tr["split_tried"] != 0) & (tr["whole_tried"] != 0)
    key = keys[np.where(idx >= 0, idx, 0)].astype(np.int64)
    keep = smp & (key < 257)
    s = np.abs(tr["j0"] - tr["j1"]) * 256.0
    q = np.where(s < 2.0 ** 40, np.floor(np.where(s < 2.0 ** 40, s, 0.0)), 2.0 ** 40 - 1).astype(np.int64)
    cell = ((depth * 257 + key) * 2 + (tr["split_won"] != 0))[keep]
    risk, count = np.zeros(4 * 257 * 2, np.int64), np.zeros(4 * 257 * 2, np.int64)
    np.add.at(risk, cell, q[keep])
    np.add.at(count, cell, 1)
    return risk, count, int((smp & ~keep).sum())


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
    w, h = 3840, 2160
    dev = torch.device("cuda", 0)
    q = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}
    res = {"width": w, "height": h, "device": torch.cuda.get_device_name(0), "hbm_sustained_Bps": HBM_SUSTAINED, "reps": args.reps, "batches": []}
    eng = pkg.CuEngine(w, h, max_chains=1)
    n_ctu, NL = eng.n_ctu, eng.label_count()
    rng = np.random.default_rng(7)
    idx, whole, nl = node_elements(w, h)
    assert nl == NL
    n_max = max(args.pics)
    host_tr = np.zeros((n_max, n_ctu, 85), e.CU_TRACE_DTYPE)
    host_tr["j0"], host_tr["j1"] = rng.random(host_tr.shape) * 1e5, rng.random(host_tr.shape) * 1e5
    host_tr["valid"], host_tr["split_tried"], host_tr["whole_tried"] = whole[None], whole[None], whole[None]
    host_tr["split_won"] = rng.integers(0, 2, host_tr.shape) * whole[None]
    traces = [torch.as_tensor(host_tr[i].view(np.uint8).reshape(-1)).to(dev) for i in range(n_max)]
    obf = torch.as_tensor(np.where(rng.random((n_max, h // 4, w // 4)) < 0.5, 0, rng.integers(1, 40, (n_max, h // 4, w // 4))).astype(np.int16)).to(dev)
    for n in args.pics:
        tb = traces[:n]
        keys = eng.nobf_maps(obf[:n])                          # warm-up of every call + the checks against the host path
        model, dropped = eng.risk_train(tb, keys)
        hk = keys.cpu().numpy()
        want = [host_train(host_tr[i], hk[i], idx, whole) for i in range(n)]
        hm = model.cpu().numpy().view(e.RISK_MODEL_DTYPE)[0]
        assert np.array_equal(hm["risk"].reshape(-1), sum(x[0] for x in want)) and np.array_equal(hm["count"].reshape(-1).astype(np.int64), sum(x[1] for x in want))
        assert dropped == sum(x[2] for x in want) == 0
        lab = eng.risk_predict(keys, model, min_count=1)
        tab = e.risk_table(model.cpu().numpy(), 1)
        d3 = NL - ((h + 7) // 8) * ((w + 7) // 8)
        assert np.array_equal(lab[0, d3:].cpu().numpy(), tab[3][hk[0, d3:]])      # (no 8x8 block is cut)
        eng.trace_maps(tb, labels=True, costs=True)
        k1, k2, call, kp, callp, km, nb_call, nb_ev, host = [], [], [], [], [], [], [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            _, _, ms = eng.risk_train(tb, keys, model=model, timed=True)
            call.append((time.perf_counter() - t0) * 1e3), k1.append(ms[0]), k2.append(ms[1])
            t0 = time.perf_counter()
            _, ms = eng.risk_predict(keys, model, min_count=1, timed=True)
            callp.append((time.perf_counter() - t0) * 1e3), kp.append(ms)
            _, ms = eng.trace_maps(tb, labels=True, costs=True, timed=True)
            km.append(ms)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            eng.nobf_maps(obf[:n])
            e1.record()
            torch.cuda.synchronize()
            nb_call.append((time.perf_counter() - t0) * 1e3), nb_ev.append(e0.elapsed_time(e1))
            t0 = time.perf_counter()
            hk2 = keys.cpu().numpy()
            for i, t in enumerate(tb):
                host_train(eng.cu_trace_array(t), hk2[i], idx, whole)
            host.append((time.perf_counter() - t0) * 1e3)
        groups = min(128, max(1, -(-n * n_ctu // 16)))
        b_train = n * n_ctu * 85 * (24 + 2) + groups * 24680
        b_add, b_pred, b_nobf, b_maps = groups * 24680 + 24672, n * NL * 3, n * (4 * (h // 4) * (w // 4) * 2 + NL * 2), n * (n_ctu * 85 * 24 + NL * 17)
        rate = lambda b, ms: {"bytes": b, "Bps": b / (np.median(ms) * 1e-3), "share_of_hbm": b / (np.median(ms) * 1e-3) / HBM_SUSTAINED}
        res["batches"].append({"n_pics": n, "train_workgroups": groups,
                               "risk_train_ms": q(k1), "risk_train": rate(b_train, k1), "risk_add_ms": q(k2), "risk_add": rate(b_add, k2), "train_call_ms": q(call),
                               "risk_predict_ms": q(kp), "risk_predict": rate(b_pred, kp), "predict_call_ms": q(callp),
                               "nobf_maps_events_ms": q(nb_ev), "nobf_maps": rate(b_nobf, nb_ev), "nobf_maps_call_ms": q(nb_call),
                               "trace_maps_ms": q(km), "trace_maps": rate(b_maps, km), "host_train_path_ms": q(host)})
    eng.destroy()
    doc = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
