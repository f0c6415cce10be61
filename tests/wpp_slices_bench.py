#!/usr/bin/env python3
"""WaveFrontSynchro inside slices: timing -- a measurement script, not a test.  QP 32, synth.mixed, wall time from launch to
device synchronise, every leg repeated --reps times in the same run (all values kept, the median and the spread reported).
Prints one JSON line and, with --out, writes it to that file.

Legs (R = 2: slices of two whole CTU rows, the bench's slicing):
  slices     the slices as plain chains (fcu_compress_chains)                 critical path 2W CTU-times
  wpp        one slice per picture, rows as chains (fcu_wpp_begin)            W + 2(H - 1); P with a partial bottom row: 2W + 2(H - 2)
  sliced     slices of R rows, rows as chains (fcu_wpp_begin_slices)          W + 2(R - 1)
(a) one I picture at 1080p (30 x 17 CTUs: 60 / 62 / 32) and at 4K (60 x 34: 120 / 126 / 62): the three legs, and the ratios
    slices / sliced and wpp / sliced next to their ideals from those counts;
(b) 1 / 8 / 32 4K I pictures in flight: the three legs in CTUs/s (1 = the figures of (a));
(c) one P picture (TZ, SearchRange 64, one reference) at 1080p and 4K: wpp against sliced.  The reference picture is a padded
    source picture of the same moving clip (what it holds does not change the work)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

R = 2
SIZES = {"1080p": (1920, 1080), "4k": (3840, 2160)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inflight", default="8,32")
    ap.add_argument("--inflight-reps", type=int, default=2)
    ap.add_argument("--p-reps", type=int, default=2)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    import search_trace as st
    pkg = g.load_package()
    res = {"bench": "wpp_slices", "qp": 32, "slice_rows": R}

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t

    def log(msg):
        print(msg, file=sys.stderr, flush=True)

    def summary(ts):
        return {"s": ts, "median_s": statistics.median(ts), "spread": (max(ts) - min(ts)) / statistics.median(ts)}

    def i_legs(eng, srcs, W, rows, reps):
        """the three legs on len(srcs) I pictures in flight, interleaved rep by rep; wall times per leg"""
        N = len(srcs)
        n_sl = (rows + R - 1) // R
        ts = {"slices": [], "wpp": [], "sliced": []}
        for _ in range(reps):
            for i in range(N):                               # the slice chains of all pictures at consecutive indices
                eng.init_slice_chains(i * n_sl, srcs[i], 32, R * W)
            ts["slices"].append(wall(lambda: eng.compress_chains(0, N * n_sl, R * W)))
            for i in range(N):
                eng.init_wpp_picture(i * rows, srcs[i], 32)
            ts["wpp"].append(wall(lambda: eng.compress_wpp(0, N * rows)))
            for i in range(N):
                eng.init_wpp_picture(i * rows, srcs[i], 32, slice_rows=R)
            ts["sliced"].append(wall(lambda: eng.compress_wpp(0, N * rows)))
        return ts

    def ratios(legs, ideal):
        out = {k: summary(v) for k, v in legs.items()}
        for base in ("slices", "wpp"):
            m = out[base]["median_s"] / out["sliced"]["median_s"]
            out[f"{base}_over_sliced"] = {"measured": m, "ideal": ideal[base] / ideal["sliced"], "measured_over_ideal": m / (ideal[base] / ideal["sliced"])}
        return out

    parts = args.parts.split(",")
    ns = [int(v) for v in args.inflight.split(",")] if "b" in parts else []
    for name, (w, h) in SIZES.items():
        if "a" not in parts and not (name == "4k" and ns):
            continue
        W, rows = (w + 63) // 64, (h + 63) // 64
        ideal = {"slices": min(R, rows) * W, "wpp": W + 2 * (rows - 1), "sliced": W + 2 * (min(R, rows) - 1)}
        n_src = 4 if (name == "4k" and ns) else 1
        srcs = [[torch.from_numpy(p).cuda() for p in pkg.synth.mixed(w, h, seed=21 + i)] for i in range(n_src)]
        eng = pkg.CuEngine(w, h, max_chains=(max(ns) if (name == "4k" and ns) else 1) * rows)
        if "a" in parts:
            res[f"{name}_i"] = dict(critical_path_ctus=ideal, **ratios(i_legs(eng, srcs[:1], W, rows, args.reps), ideal))
            log(f"{name} I picture: {res[f'{name}_i']}")
        if name == "4k":
            curve = {}
            for N in ns:
                legs = i_legs(eng, [srcs[i % n_src] for i in range(N)], W, rows, args.inflight_reps)
                curve[str(N)] = {k: dict(summary(v), ctu_per_s=N * eng.n_ctu / statistics.median(v)) for k, v in legs.items()}
                log(f"4k in flight {N}: {curve[str(N)]}")
            if ns:
                res["4k_i_inflight"] = curve
        eng.destroy()

    if "c" in parts:
        for name, (w, h) in SIZES.items():
            W, rows = (w + 63) // 64, (h + 63) // 64
            full_bottom = h % 64 == 0
            ideal = {"wpp": W + 2 * (rows - 1) if full_bottom else 2 * W + 2 * (rows - 2), "sliced": W + 2 * (R - 1)}
            eng = pkg.CuEngine(w, h, max_chains=rows)
            frames = [[torch.from_numpy(p).cuda() for p in st.moving_frame(pkg.synth, "mixed", w, h, 7, poc)] for poc in (3, 4)]
            pad = eng.pad_reference(frames[0])
            fp = pkg.engine.ldp_slice(32, 4)
            fp.search_range, fp.fast_search = 64, 1
            kw = dict(refs=[pad], ref_pocs=[3], poc=4)
            ts = {"wpp": [], "sliced": []}
            for _ in range(args.p_reps):
                eng.init_wpp_picture(0, frames[1], fp.qp, params=fp, **kw)
                ts["wpp"].append(wall(lambda: eng.compress_wpp(0, rows)))
                eng.init_wpp_picture(0, frames[1], fp.qp, params=fp, slice_rows=R, **kw)
                ts["sliced"].append(wall(lambda: eng.compress_wpp(0, rows)))
            out = {k: summary(v) for k, v in ts.items()}
            m = out["wpp"]["median_s"] / out["sliced"]["median_s"]
            out["wpp_over_sliced"] = {"measured": m, "ideal": ideal["wpp"] / ideal["sliced"], "measured_over_ideal": m / (ideal["wpp"] / ideal["sliced"])}
            res[f"{name}_p"] = dict(critical_path_ctus=ideal, search_range=64, fast_search="TZ", n_ref=1, **out)
            log(f"{name} P picture: {res[f'{name}_p']}")
            eng.destroy()

    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
