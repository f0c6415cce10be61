#!/usr/bin/env python3
"""Tiles: timing -- a measurement script, not a test.  QP 32, synth.mixed, wall time from launch to device synchronise, every
leg repeated --reps times in the same run, interleaved rep by rep (all values kept, the median and the spread reported).
Prints one JSON line and, with --out, writes it to that file (parts run separately are merged into an existing file).

Legs, with uniform 4 x 2 tiles:
  wpp        one slice per picture, rows as chains (fcu_wpp_begin)                        critical path W + 2(H - 1) CTU-times
  tiles      one chain per tile (fcu_tiles_begin)                                          the largest tile: tw x th
  wpp_tiles  WaveFrontSynchro inside every tile (fcu_wpp_begin_tiles)                      tw + 2(th - 1)
(a) one I picture at 1080p (30 x 17 CTUs: 62 / 72 / 24) and at 4K (60 x 34: 126 / 255 / 47): the three legs and the ratios
    wpp / wpp_tiles and wpp / tiles next to their arithmetic ideals;
(b) 1 / 8 / 32 4K I pictures in flight for each binding, in CTUs/s;
(c) one 4K P picture (TZ, SearchRange 64, one reference, TMVP off): wpp against wpp_tiles.  The reference picture is a padded
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

TILES = (4, 2)
SIZES = {"1080p": (1920, 1080), "4k": (3840, 2160)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inflight", default="8,32")
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--sizes", default="1080p,4k")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    import search_trace as st
    pkg = g.load_package()
    res = {"bench": "tiles", "qp": 32, "tiles": list(TILES), "reps": args.reps}

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

    def ideals(W, H):
        cb, rb = pkg.engine.tile_grid(W, H, *TILES)
        tw, th = max(b - a for a, b in zip(cb, cb[1:])), max(b - a for a, b in zip(rb, rb[1:]))
        return {"wpp": W + 2 * (H - 1), "tiles": tw * th, "wpp_tiles": tw + 2 * (th - 1)}

    def legs(eng, srcs, rows, reps, params=None, names=("wpp", "tiles", "wpp_tiles"), **kw):
        N = len(srcs)
        n_t, n_wt = eng.tile_chains(*TILES, False), eng.tile_chains(*TILES, True)
        qp = 32 if params is None else params.qp
        ts = {k: [] for k in names}
        for _ in range(reps):
            for k in names:
                if k == "wpp":
                    for i in range(N):
                        eng.init_wpp_picture(i * rows, srcs[i], qp, params=params, **kw)
                    ts[k].append(wall(lambda: eng.compress_wpp(0, N * rows)))
                elif k == "tiles":
                    for i in range(N):
                        eng.init_tile_picture(i * n_t, srcs[i], qp, *TILES, params=params, **kw)
                    ts[k].append(wall(lambda: eng.compress_chains(0, N * n_t, eng.n_ctu)))
                else:
                    for i in range(N):
                        eng.init_tile_picture(i * n_wt, srcs[i], qp, *TILES, wpp=True, params=params, **kw)
                    ts[k].append(wall(lambda: eng.compress_wpp(0, N * n_wt)))
                log(f"  {k}: {ts[k][-1]:.3f} s")
        return ts

    def with_ratios(ts, ideal):
        out = {k: summary(v) for k, v in ts.items()}
        for k in ts:
            if k != "wpp":
                m, want = out["wpp"]["median_s"] / out[k]["median_s"], ideal["wpp"] / ideal[k]
                out[f"wpp_over_{k}"] = {"measured": m, "ideal": want, "measured_over_ideal": m / want,
                                        "faster_by_more_than_the_spread": out[k]["median_s"] * (1 + max(out[k]["spread"], out["wpp"]["spread"])) < out["wpp"]["median_s"]}
        return out

    parts, sizes = args.parts.split(","), args.sizes.split(",")
    ns = [int(v) for v in args.inflight.split(",")] if "b" in parts else []
    for name in sizes:
        w, h = SIZES[name]
        W, rows = (w + 63) // 64, (h + 63) // 64
        ideal = ideals(W, rows)
        many = name == "4k" and ns
        per_pic = max(rows * TILES[0], TILES[0] * TILES[1], rows)
        if "a" in parts or many:
            srcs = [[torch.from_numpy(p).cuda() for p in pkg.synth.mixed(w, h, seed=21 + i)] for i in range(4 if many else 1)]
            eng = pkg.CuEngine(w, h, max_chains=(max(ns) if many else 1) * per_pic)
            if "a" in parts:
                log(f"{name} I picture")
                res[f"{name}_i"] = dict(critical_path_ctus=ideal, **with_ratios(legs(eng, srcs[:1], rows, args.reps), ideal))
            if many:
                curve = {}
                for N in ns:
                    log(f"4k, {N} in flight")
                    ts = legs(eng, [srcs[i % 4] for i in range(N)], rows, args.reps)
                    curve[str(N)] = {k: dict(summary(v), ctu_per_s=N * eng.n_ctu / statistics.median(v)) for k, v in ts.items()}
                res["4k_i_inflight"] = curve
            eng.destroy()
        if "c" in parts and name == "4k":
            eng = pkg.CuEngine(w, h, max_chains=per_pic)
            frames = [[torch.from_numpy(p).cuda() for p in st.moving_frame(pkg.synth, "mixed", w, h, 7, poc)] for poc in (3, 4)]
            pad = eng.pad_reference(frames[0])
            fp = pkg.engine.ldp_slice(32, 4)
            fp.search_range, fp.fast_search, fp.tmvp = 64, 1, 0
            log("4k P picture")
            ts = legs(eng, [frames[1]], rows, args.reps, params=fp, names=("wpp", "wpp_tiles"), refs=[pad], ref_pocs=[3], poc=4)
            res["4k_p"] = dict(critical_path_ctus={k: ideal[k] for k in ts}, search_range=64, fast_search="TZ", n_ref=1, tmvp=0, **with_ratios(ts, ideal))
            eng.destroy()

    if args.out and os.path.exists(args.out):                # parts run one after the other end up in one file
        old = json.loads(open(args.out).read())
        old.update(res)
        res = old
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
