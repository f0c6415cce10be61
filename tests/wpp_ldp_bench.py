#!/usr/bin/env python3
"""WaveFrontSynchro timing for lowdelay_P -- a measurement script, not a test.  QP 32 (a P picture of HM's lowdelay_P GOP
table), TZ search, SearchRange 64, with one reference picture and with the cfg's four.  Prints one JSON line and, with --out,
writes it to that file:
  (a) one P picture at 1080p and at 4K: wall time (launch to device synchronise) with WPP (fcu_wpp_begin_p + fcu_compress_wpp)
      and without (one chain through fcu_compress_chains, timed over its first --serial-ctus CTUs and scaled to the picture:
      a whole picture as one chain takes minutes; a chain's CTU rate does not change along the picture beyond the content);
      critical paths in CTU-times: W x H without WPP; with WPP, W + 2(H-1) when every row starts on a full CTU, and
      W + 2(H-2) + W when the partial bottom row waits for the whole row above (the price of the exact search-state hand-off);
  (b) clips in flight 1 / 8 / 32 at 1080p: CTUs/s with WPP (all rows of all clips in one launch) and without (one chain per
      clip, first --serial-ctus CTUs).
The reference pictures are padded source pictures of the same moving clip (what they hold does not change the work)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inflight", default="1,8,32")
    ap.add_argument("--refs", default="1,4")
    ap.add_argument("--serial-ctus", type=int, default=16)
    ap.add_argument("--sizes", default="1080p,4k")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    import search_trace as st
    pkg = g.load_package()
    res = {"bench": "wpp_ldp", "base_qp": 32, "search_range": 64, "fast_search": "TZ"}

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t

    def log(msg):
        print(msg, file=sys.stderr, flush=True)

    def setup(w, h, n_max):
        rows = (h + 63) // 64
        eng = pkg.CuEngine(w, h, max_chains=n_max * rows)
        frames = [[torch.from_numpy(p).cuda() for p in st.moving_frame(pkg.synth, "mixed", w, h, 7, poc)] for poc in range(5)]
        pads = [eng.pad_reference(f) for f in frames[:4]]
        fp = pkg.engine.ldp_slice(32, 4)
        fp.search_range, fp.fast_search = 64, 1
        return eng, rows, frames[4], pads, fp

    def refkw(pads, nref):
        return dict(refs=[pads[3 - k] for k in range(nref)], ref_pocs=[3 - k for k in range(nref)], poc=4)

    sizes = {"1080p": (1920, 1080), "4k": (3840, 2160)}
    for name in args.sizes.split(","):
        w, h = sizes[name]
        eng, rows, cur, pads, fp = setup(w, h, 1)
        W = (w + 63) // 64
        full_bottom = h % 64 == 0
        res[f"{name}_critical_path_ctus"] = {"one_chain": W * rows, "wpp": W + 2 * (rows - 1) if full_bottom else W + 2 * (rows - 2) + W}
        for nref in [int(v) for v in args.refs.split(",")]:
            kw = refkw(pads, nref)
            eng.init_wpp_picture(0, cur, fp.qp, params=fp, **kw)
            t_wpp = wall(lambda: eng.compress_wpp(0, rows))
            eng.init_chain(0, cur, fp.qp, params=fp, **kw)
            t_ser = wall(lambda: eng.compress_chains(0, 1, args.serial_ctus))
            est = t_ser / args.serial_ctus * eng.n_ctu
            res[f"{name}_{nref}ref"] = {"wpp_s": t_wpp, "one_chain_first_ctus": args.serial_ctus, "one_chain_first_ctus_s": t_ser,
                                        "one_chain_picture_s_estimated": est, "speedup_estimated": est / t_wpp}
            log(f"{name} {nref} ref: {res[f'{name}_{nref}ref']}")
        eng.destroy()

    ns = [int(v) for v in args.inflight.split(",")]
    w, h = sizes["1080p"]
    eng, rows, cur, pads, fp = setup(w, h, max(ns))
    for nref in [int(v) for v in args.refs.split(",")]:
        kw = refkw(pads, nref)
        curve = {}
        for N in ns:
            for i in range(N):
                eng.init_wpp_picture(i * rows, cur, fp.qp, params=fp, **kw)
            t = wall(lambda: eng.compress_wpp(0, N * rows))
            for i in range(N):
                eng.init_chain(i, cur, fp.qp, params=fp, **kw)
            t0 = wall(lambda: eng.compress_chains(0, N, args.serial_ctus))
            curve[str(N)] = {"wpp_wall_s": t, "wpp_ctu_per_s": N * eng.n_ctu / t, "no_wpp_ctu_per_s": N * args.serial_ctus / t0}
            log(f"1080p in flight {N}, {nref} ref: {curve[str(N)]}")
        res[f"1080p_inflight_{nref}ref"] = curve
    eng.destroy()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
