#!/usr/bin/env python3
"""WaveFrontSynchro timing -- a measurement script, not a test.  Prints one JSON line:
  (a) 1080p QP 32, one picture, one slice: wall time (launch to device synchronise) with WPP (fcu_compress_wpp) and without
      (one chain through fcu_compress_chains); ideal ratio = 510 CTUs / critical path W + 2(H-1) = 62 CTU-times = 8.2;
  (b) 4K (3840x2160) one picture with WPP: wall time;
  (c) 4K all-intra, N pictures in flight with WPP (N = --inflight): CTU/s, next to the slice_mode_0 figure of the same run --
      N one-slice pictures without WPP as N chains, timed over their first --sm0-ctus CTUs (a whole 4K picture as one chain takes
      minutes; a chain's CTU rate does not change along the picture beyond the content)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inflight", default="1,8,32,120")
    ap.add_argument("--sm0-ctus", type=int, default=8)
    ap.add_argument("--skip-serial-1080p", action="store_true", help="leave out the ~90 s one-chain 1080p picture")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    res = {"bench": "wpp", "qp": 32}

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t

    # (a) 1080p
    w, h = 1920, 1080
    src = pkg.synth.mixed(w, h, seed=21)
    rows = (h + 63) // 64
    eng = pkg.CuEngine(w, h, max_chains=rows)
    n, _, _ = eng.init_wpp_picture(0, src, 32)
    res["1080p_wpp_s"] = wall(lambda: eng.compress_wpp(0, n))
    if not args.skip_serial_1080p:
        eng.init_chain(0, src, 32)
        res["1080p_one_chain_s"] = wall(lambda: eng.compress_chains(0, 1, eng.n_ctu))
        res["1080p_speedup"] = res["1080p_one_chain_s"] / res["1080p_wpp_s"]
    else:
        res["1080p_one_chain_s"] = "not measured"
    res["1080p_ideal_speedup"] = eng.n_ctu / ((w + 63) // 64 + 2 * (rows - 1))
    eng.destroy()

    # (b), (c) 4K
    w, h = 3840, 2160
    rows = (h + 63) // 64
    ns = [int(v) for v in args.inflight.split(",")]
    eng = pkg.CuEngine(w, h, max_chains=max(ns) * rows)
    srcs = [[torch.from_numpy(p).cuda() for p in pkg.synth.mixed(w, h, seed=30 + i)] for i in range(max(ns))]
    curve = {}
    for N in ns:
        for i in range(N):
            eng.init_wpp_picture(i * rows, srcs[i], 32)
        t = wall(lambda: eng.compress_wpp(0, N * rows))
        curve[str(N)] = {"wall_s": t, "ctu_per_s": N * eng.n_ctu / t}
        if N == 1:
            res["4k_wpp_one_picture_s"] = t
        # slice_mode_0 of the same N: N one-slice pictures without WPP, first sm0_ctus CTUs of each
        for i in range(N):
            eng.init_chain(i, srcs[i], 32)
        t0 = wall(lambda: eng.compress_chains(0, N, args.sm0_ctus))
        curve[str(N)]["slice_mode_0_ctu_per_s"] = N * args.sm0_ctus / t0
    res["4k_inflight"] = curve
    eng.destroy()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
