#!/usr/bin/env python3
"""Loop filters with and without LFCrossSliceBoundaryFlag 0 on 4K pictures -- a measurement script, not a test.
The shapes are those of tests/lf_tiles_bench.py: `--pics` pictures per SAO call, `--frames` copies of one picture whose CU data
comes from `--rows` decided CTU rows.  Times fcu_sao / fcu_deblock and, where the library has them, the slice calls with
slice_ctus 120 (two CTU rows of the 60-CTU-wide picture) and 100 (a staircase) and LFCrossSliceBoundaryFlag 1 and 0.  With the
flag 1 fcu_deblock_slices launches fcu_deblock's kernels, and CuEngine.sao hands the batch to fcu_sao: those columns measure the
plain kernels through the slice arguments.  On a library without the slice entry points only the plain calls are timed, so that
the same script measures the commit before them.
Prints one JSON line per repetition (`--reps`): ms per picture of each variant (best of `--inner` runs); `--out FILE` also
writes the lines as one JSON document."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SLICES = (120, 100)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pics", type=int, default=8)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--rows", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    w, h, qp, sl = 3840, 2160, 32, 60
    lam = 0.57 * 2.0 ** ((qp - 12) / 3.0)
    dev = torch.device("cuda", 0)
    eng = pkg.CuEngine(w, h, max_chains=args.rows)
    has_slices = hasattr(eng.lib, "fcu_sao_slices") and hasattr(eng.lib, "fcu_deblock_slices")
    variants = [("plain", None, {})] + ([("slices%d_cross%d" % (s, c), s, dict(lf_cross_slices=c)) for s in SLICES for c in (1, 0)] if has_slices else [])
    # ---- SAO input (tests/sao_bench.py)
    pics = []
    for i in range(args.pics):
        org = [torch.from_numpy(p).to(dev) for p in pkg.synth.textured(w, h, seed=7 + i)]
        rec = []
        for p in org:
            f = p.float()[None, None]
            f = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(f, (1, 1, 1, 1), mode="replicate"), 3, 1)[0, 0]
            rec.append(((f / 6).round() * 6).clamp(0, 255).to(torch.uint8).contiguous())
        pics.append({"org": org, "rec": rec, "qp": qp, "lambda_": lam})
    # ---- deblocking input (tests/deblock_bench.py)
    Y, U, V = pkg.synth.textured(w, h, seed=7)
    rec, out = eng.init_chain(0, (Y, U, V), qp, slice_ctus=sl)
    planes = eng._keep[0][0]
    for k in range(args.rows):
        if k:
            eng.init_chain(k, planes, qp, slice_ctus=sl, rec=rec, out=out)
        eng.set_range(k, k * sl, sl)
    eng.compress_chains(0, args.rows, sl)
    eng.sync()
    o = out.view(eng.n_ctu, pkg.engine.CTU_OUT_BYTES)
    for r in range(args.rows, 34):
        src = (r % args.rows) * sl
        o[r * sl:(r + 1) * sl] = o[src:src + sl]
    for p, rows in ((rec[0], 64), (rec[1], 32), (rec[2], 32)):
        for r in range(args.rows, 34):
            src = (r % args.rows) * rows
            n = min(rows, p.shape[0] - r * rows)
            p[r * rows:r * rows + n] = p[src:src + n]
    frames = [[p.clone() for p in rec] for _ in range(args.frames)]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    lines = []
    for rep in range(args.reps):
        res = {"label": args.label, "rep": rep, "pictures": args.pics, "frames": args.frames, "slice_ctus": list(SLICES) if has_slices else None, "sao_ms_per_picture": {}, "sao_kernel_ms": {}, "deblock_ms_per_frame": {}}
        for name, s_ctus, kw in variants:
            best = None
            for _ in range(args.inner):
                work = [dict(p, rec=[r.clone() for r in p["rec"]], slice_ctus=s_ctus or 0) for p in pics]      # SAO is in place
                torch.cuda.synchronize()
                _, _, ms = eng.sao(work, timed=True, **kw)
                if best is None or sum(ms) < sum(best):
                    best = ms
            res["sao_ms_per_picture"][name] = sum(best) / args.pics
            res["sao_kernel_ms"][name] = [round(m, 4) for m in best]
            best = None
            for _ in range(args.inner):
                work = [[p.clone() for p in f] for f in frames]                       # deblocking is in place
                torch.cuda.synchronize()
                ev[0].record()
                for f in work:
                    eng.deblock(out=out, rec=f, stream=torch.cuda.current_stream(), **(dict(kw, slice_ctus=s_ctus) if s_ctus else {}))
                ev[1].record()
                torch.cuda.synchronize()
                ms = ev[0].elapsed_time(ev[1])
                best = ms if best is None else min(best, ms)
            res["deblock_ms_per_frame"][name] = best / args.frames
        print(json.dumps(res), flush=True)
        lines.append(res)
    eng.destroy()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
