#!/usr/bin/env python3
"""Time of the picture report (fcu_picture_report) on 4K pictures -- a measurement script, not a test.

For n_pics = 1 and 16 pictures of 3840x2160 in one call: the two kernels (report_ctu, report_pic) from the call's own events
(kernel_ms2), the whole call -- descriptor upload, both kernels, the records back, the host PSNR -- between two events on the
stream, and next to it the host path the call replaces, exactly as tools/fcu_decide.py and sequence.py do it: copy the three
reconstruction planes and the depth array to the host, PSNR and depth histogram in numpy.  That host path uses nothing this
entry point adds, so it is the same code on the commit before it.

Planes: the textured generator and a low-passed, re-quantised copy of it (a stand-in for a decided picture; the kernels' work
does not depend on where the distortion came from), further pictures rolled copies; records: heads with random values in 0..3.
Every shape is warmed up; a timed window repeats the call until it spans about a second; the median of the per-call times and
their spread are reported.  The SSD is checked against a sum formed with torch on the device before anything is timed.
Writes one JSON document (--out) and prints it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pics", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--window", type=float, default=1.0, help="seconds a timed window should span")
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    e = pkg.engine
    w, h = 3840, 2160
    dev = torch.device("cuda", 0)
    eng = pkg.CuEngine(w, h, max_chains=1)
    n_ctu, nb = eng.n_ctu, e.CTU_OUT_BYTES
    host_org = pkg.synth.textured(w, h, seed=7)
    org0 = [torch.from_numpy(p).to(dev) for p in host_org]
    rec0 = []
    for p in org0:
        f = p.float()[None, None]
        f = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(f, (1, 1, 1, 1), mode="replicate"), 3, 1)[0, 0]
        rec0.append(((f / 6).round() * 6).clamp(0, 255).to(torch.uint8).contiguous())
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    pics = []
    for i in range(max(args.pics)):
        out = torch.zeros((n_ctu, nb), dtype=torch.uint8, device=dev)
        out[:, :32 * 256] = torch.randint(0, 4, (n_ctu, 32 * 256), dtype=torch.uint8, device=dev, generator=gen)
        pics.append({"org": [torch.roll(p, (i, 2 * i), (0, 1)).contiguous() for p in org0],
                     "rec": [torch.roll(p, (i, 2 * i), (0, 1)).contiguous() for p in rec0], "out": out.view(-1)})
    head_bytes = 8 * 256 + 12                                # the eight per-partition arrays and the three totals the kernel reads
    plane_bytes = w * h * 3 // 2
    res = {"width": w, "height": h, "device": torch.cuda.get_device_name(0),
           "bytes_per_picture": {"planes_org_and_rec": 2 * plane_bytes, "record_heads_read": n_ctu * head_bytes, "ctu_records_written": n_ctu * 64},
           "runs": []}
    for n in args.pics:
        batch = pics[:n]
        got = eng.report(batch)
        for p, r in zip(batch, got):                         # results first: the SSD against a device-side sum
            want = [int(((o.long() - q.long()) ** 2).sum().item()) for o, q in zip(p["org"], p["rec"])]
            assert [int(v) for v in r["ssd"]] == want, (r["ssd"], want)
            assert int(r["n_part"]) == (w // 4) * (h // 4) == sum(int(v) for v in r["depth_part"])      # every depth is 0..3 here
        for _ in range(10):                                   # warm-up of this shape
            eng.report(batch, timed=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            eng.report(batch)
        per_call = (time.perf_counter() - t0) / 20
        reps = int(min(5000, max(50, args.window / per_call)))
        k_ctu, k_pic, call = [], [], []
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for _ in range(reps):
            ev[0].record()
            _, ms = eng.report(batch, timed=True)
            ev[1].record()
            ev[1].synchronize()
            k_ctu.append(ms[0]); k_pic.append(ms[1]); call.append(ev[0].elapsed_time(ev[1]))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):                                 # the call as a caller sees it (no kernel events), host clock around a call that ends synchronised
            eng.report(batch)
        wall = (time.perf_counter() - t0) / reps * 1e3
        # the host path this replaces, per picture as the tool does it
        host = []
        for _ in range(args.host_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for p in batch:
                psnr = []
                for q, o in zip(p["rec"], host_org):
                    d = q.cpu().numpy().astype(np.int64) - o.astype(np.int64)
                    ssd = float((d * d).sum())
                    psnr.append(999.99 if ssd == 0 else 10.0 * np.log10(255.0 * 255.0 * d.size / ssd))
                depth = p["out"].view(n_ctu, nb)[:, :256].cpu().numpy().copy()
                np.bincount(depth.ravel(), minlength=4)
            host.append((time.perf_counter() - t0) * 1e3)
        q = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "p90": float(np.percentile(v, 90))}
        read = n * (2 * plane_bytes + n_ctu * head_bytes)
        res["runs"].append({"n_pics": n, "reps": reps, "report_ctu_ms": q(k_ctu), "report_pic_ms": q(k_pic), "call_events_ms": q(call),
                            "call_host_clock_ms": wall, "host_path_ms": q(host), "host_path_reps": args.host_reps,
                            "report_ctu_bytes_read": read, "report_ctu_GBps": read / (float(np.median(k_ctu)) * 1e-3) / 1e9,
                            "device_call_per_picture_ms": wall / n, "host_path_per_picture_ms": float(np.median(host)) / n,
                            "psnr_first_picture": [float(v) for v in got[0]["psnr"]]})
    eng.destroy()
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
