#!/usr/bin/env python3
"""Time of the picture hash (fcu_picture_hash) on 4K pictures -- a measurement script, not a test.

For n_pics = 1 and 16 pictures of 3840x2160 in one call and each kind alone (MD5, CRC, checksum): the three kernels (hash_chunk,
hash_fold, hash_md5) from the call's own events (kernel_ms3; 0 for one that is not launched), the whole call -- pointer upload,
kernels, the records back -- between two events on the stream, and next to it the host path the call replaces: a copy of the
three planes to the host and hashlib.md5 for MD5, the copy and the numpy checksum for the checksum.  The CRC has no sensible
host implementation in Python, so its floor is the copy alone.  The host path uses nothing this entry point adds, so it is the
same code on the commit before it.

Planes: the textured generator, further pictures rolled copies.  The digests are checked against tests/hash_ref.py before
anything is timed.  Every shape is warmed up; a timed window repeats the call until it spans about a second (at least five
calls); the median of the per-call times and their spread are reported.  Writes one JSON document (--out) and prints it."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pics", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--kinds", nargs="+", default=["md5", "crc", "checksum"])
    ap.add_argument("--window", type=float, default=1.0, help="seconds a timed window should span")
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    import hash_ref
    pkg = g.load_package()
    w, h = 3840, 2160
    dev = torch.device("cuda", 0)
    eng = pkg.CuEngine(w, h, max_chains=1)
    host0 = pkg.synth.textured(w, h, seed=7)
    rec0 = [torch.from_numpy(p).to(dev) for p in host0]
    pics = [[torch.roll(p, (i, 2 * i), (0, 1)).contiguous() for p in rec0] for i in range(max(args.pics))]
    plane_bytes = w * h * 3 // 2
    res = {"width": w, "height": h, "device": torch.cuda.get_device_name(0), "plane_bytes_per_picture": plane_bytes, "runs": []}
    want = {}
    for i in sorted({0, max(args.pics) - 1}):                 # results first: the first and the last picture against the reference
        want[i] = hash_ref.picture([p.cpu().numpy() for p in pics[i]])
    got = eng.picture_hash(pics, kinds=hash_ref.KINDS)
    for i, ref in want.items():
        assert got[i] == ref, (i, got[i], ref)
    q = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "p90": float(np.percentile(v, 90))}
    for kind in args.kinds:
        for n in args.pics:
            batch = pics[:n]
            assert eng.picture_hash(batch, kinds=(kind,))[0][kind] == want[0][kind]
            for _ in range(3):                                # warm-up of this shape
                eng.picture_hash(batch, kinds=(kind,), timed=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.picture_hash(batch, kinds=(kind,))
            per_call = time.perf_counter() - t0
            reps = int(min(2000, max(5, args.window / per_call)))
            k0, k1, k2, call = [], [], [], []
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            for _ in range(reps):
                ev[0].record()
                _, ms = eng.picture_hash(batch, kinds=(kind,), timed=True)
                ev[1].record()
                ev[1].synchronize()
                k0.append(ms[0]); k1.append(ms[1]); k2.append(ms[2]); call.append(ev[0].elapsed_time(ev[1]))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):                             # the call as a caller sees it (no kernel events), host clock around a call that ends synchronised
                eng.picture_hash(batch, kinds=(kind,))
            wall = (time.perf_counter() - t0) / reps * 1e3
            # the host path this replaces, per picture: the copy, and what Python can do with it
            copy, host = [], []
            for _ in range(args.host_reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                planes = [[p.cpu().numpy() for p in pic] for pic in batch]
                t1 = time.perf_counter()
                for pl in planes:
                    if kind == "md5":
                        [hashlib.md5(p.tobytes()).digest() for p in pl]
                    elif kind == "checksum":
                        [hash_ref.checksum(p) for p in pl]
                t2 = time.perf_counter()
                copy.append((t1 - t0) * 1e3); host.append((t2 - t0) * 1e3)
            run = {"kind": kind, "n_pics": n, "reps": reps, "hash_chunk_ms": q(k0), "hash_fold_ms": q(k1), "hash_md5_ms": q(k2), "call_events_ms": q(call),
                   "call_host_clock_ms": wall, "device_call_per_picture_ms": wall / n,
                   "host_copy_ms": q(copy), "host_path_ms": q(host), "host_path_is": {"md5": "D2H copy + hashlib.md5", "checksum": "D2H copy + numpy checksum", "crc": "D2H copy alone (floor)"}[kind],
                   "host_path_reps": args.host_reps, "host_path_per_picture_ms": float(np.median(host)) / n}
            if kind != "md5":
                run["hash_chunk_GBps"] = n * plane_bytes / (float(np.median(k0)) * 1e-3) / 1e9
            else:
                run["hash_md5_MBps_per_stream"] = w * h / (float(np.median(k2)) * 1e-3) / 1e6      # the luma plane is the longest chain
            res["runs"].append(run)
    eng.destroy()
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
