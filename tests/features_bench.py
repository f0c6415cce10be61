#!/usr/bin/env python3
"""Time of the feature maps (fcu_feature_maps) on 4K pictures -- a measurement script, not a test.

For n_pics = 1 and 16 pictures of 3840x2160 in one call and the sets "tmv", "soc" and both: the kernel (feat_ctu) from the call's
own events and the call on the host clock (it ends synchronised), medians over repeated calls after a warm-up.  Per kernel the
achieved bytes/s are the bytes WRITTEN (NL x F x 4 per picture, computed from the shapes) over the kernel time, next to the HBM
rate an MI355X sustains (6.3 TB/s of its 8 TB/s).  In the same run the path the call replaces: the luma plane copied to the host
plus the numpy reference tests/features_ref.py -- timed on a 256x128 CROP of the picture and scaled by the area (the numpy
reference needs minutes for a whole 4K picture); it is a crop, the figure an extrapolation.  One picture is checked against the
reference on that crop before anything is timed.  Writes one JSON document (--out) and prints it."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
HBM_SUSTAINED = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    import features_ref as FR
    pkg = g.load_package()
    w, h, cw, ch = 3840, 2160, 256, 128
    eng = pkg.CuEngine(w, h, max_chains=1)
    NL = eng.label_count()
    planes = [torch.from_numpy(np.ascontiguousarray(pkg.synth.textured(w, h, seed=s)[0])).cuda() for s in (1, 2)]
    planes = [planes[i % 2].clone() for i in range(16)]
    _, yc, obf_ms = eng.obf_prepass(torch.stack(planes[:2]))
    yc16 = np.stack([yc[i % 2] for i in range(16)])
    # check: the crop as a picture of its own (features depend on the block's samples only; SOC on the thresholds given)
    crop = np.ascontiguousarray(planes[0][:ch, :cw].cpu().numpy())
    small = pkg.CuEngine(cw, ch, max_chains=1)
    got = small.feature_maps([torch.from_numpy(crop).cuda()], yc=yc[:1])[0].cpu().numpy()
    t0 = time.perf_counter()
    want = FR.feature_maps(crop, ("tmv", "soc"), yc[0])
    numpy_crop_s = time.perf_counter() - t0
    assert np.array_equal(got, want), "device features differ from the numpy reference on the crop"
    small.destroy()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        planes[0].cpu()
    copy_s = (time.perf_counter() - t0) / 5
    res = {"picture": [w, h], "NL": NL, "hbm_sustained_bytes_per_s": HBM_SUSTAINED, "obf_prepass_kernels_ms_2_pictures": list(obf_ms),
           "host_path": {"luma_copy_to_host_ms_per_picture": copy_s * 1e3, "numpy_reference_crop": [cw, ch], "numpy_reference_crop_s": numpy_crop_s,
                         "numpy_reference_scaled_to_picture_s": numpy_crop_s * (w * h) / (cw * ch), "note": "numpy timed on a crop and scaled by area"},
           "runs": []}
    for n in (1, 16):
        for sets in (("tmv",), ("soc",), ("tmv", "soc")):
            F = len(pkg.engine.feature_columns(sets))
            y = yc16[:n] if "soc" in sets else None
            for _ in range(3):
                eng.feature_maps(planes[:n], sets=sets, yc=y)
            call, kern = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                _, ms = eng.feature_maps(planes[:n], sets=sets, yc=y, timed=True)
                call.append((time.perf_counter() - t0) * 1e3)
                kern.append(ms)
            k = statistics.median(kern)
            written = n * NL * F * 4
            res["runs"].append({"n_pics": n, "sets": list(sets), "F": F, "call_ms_median": statistics.median(call), "kernel_ms_median": k,
                                "kernel_ms_min": min(kern), "kernel_ms_max": max(kern), "bytes_written": written, "bytes_read": n * w * h,
                                "written_bytes_per_s": written / (k * 1e-3), "share_of_hbm_sustained": written / (k * 1e-3) / HBM_SUSTAINED})
    eng.destroy()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
