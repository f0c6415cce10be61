#!/usr/bin/env python3
"""Decide the CU quadtrees of an all-intra 8-bit 4:2:0 .yuv clip on an MI355X -- the part of `TAppEncoder -c
encoder_intra_main.cfg` that this repository replaces (no bitstream is written).

  python tools/fcu_decide.py -i clip_1920x1080.yuv -w 1920 -h 1080 -q 32 -f 10 --fast --rec rec.yuv --depth depth.npy

--fast runs the fork's Training / Verifying / Testing cycle (period / training / verifying pictures as in the reference:
60 / 2 / 1); without it every picture gets the exhaustive HM search.  --rec receives the deblocked reconstruction,
--depth an array [pictures, CTUs, 256] of CU depths per 4x4 partition in z-order (TComDataCU::getDepth).

Slices: by default a picture is ONE slice, as in the reference's configuration (SliceMode 0) -- pictures side by side
(--in-flight) are then the source of parallelism.  --slice-ctus N / --row-slices select HM's SliceMode 1 with N CTUs (one
CTU row) per slice: a different encoder configuration (neighbourhood cut and CABAC reset at every slice start), whose
slices are decided concurrently.  --wpp keeps one slice per picture and switches WaveFrontSynchro on (HM's WaveFrontSynchro=1):
the CTU rows of a picture are decided concurrently, each row starting from the contexts the row above had after its second CTU
and waiting for the row above to stay two CTUs ahead.  --tiles CxR keeps one slice per picture and cuts it into C x R uniform
tiles (HM's NumTileColumnsMinus1 / NumTileRowsMinus1 with TileUniformSpacing) decided concurrently; with --wpp the CTU rows of
every tile are decided concurrently as well; --lf-cross-tiles 0 makes the deblocking leave the tile boundaries unfiltered (HM's
LFCrossTileBoundaryFlag, default 1); --lf-cross-slices 0 does the same for the slice boundaries of --slice-ctus / --row-slices /
--slice-rows (HM's LFCrossSliceBoundaryFlag, default 1).  The slice mode is echoed on every picture line.
--report takes the picture line's figures from the device (fcu_picture_report): the PSNR, the picture's bits and the shares of
intra / skipped / merged area; the reconstruction is then copied to the host only when --rec asks for the file.
--hash md5|crc|checksum appends the decoded-picture hash of the reconstruction to the picture line exactly as the reference encoder
prints it with SEIDecodedPictureHash 1 / 2 / 3 (` [MD5:...]`, ` [CRC:...]`, ` [Checksum:...]`, TEncGOP.cpp:1746-1754), taken on the
device (fcu_picture_hash): with --report --hash and no --rec no plane is copied to the host.
--maps FILE.npz saves the decision as pictures, formed on the device (fcu_decision_maps): `depth`, `part_size`, `pred_mode` and
`intra_dir_luma` as arrays [pictures, height / 4, width / 4] aligned with the pixels, and `label0` .. `label3`, the split labels per
64x64 .. 8x8 block ([pictures, ceil(height / s), ceil(width / s)]; -1 absent, 0 not split, 1 split, 2 split forced by the picture edge).
With --fast it also holds `n_obf0` .. `n_obf3`, the fork's N_OBF feature of the same blocks, for the pictures decided with an OBF map
(Verifying and Testing), and `n_obf_poc`, the POCs of those pictures.
--cu-trace FILE.npz decides the Training pictures (all pictures without --fast) with a CU trace bound and saves what fcu_trace_maps
makes of it on the device: `trace_label`, `j0` and `j1` as arrays [Training pictures, NL] in the flat layout of the label maps (the
four levels one after the other) -- the split outcome and both RD costs of every CU the exhaustive search visited, not only of those
on the chosen tree -- and `trace_poc`, the POCs of those pictures.
--features FILE.npz saves the fork's TMV and SOC model inputs of every block, formed on the device (fcu_feature_maps): `features`
[pictures, NL, 146] float32, `feature_names` (the 146 column names) and `features_poc`.  Row r of a picture is the block of element r
of `trace_label` / `j0` / `j1` of --cu-trace for the picture of the same POC: the arrays line up row for row.
--risk (with --fast) runs the cycle on the risk-table model instead of the Naive label: the Training pictures are decided with a CU
trace, the model is trained on the device from their traces and N_OBF maps (fcu_risk_train) and predicts the split labels of every
Verifying and Testing picture (fcu_risk_predict); --risk-tree LEVELS keys the table by the leaves of a key tree over the binned feature maps (fcu_tree_train) instead of N_OBF; --risk-min-count N leaves a bin with fewer than N training samples without a
prediction (default 1; 0 is the fork's rule on every bin).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--help", action="help")
    ap.add_argument("-i", "--input", required=True)
    ap.add_argument("-w", "--width", type=int, required=True)
    ap.add_argument("-h", "--height", type=int, required=True)
    ap.add_argument("-q", "--qp", type=int, default=32)
    ap.add_argument("-f", "--frames", type=int, default=1 << 30)
    ap.add_argument("--fast", action="store_true")
    ap.add_argument("--period", type=int, default=60)
    ap.add_argument("--training", type=int, default=2)
    ap.add_argument("--verifying", type=int, default=1)
    ap.add_argument("--no-deblock", action="store_true")
    ap.add_argument("--in-flight", type=int, default=16, help="pictures decided side by side when the schedule allows it")
    ap.add_argument("--slice-ctus", type=int, default=0, help="SliceMode 1: CTUs per slice (default: one slice per picture)")
    ap.add_argument("--row-slices", action="store_true", help="SliceMode 1 with one CTU row per slice")
    ap.add_argument("--wpp", action="store_true", help="WaveFrontSynchro: one slice per picture, its CTU rows decided as chains that wait for the row above")
    ap.add_argument("--slice-rows", type=int, default=None, help="with --wpp: SliceMode 1 with slices of this many whole CTU rows, the rows of every slice decided as chains")
    ap.add_argument("--tiles", default=None, metavar="CxR", help="one slice per picture cut into C x R uniform tiles decided as chains; with --wpp, WaveFrontSynchro inside every tile")
    ap.add_argument("--lf-cross-tiles", type=int, choices=(0, 1), default=None, help="with --tiles: LFCrossTileBoundaryFlag of the deblocking (default 1: the tile boundaries are filtered)")
    ap.add_argument("--lf-cross-slices", type=int, choices=(0, 1), default=None, help="with slices: LFCrossSliceBoundaryFlag of the deblocking (default 1: the slice boundaries are filtered)")
    ap.add_argument("--report", action="store_true", help="PSNR, bits and intra / skip / merge shares per picture from the device report; no plane is copied to the host unless --rec is given")
    ap.add_argument("--hash", choices=("md5", "crc", "checksum"), default=None, help="append HM's decoded-picture hash of the reconstruction to the picture line, taken on the device")
    ap.add_argument("--rec")
    ap.add_argument("--depth")
    ap.add_argument("--maps", metavar="FILE.npz", help="save the raster depth, part-size, prediction-mode and luma-mode maps and the split-label maps of every picture (with --fast: the N_OBF maps as well)")
    ap.add_argument("--cu-trace", metavar="FILE.npz", help="decide the Training pictures with a CU trace and save its label / J0 / J1 maps (every CU the search visited)")
    ap.add_argument("--features", metavar="FILE.npz", help="save the TMV + SOC features of every block of every picture (features [pictures, NL, 146], feature_names, features_poc); "
                                                           "with --cu-trace the arrays line up row for row: row r of `features` of a picture is the block of element r of trace_label / j0 / j1 of the same POC")
    ap.add_argument("--risk", action="store_true", help="with --fast: predict the split labels of the Verifying / Testing pictures with the risk-table model trained on the Training pictures, all on the device")
    ap.add_argument("--risk-tree", type=int, default=None, metavar="LEVELS", help="with --risk: key the risk table by the leaves of a key tree of LEVELS (0..5) levels trained on the binned feature maps of the Training pictures, in the place of N_OBF")
    ap.add_argument("--risk-min-count", type=int, default=None, metavar="N", help="with --risk: a bin with fewer than N training samples gives no prediction (default 1)")
    args = ap.parse_args()
    if args.risk_tree is not None and not args.risk:
        ap.error("--risk-tree needs --risk")
    if args.risk_min_count is not None and not args.risk:
        ap.error("--risk-min-count needs --risk")
    tiles = None
    if args.tiles is not None:
        try:
            tiles = tuple(int(v) for v in args.tiles.lower().split("x"))
            assert len(tiles) == 2
        except (ValueError, AssertionError):
            ap.error("--tiles takes COLUMNSxROWS, e.g. 4x2")
    import __graft_entry__ as g
    pkg = g.load_package()
    seq = pkg.sequence
    slice_ctus = (args.width + 63) // 64 if args.row_slices else (args.slice_ctus or None)
    try:                                                       # the rules of these combinations: PictureLayout
        dec = seq.SequenceDecider(args.width, args.height, args.qp, slice_ctus=slice_ctus, fast=args.fast, deblock=not args.no_deblock, in_flight=args.in_flight, wpp=args.wpp, slice_rows=args.slice_rows, tiles=tiles, lf_cross_tiles=args.lf_cross_tiles, lf_cross_slices=args.lf_cross_slices, report=args.report, pic_hash=args.hash, maps=True if args.maps else None, cu_trace=bool(args.cu_trace), features=True if args.features else None,
                                  risk=(dict({"min_count": 1 if args.risk_min_count is None else args.risk_min_count}, **({"tree": {"levels": args.risk_tree}} if args.risk_tree is not None else {})) if args.risk else None),
                                  schedule=seq.FastDecisionSchedule(args.period, args.training, args.verifying))
    except ValueError as e:
        ap.error(str(e))
    names = {seq.TRAINING: "training", seq.VERIFYING: "verifying", seq.TESTING: "testing"}
    rec_f = open(args.rec, "wb") if args.rec else None
    depths = []
    maps, traces, feats = {}, {}, {}
    n = 0
    t_all = time.perf_counter()
    while n < args.frames:
        group = []
        for i in range(min(dec.group_size(), args.frames - n)):
            yuv = seq.read_yuv420(args.input, args.width, args.height, n + i)
            if yuv is None:
                break
            group.append(yuv)
        if not group:
            break
        t0 = time.perf_counter()
        res = dec.decide_group(group)
        dt = time.perf_counter() - t0
        for r, yuv in zip(res, group):
            # PSNR of the (deblocked) reconstruction as TEncGOP::xCalculateAddPSNR reports it (TEncGOP.cpp): 10 log10(255^2 N / SSD)
            psnr, more = [], ""
            if args.report:                                    # the sums were formed on the device: nothing but the report came back
                rep = r["report"]
                psnr = [float(v) for v in rep["psnr"]]
                parts = max(int(rep["n_part"]), 1)
                more = (f"  bits {int(rep['bits'])}  intra {100.0 * int(rep['intra_part']) / parts:.1f}% skip {100.0 * int(rep['skip_part']) / parts:.1f}% "
                        f"merge {100.0 * int(rep['merge_part']) / parts:.1f}%")
            else:
                for p, o in zip(r["rec"], yuv):
                    d = p.cpu().numpy().astype(np.int64) - o.astype(np.int64)
                    ssd = float((d * d).sum())
                    psnr.append(999.99 if ssd == 0 else 10.0 * np.log10(255.0 * 255.0 * d.size / ssd))
            digest = pkg.engine.hash_line(args.hash, r["hash"]) if args.hash else ""
            hist = np.bincount(r["depth"].ravel(), minlength=4)
            print(f"POC {r['poc']:4d} {names[r['state']]:9s} [{dec.slice_mode}] skip2Nx2N={r['sw_skip'].tolist()} terminate={r['sw_term'].tolist()} "
                  f"partitions at depth 0..3 = {hist.tolist()}  TU trials {r['tu_trials']}  "
                  f"PSNR Y {psnr[0]:.4f} U {psnr[1]:.4f} V {psnr[2]:.4f} dB{more}{digest}", flush=True)
            if rec_f:
                seq.write_yuv420(rec_f, [p.cpu().numpy() for p in r["rec"]])
            if args.depth:
                depths.append(r["depth"])
            if args.maps:
                m = r["maps"]
                for k in ("depth", "part_size", "pred_mode", "intra_dir_luma"):
                    maps.setdefault(k, []).append(m[k].cpu().numpy())
                for d in range(4):
                    maps.setdefault("label%d" % d, []).append(m["labels"][d].cpu().numpy())
                    if "n_obf" in m:
                        maps.setdefault("n_obf%d" % d, []).append(m["n_obf"][d].cpu().numpy().astype(np.uint16))
                if "n_obf" in m:
                    maps.setdefault("n_obf_poc", []).append(np.int32(r["poc"]))
            if args.features:
                feats.setdefault("features", []).append(r["features"].cpu().numpy())
                feats.setdefault("features_poc", []).append(np.int32(r["poc"]))
        with_trace = [r for r in res if "cu_trace" in r]
        if args.cu_trace and with_trace:                       # one batched call for the Training pictures of the group
            tm = dec.eng.trace_maps(with_trace, labels=True, costs=True)
            for k, name in (("labels", "trace_label"), ("j0", "j0"), ("j1", "j1")):
                traces.setdefault(name, []).extend(tm[k].cpu().numpy())
            traces.setdefault("trace_poc", []).extend(np.int32(r["poc"]) for r in with_trace)
        print(f"  {len(res)} picture(s) side by side: {dt * 1e3:.1f} ms", flush=True)
        n += len(res)
    dt_all = time.perf_counter() - t_all
    if rec_f:
        rec_f.close()
    if args.depth:
        np.save(args.depth, np.stack(depths) if depths else np.zeros((0, 0, 256), np.uint8))
    if args.maps:
        np.savez(args.maps, **{k: np.stack(v) for k, v in maps.items()})
    if args.cu_trace:
        np.savez(args.cu_trace, **{k: np.stack(v) for k, v in traces.items()})
    if args.features:
        np.savez(args.features, feature_names=np.array(pkg.engine.FEATURE_NAMES), **{k: np.stack(v) for k, v in feats.items()})
    dec.close()
    print(f"{n} pictures decided in {dt_all:.2f} s")


if __name__ == "__main__":
    main()
