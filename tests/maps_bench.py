#!/usr/bin/env python3
"""Time of the decision maps (fcu_decision_maps) and of the split match (fcu_split_match) on 4K pictures -- a measurement
script, not a test.

For n_pics = 1 and 16 pictures of 3840x2160 in one call, two requests: the depth map alone, and all nineteen byte maps + the
split labels + the N_OBF maps.  Per request: the kernel (maps_ctu) from the call's own events, the call on the host clock (it
ends synchronised), and next to it the host path the call replaces, in the same run: the strided copy of the requested part of
the record heads to the host and the de-interleave in numpy (a gather through the z-order permutation; labels and N_OBF with
array operations, not loops).  The split match likewise: match_ctu and match_pic from the call's events against copying depth and
part_size of both decisions to the host and counting in numpy.  The host paths use nothing these entry points add.

Per kernel the achieved bytes/s are the ALGORITHMIC bytes (computed here from the shapes: the 256-byte rows read per CTU, the OBF
map, the bytes written) over the kernel time, and their share of the HBM rate an MI355X sustains (6.3 TB/s of its 8 TB/s).
Records: heads with random depths 0..3 and part sizes 0..3; OBF maps random.  Every shape is warmed up; a timed window repeats
the call until it spans about a second; medians and spread are reported.  One map of every run is checked against the host path
before anything is timed.  Writes one JSON document (--out) and prints it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_SUSTAINED = 6.3e12


def z_of_raster():
    """[16, 16] -> z-order index of the partition in column x, row y of a CTU (bit interleave)"""
    z = np.zeros((16, 16), np.int64)
    for y in range(16):
        for x in range(16):
            z[y, x] = sum((((x >> i) & 1) << (2 * i)) | (((y >> i) & 1) << (2 * i + 1)) for i in range(4))
    return z


def host_raster(rows, w, h, zr):
    """rows: uint8 [n_ctu, 256] in z-order -> [h/4, w/4]"""
    w_ctu, h_ctu = (w + 63) // 64, (h + 63) // 64
    t = rows[:, zr.reshape(-1)].reshape(h_ctu, w_ctu, 16, 16).transpose(0, 2, 1, 3).reshape(h_ctu * 16, w_ctu * 16)
    return np.ascontiguousarray(t[:h // 4, :w // 4])


def host_labels(depth, part_size, w, h):
    out = []
    for d in range(4):
        s, s4 = 64 >> d, 16 >> d
        dm, pm = depth[::s4, ::s4].astype(np.int16), part_size[::s4, ::s4]
        bh, bw = dm.shape
        whole = ((np.arange(bh)[:, None] + 1) * s <= h) & ((np.arange(bw)[None, :] + 1) * s <= w)
        lab = np.where(dm > d, 1, 0) if d < 3 else np.where(pm == 3, 1, 0)
        if d < 3:
            lab = np.where(whole, lab, 2)
        out.append(np.where(dm < d, -1, lab).astype(np.int8))
    return out


def host_nobf(obf, w, h):
    out, f = [], (obf > 0)
    for d in range(4):
        s4 = 16 >> d
        bh, bw = (h // 4 + s4 - 1) // s4, (w // 4 + s4 - 1) // s4
        p = np.zeros((bh * s4, bw * s4), np.uint16)
        p[:h // 4, :w // 4] = f
        out.append(p.reshape(bh, s4, bw, s4).sum(axis=(1, 3)).astype(np.uint16))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pics", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--window", type=float, default=1.0, help="seconds a timed window should span")
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    e = pkg.engine
    w, h = 3840, 2160
    H4, W4 = h // 4, w // 4
    dev = torch.device("cuda", 0)
    eng = pkg.CuEngine(w, h, max_chains=1)
    n_ctu, nb = eng.n_ctu, e.CTU_OUT_BYTES
    NL = sum(a * b for a, b in e.map_level_shapes(w, h))
    head = e.CtuOut.coeff_y.offset
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    pics, obfs = [], []
    for i in range(max(args.pics)):
        out = torch.zeros((n_ctu, nb), dtype=torch.uint8, device=dev)
        out[:, :head] = torch.randint(0, 4, (n_ctu, head), dtype=torch.uint8, device=dev, generator=gen)
        pics.append(out.view(-1))
        obfs.append((torch.randint(0, 8, (H4, W4), device=dev, generator=gen) - 4).clamp(min=0).to(torch.int16).contiguous())
    all_fields = tuple(sorted(e.MAP_FIELDS, key=e.MAP_FIELDS.get))
    offs = {n: getattr(e.CtuOut, {"cbf_y": "cbf", "cbf_cb": "cbf", "cbf_cr": "cbf", "tskip_y": "tskip", "tskip_cb": "tskip", "tskip_cr": "tskip",
                                  "intra_dir_luma": "intra_dir", "intra_dir_chroma": "intra_dir"}.get(n, n)).offset +
            256 * {"cbf_cb": 1, "cbf_cr": 2, "tskip_cb": 1, "tskip_cr": 2, "intra_dir_chroma": 1}.get(n, 0) for n in all_fields}
    zr = z_of_raster()
    requests = {"depth": dict(fields=("depth",), labels=False, nobf=False), "all_labels_nobf": dict(fields=all_fields, labels=True, nobf=True)}
    q = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "p90": float(np.percentile(v, 90))}
    res = {"width": w, "height": h, "device": torch.cuda.get_device_name(0), "hbm_sustained_Bps": HBM_SUSTAINED, "n_ctu": n_ctu, "maps": [], "match": []}

    def host_maps(batch, req, obf):
        """the path the call replaces: per picture the strided copy of the head's requested part, then numpy"""
        outm = []
        for i, p in enumerate(batch):
            v = p.view(n_ctu, nb)
            hb = (v[:, :256] if req["fields"] == ("depth",) else v[:, :head]).cpu().numpy()
            m = {f: host_raster(hb[:, offs[f]:offs[f] + 256], w, h, zr) for f in req["fields"]}
            if req["labels"]:
                m["labels"] = host_labels(m["depth"], m["part_size"].view(np.int8), w, h)
            if req["nobf"]:
                m["n_obf"] = host_nobf(obf[i].cpu().numpy(), w, h)
            outm.append(m)
        return outm

    for n in args.pics:
        batch, obf = pics[:n], obfs[:n]
        for name, req in requests.items():
            kw = dict(fields=req["fields"], labels=req["labels"], obf=obf if req["nobf"] else None)
            got = eng.decision_maps(batch, **kw)
            want = host_maps(batch[:1], req, obf)[0]                   # results first
            for f in req["fields"]:
                assert np.array_equal(got[f][0].cpu().numpy().view(np.uint8), want[f]), f
            for k in ("labels", "n_obf"):
                if k in want:
                    assert all(np.array_equal(got[k][d][0].cpu().numpy().view(want[k][d].dtype), want[k][d]) for d in range(4)), k
            for _ in range(10):
                eng.decision_maps(batch, timed=True, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                eng.decision_maps(batch, **kw)
            per_call = (time.perf_counter() - t0) / 10
            reps = int(min(3000, max(30, args.window / per_call)))
            kms = [eng.decision_maps(batch, timed=True, **kw)[1] for _ in range(reps)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                eng.decision_maps(batch, **kw)
            wall = (time.perf_counter() - t0) / reps * 1e3
            host = []
            for _ in range(args.host_reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host_maps(batch, req, obf)
                host.append((time.perf_counter() - t0) * 1e3)
            nf = len(req["fields"])
            rd = n_ctu * 256 * nf + (2 * H4 * W4 if req["nobf"] else 0)
            wr = nf * H4 * W4 + (NL if req["labels"] else 0) + (2 * NL if req["nobf"] else 0)
            rate = n * (rd + wr) / (float(np.median(kms)) * 1e-3)
            res["maps"].append({"n_pics": n, "request": name, "reps": reps, "maps_ctu_ms": q(kms), "call_host_clock_ms": wall,
                                "call_includes": "the output allocation in torch, the descriptor upload, the kernel, one synchronise",
                                "host_path_ms": q(host), "host_path_reps": args.host_reps, "bytes_read_per_picture": rd, "bytes_written_per_picture": wr,
                                "maps_ctu_Bps": rate, "share_of_hbm_sustained": rate / HBM_SUSTAINED,
                                "device_call_per_picture_ms": wall / n, "host_path_per_picture_ms": float(np.median(host)) / n})
        # split match: picture i against the next picture generated
        a, b = batch, [pics[(i + 1) % len(pics)] for i in range(n)]
        got = eng.split_match(a, b)
        ps_off = e.CtuOut.part_size.offset

        def host_match():
            outm = []
            for x, y in zip(a, b):
                vx, vy = x.view(n_ctu, nb), y.view(n_ctu, nb)
                d = [host_raster(v[:, :256].cpu().numpy(), w, h, zr) for v in (vx, vy)]
                p = [host_raster(v[:, ps_off:ps_off + 256].cpu().numpy(), w, h, zr).view(np.int8) for v in (vx, vy)]
                la, lb = host_labels(d[0], p[0], w, h), host_labels(d[1], p[1], w, h)
                node = [[[int(((la[k] == i) & (lb[k] == j)).sum()) for j in (0, 1)] for i in (0, 1)] for k in range(4)]
                outm.append({"part_equal": int((d[0] == d[1]).sum()), "node": node})
            return outm

        want = host_match()
        for g_, w_ in zip(got, want):
            assert g_["part_equal"] == w_["part_equal"] and g_["node"].tolist() == w_["node"], (g_, w_)
        for _ in range(10):
            eng.split_match(a, b, timed=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            eng.split_match(a, b)
        per_call = (time.perf_counter() - t0) / 10
        reps = int(min(3000, max(30, args.window / per_call)))
        k1, k2 = [], []
        for _ in range(reps):
            _, ms = eng.split_match(a, b, timed=True)
            k1.append(ms[0]); k2.append(ms[1])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            eng.split_match(a, b)
        wall = (time.perf_counter() - t0) / reps * 1e3
        host = []
        for _ in range(args.host_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_match()
            host.append((time.perf_counter() - t0) * 1e3)
        b1, b2 = n * n_ctu * (4 * 256 + 64), n * (n_ctu * 64 + 208)
        res["match"].append({"n_pics": n, "reps": reps, "match_ctu_ms": q(k1), "match_pic_ms": q(k2), "call_host_clock_ms": wall, "host_path_ms": q(host),
                             "host_path_reps": args.host_reps, "match_ctu_bytes": b1, "match_pic_bytes": b2,
                             "match_ctu_Bps": b1 / (float(np.median(k1)) * 1e-3), "match_pic_Bps": b2 / (float(np.median(k2)) * 1e-3),
                             "match_ctu_share_of_hbm_sustained": b1 / (float(np.median(k1)) * 1e-3) / HBM_SUSTAINED,
                             "device_call_per_picture_ms": wall / n, "host_path_per_picture_ms": float(np.median(host)) / n,
                             "split_match_first_picture": got[0]["split_match"]})
    eng.destroy()
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
