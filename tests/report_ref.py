"""Reference of the picture report (fcu_picture_report) in plain numpy, over host copies of the original planes, the
reconstruction planes and the picture's fcu_ctu_out records.  It shares nothing with the kernel source: inside / outside the
picture comes from its own z-order computation (de-interleaving the bits of the partition index), the sums are Python integers /
int64, and the PSNR is HM's expression (TEncGOP.cpp:2254-2256) in double precision through libm's log10."""
import math

import numpy as np

CTU_REPORT = np.dtype([("ssd", np.uint32, (3,)), ("bits", np.uint32), ("bins", np.uint32), ("dist", np.uint32),
                       ("n_part", np.uint16), ("depth_part", np.uint16, (4,)), ("part_size_part", np.uint16, (8,)), ("intra_part", np.uint16),
                       ("skip_part", np.uint16), ("merge_part", np.uint16), ("cbf_part", np.uint16, (3,)), ("pad", np.uint16)])
SUMMED = ("ssd", "bits", "bins", "dist", "n_part", "depth_part", "part_size_part", "intra_part", "skip_part", "merge_part", "cbf_part")
FIELDS = SUMMED + ("n_samples", "psnr")


def z_to_xy(z):
    """4x4 partition z of a 64x64 CTU in z-order -> its column and row (0..15): x takes the even bits of z, y the odd ones"""
    x = sum(((z >> (2 * i)) & 1) << i for i in range(4))
    y = sum(((z >> (2 * i + 1)) & 1) << i for i in range(4))
    return x, y


def _fields(pkg):
    """byte offsets of the fields of fcu_ctu_out that the report reads, from the binding's structure"""
    c = pkg.engine.CtuOut
    return {n: getattr(c, n).offset for n in ("depth", "skip", "part_size", "pred_mode", "cbf", "merge_flag", "total_dist", "total_bits", "total_bins")}


def psnr(ssd, n):
    return 10.0 * math.log10(255.0 * 255.0 * float(n) / float(ssd)) if ssd else 999.99


def picture_report(pkg, org, rec, records):
    """org, rec: (Y, U, V) uint8 arrays; records: the picture's fcu_ctu_out array as uint8 [n_ctu, sizeof(fcu_ctu_out)] (or flat).
    Returns (dict of the fcu_pic_report fields, structured array [n_ctu] of the fcu_ctu_report records)."""
    h, w = org[0].shape
    w_ctu, h_ctu = (w + 63) // 64, (h + 63) // 64
    n_ctu = w_ctu * h_ctu
    nb = pkg.engine.CTU_OUT_BYTES
    records = np.asarray(records, np.uint8).reshape(-1)[:n_ctu * nb].reshape(n_ctu, nb)
    off = _fields(pkg)
    xy = [z_to_xy(z) for z in range(256)]
    ctu = np.zeros(n_ctu, CTU_REPORT)
    for a in range(n_ctu):
        cx, cy = a % w_ctu, a // w_ctu
        r = records[a]
        c = ctu[a]
        for k in range(3):
            s = 1 if k else 0
            x0, y0, x1, y1 = (cx * 64) >> s, (cy * 64) >> s, min(cx * 64 + 64, w) >> s, min(cy * 64 + 64, h) >> s
            d = org[k][y0:y1, x0:x1].astype(np.int64) - rec[k][y0:y1, x0:x1].astype(np.int64)
            c["ssd"][k] = int((d * d).sum())
        for name, key in (("bits", "total_bits"), ("bins", "total_bins"), ("dist", "total_dist")):
            c[name] = int(r[off[key]:off[key] + 4].view("<u4")[0])
        inside = np.array([cx * 64 + 4 * x < w and cy * 64 + 4 * y < h for x, y in xy])
        depth = r[off["depth"]:off["depth"] + 256]
        ps = r[off["part_size"]:off["part_size"] + 256].view(np.int8)
        pm = r[off["pred_mode"]:off["pred_mode"] + 256].view(np.int8)
        c["n_part"] = int(inside.sum())
        for d_ in range(4):
            c["depth_part"][d_] = int((inside & (depth == d_)).sum())
        for s_ in range(8):
            c["part_size_part"][s_] = int((inside & (ps == s_)).sum())
        c["intra_part"] = int((inside & (pm == 1)).sum())
        c["skip_part"] = int((inside & (r[off["skip"]:off["skip"] + 256] != 0)).sum())
        c["merge_part"] = int((inside & (r[off["merge_flag"]:off["merge_flag"] + 256] != 0)).sum())
        for k in range(3):
            c["cbf_part"][k] = int((inside & ((r[off["cbf"] + 256 * k:off["cbf"] + 256 * (k + 1)] & 1) != 0)).sum())
    pic = sum_records(ctu)
    pic["n_samples"] = np.array([w * h, (w // 2) * (h // 2), (w // 2) * (h // 2)], np.uint64)
    pic["psnr"] = np.array([psnr(int(pic["ssd"][k]), int(pic["n_samples"][k])) for k in range(3)], np.float64)
    return pic, ctu


def sum_records(ctu):
    """the sums report_pic forms from per-CTU records (Python integers: no width to overflow)"""
    out = {}
    for n in SUMMED:
        v = ctu[n]
        out[n] = np.array([sum(int(x) for x in v[:, k]) for k in range(v.shape[1])], np.uint64) if v.ndim == 2 else sum(int(x) for x in v)
    return out


def assert_equal(got_pic, got_ctu, want_pic, want_ctu, what=""):
    """exact equality of every field of both structures (psnr as doubles)"""
    for n in FIELDS:
        g, w = np.asarray(got_pic[n]), np.asarray(want_pic[n])
        assert g.shape == w.shape and np.array_equal(g.astype(np.float64) if n == "psnr" else g.astype(np.uint64), w), (what, n, g, w)
    if got_ctu is not None:
        assert got_ctu.shape == want_ctu.shape, (what, got_ctu.shape, want_ctu.shape)
        for n in CTU_REPORT.names:
            assert np.array_equal(got_ctu[n], want_ctu[n]), (what, "ctu", n, got_ctu[n], want_ctu[n])
        summed = sum_records(got_ctu)                        # the per-CTU records against the picture sums
        for n in SUMMED:
            assert np.array_equal(np.asarray(summed[n]).astype(np.uint64), np.asarray(got_pic[n]).astype(np.uint64)), (what, "sum", n)
