"""Reference of the decision maps and of the split match (fcu_decision_maps, fcu_split_match) in plain numpy, written from the
definitions in include/fcu.h over a host copy of a picture's fcu_ctu_out records.  It shares nothing with the kernel source:
z-order is the bit de-interleave of a partition's column and row, computed here; labels and counts are loops over blocks."""
import numpy as np

# name -> (FCU_MAP_* id, field of fcu_ctu_out, plane of that field, numpy type of the entries)
FIELDS = {"depth": (0, "depth", 0, np.uint8), "part_size": (1, "part_size", 0, np.int8), "pred_mode": (2, "pred_mode", 0, np.int8),
          "skip": (3, "skip", 0, np.uint8), "merge_flag": (4, "merge_flag", 0, np.uint8), "merge_idx": (5, "merge_idx", 0, np.uint8),
          "tr_idx": (6, "tr_idx", 0, np.uint8), "cbf_y": (7, "cbf", 0, np.uint8), "cbf_cb": (8, "cbf", 1, np.uint8), "cbf_cr": (9, "cbf", 2, np.uint8),
          "tskip_y": (10, "tskip", 0, np.uint8), "tskip_cb": (11, "tskip", 1, np.uint8), "tskip_cr": (12, "tskip", 2, np.uint8),
          "intra_dir_luma": (13, "intra_dir", 0, np.uint8), "intra_dir_chroma": (14, "intra_dir", 1, np.uint8), "qp": (15, "qp", 0, np.int8),
          "inter_dir": (16, "inter_dir", 0, np.uint8), "mvp_idx": (17, "mvp_idx", 0, np.int8), "ref_idx": (18, "ref_idx", 0, np.int8)}
ABSENT, NOT_SPLIT, SPLIT, FORCED = -1, 0, 1, 2
SIZE_NXN = 3
MATCH_KEYS = ("part_total", "part_equal", "node", "only_a", "only_b")


def z_to_xy(z):
    """4x4 partition z of a 64x64 CTU in z-order -> its column and row (0..15): x takes the even bits of z, y the odd ones"""
    x = sum(((z >> (2 * i)) & 1) << i for i in range(4))
    y = sum(((z >> (2 * i + 1)) & 1) << i for i in range(4))
    return x, y


def xy_to_z(x, y):
    return sum((((x >> i) & 1) << (2 * i)) | (((y >> i) & 1) << (2 * i + 1)) for i in range(4))


def field_offset(pkg, name):
    _, field, plane, _ = FIELDS[name]
    return getattr(pkg.engine.CtuOut, field).offset + 256 * plane


def records_2d(pkg, records, w, h):
    n_ctu = ((w + 63) // 64) * ((h + 63) // 64)
    nb = pkg.engine.CTU_OUT_BYTES
    return np.asarray(records, np.uint8).reshape(-1)[:n_ctu * nb].reshape(n_ctu, nb)


def raster(pkg, records, w, h, name):
    """[h/4, w/4] map of one byte-per-partition array (or, name "mv", the int16 [h/4, w/4, 2] motion map): only partitions
    inside the picture are looked at"""
    r = records_2d(pkg, records, w, h)
    w_ctu = (w + 63) // 64
    if name == "mv":
        out = np.zeros((h // 4, w // 4, 2), np.int16)
        off = pkg.engine.CtuOut.mv.offset
    else:
        out = np.zeros((h // 4, w // 4), FIELDS[name][3])
        off = field_offset(pkg, name)
    for y4 in range(h // 4):
        for x4 in range(w // 4):
            a, z = (y4 // 16) * w_ctu + x4 // 16, xy_to_z(x4 % 16, y4 % 16)
            if name == "mv":
                out[y4, x4] = r[a, off + 4 * z:off + 4 * z + 4].view("<i2")
            else:
                out[y4, x4] = r[a, off + z:off + z + 1].view(out.dtype)[0]
    return out


def label(d, depth, part_size, whole):
    if depth < d:
        return ABSENT
    if d < 3 and not whole:
        return FORCED
    if d < 3:
        return SPLIT if depth > d else NOT_SPLIT
    return SPLIT if part_size == SIZE_NXN else NOT_SPLIT


def label_maps(depth_map, part_size_map, w, h):
    """four int8 maps [ceil(h / s), ceil(w / s)], s = 64 >> d, from the raster depth and part-size maps"""
    out = []
    for d in range(4):
        s = 64 >> d
        m = np.zeros(((h + s - 1) // s, (w + s - 1) // s), np.int8)
        for by in range(m.shape[0]):
            for bx in range(m.shape[1]):
                whole = bx * s + s <= w and by * s + s <= h
                m[by, bx] = label(d, int(depth_map[by * s // 4, bx * s // 4]), int(part_size_map[by * s // 4, bx * s // 4]), whole)
        out.append(m)
    return out


def nobf_maps(obf, w, h):
    """four uint16 maps of the label maps' shapes: 4x4 blocks of the block's area inside the picture whose OBF count is > 0"""
    out = []
    for d in range(4):
        s4 = 16 >> d
        m = np.zeros(((h // 4 + s4 - 1) // s4, (w // 4 + s4 - 1) // s4), np.uint16)
        for by in range(m.shape[0]):
            for bx in range(m.shape[1]):
                m[by, bx] = int((obf[by * s4:(by + 1) * s4, bx * s4:(bx + 1) * s4] > 0).sum())      # (slices end at the picture)
        out.append(m)
    return out


def depth_from_labels(labels, w, h):
    """the depth map inside the picture rebuilt from the four label maps alone"""
    out = np.full((h // 4, w // 4), 255, np.uint8)
    for y4 in range(h // 4):
        for x4 in range(w // 4):
            for d in range(4):
                v = int(labels[d][y4 >> (4 - d), x4 >> (4 - d)])
                assert v != ABSENT
                if v == NOT_SPLIT or d == 3:
                    out[y4, x4] = d
                    break
    return out


def split_match(pkg, rec_a, rec_b, w, h):
    """the fcu_pic_match fields as Python integers / int64 arrays"""
    maps = [(raster(pkg, r, w, h, "depth"), raster(pkg, r, w, h, "part_size")) for r in (rec_a, rec_b)]
    la, lb = [label_maps(dm, pm, w, h) for dm, pm in maps]
    out = {"part_total": (h // 4) * (w // 4), "part_equal": int((maps[0][0] == maps[1][0]).sum()),
           "node": np.zeros((4, 2, 2), np.int64), "only_a": np.zeros(4, np.int64), "only_b": np.zeros(4, np.int64)}
    for d in range(4):
        for by in range(la[d].shape[0]):
            for bx in range(la[d].shape[1]):
                a, b = int(la[d][by, bx]), int(lb[d][by, bx])
                if a in (0, 1) and b in (0, 1):
                    out["node"][d, a, b] += 1
                elif a in (0, 1) and b == ABSENT:
                    out["only_a"][d] += 1
                elif b in (0, 1) and a == ABSENT:
                    out["only_b"][d] += 1
    return out


def picture_maps(pkg, records, w, h, fields, mv=False, labels=False, obf=None):
    """everything fcu_decision_maps gives for one picture: {"bytes": [n_fields, h/4, w/4] uint8 (the bytes verbatim), "mv", "labels":
    four maps, "n_obf": four maps}"""
    out = {"bytes": np.stack([raster(pkg, records, w, h, f).view(np.uint8) for f in fields]) if fields else None}
    if mv:
        out["mv"] = raster(pkg, records, w, h, "mv")
    if labels:
        out["labels"] = label_maps(raster(pkg, records, w, h, "depth"), raster(pkg, records, w, h, "part_size"), w, h)
    if obf is not None:
        out["n_obf"] = nobf_maps(np.asarray(obf), w, h)
    return out


def level_shapes(w, h):
    return [((h + (64 >> d) - 1) // (64 >> d), (w + (64 >> d) - 1) // (64 >> d)) for d in range(4)]


def split_levels(flat, w, h):
    """[.., NL] array of the four levels one after the other -> four arrays [.., BH(d), BW(d)]"""
    out, o = [], 0
    for bh, bw in level_shapes(w, h):
        out.append(flat[..., o:o + bh * bw].reshape(flat.shape[:-1] + (bh, bw)))
        o += bh * bw
    assert o == flat.shape[-1]
    return out


def assert_maps_equal(got, want, what=""):
    for k, v in want.items():
        if v is None:
            continue
        if isinstance(v, list):
            for d in range(4):
                g = np.asarray(got[k][d])
                assert g.shape == v[d].shape and g.dtype.itemsize == v[d].dtype.itemsize and np.array_equal(g.view(v[d].dtype), v[d]), (what, k, d)
        else:
            g = np.asarray(got[k])
            assert g.shape == v.shape and g.dtype == v.dtype and np.array_equal(g, v), (what, k)


def assert_match_equal(got, want, what=""):
    for k in MATCH_KEYS:
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)), (what, k, got[k], want[k])
