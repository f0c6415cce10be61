"""Inputs of the decision-map tests, shared by the emulator tests (test_maps.py) and the GPU tests (test_gpu_maps.py): seeded
fcu_ctu_out records holding random VALID quadtrees -- with every entry of a partition outside the picture poisoned -- and seeded
OBF maps, with the numpy reference (maps_ref.py) computed once per case."""
import functools

import numpy as np

import maps_ref

# 208x136: 4 x 3 CTUs, last column 16 samples, last row 8, W4 = 52: the 2-byte store path, forced nodes at levels 0..2 on two sides;
# 72x200: a cut column one 8x8 CU wide, W4 = 18; 64x64: one CTU; 8x8: the smallest picture fcu_create accepts, smaller than a CTU;
# 256x128: whole CTUs and 16-byte rows, the 16-byte store path
SIZES = [(208, 136), (72, 200), (64, 64), (8, 8), (256, 128)]
ALL_FIELDS = tuple(sorted(maps_ref.FIELDS, key=lambda n: maps_ref.FIELDS[n][0]))
MIXED_FIELDS = ("ref_idx", "cbf_cr", "depth", "qp", "intra_dir_luma", "part_size")      # not in record order
FIELD_LISTS = {"one": ("depth",), "all": ALL_FIELDS, "mixed": MIXED_FIELDS}
POISON = {"depth": 7, "part_size": 9, "mv": 0x7fff, "other": 0xee}


def _pkg():
    import __graft_entry__ as g
    return g.load_package()


def records(w, h, seed):
    """uint8 [n_ctu, sizeof(fcu_ctu_out)]: per CTU a random quadtree that is valid for the picture (a block that is not wholly
    inside is split, down to the 8x8 blocks, which a picture cuts nowhere), part sizes, modes, flags and vectors random per
    partition within their ranges.  EVERY entry of a partition outside the picture holds a poison value no inside entry can
    hold: depth 7, part_size 9, mv 0x7fff, 0xee in the other arrays."""
    e = _pkg().engine
    rng = np.random.default_rng(seed)
    w_ctu, h_ctu = (w + 63) // 64, (h + 63) // 64
    n_ctu = w_ctu * h_ctu
    r = np.zeros((n_ctu, e.CTU_OUT_BYTES), np.uint8)
    rngs = {"part_size": None, "depth": None, "pred_mode": (0, 2), "skip": (0, 2), "merge_flag": (0, 2), "merge_idx": (0, 5), "tr_idx": (0, 3),
            "cbf_y": (0, 8), "cbf_cb": (0, 8), "cbf_cr": (0, 8), "tskip_y": (0, 2), "tskip_cb": (0, 2), "tskip_cr": (0, 2),
            "intra_dir_luma": (0, 35), "intra_dir_chroma": (0, 37), "qp": (-5, 52), "inter_dir": (0, 3), "mvp_idx": (-1, 2), "ref_idx": (-1, 4)}
    off = {n: maps_ref.field_offset(_pkg(), n) for n in maps_ref.FIELDS}
    mv_off = e.CtuOut.mv.offset
    for a in range(n_ctu):
        x0, y0 = (a % w_ctu) * 64, (a // w_ctu) * 64
        depth = np.full(256, POISON["depth"], np.uint8)
        ps = np.full(256, POISON["part_size"], np.int8)

        def grow(x, y, d):
            s = 64 >> d
            if x >= w or y >= h:
                return
            whole = x + s <= w and y + s <= h
            if d < 3 and (not whole or rng.random() < 0.55):
                for k in range(4):
                    grow(x + (k & 1) * (s // 2), y + (k >> 1) * (s // 2), d + 1)
                return
            size = int(rng.choice([0, 3, 3, 1, 2])) if d == 3 else int(rng.choice([0, 0, 1, 2, 4, 5, 6, 7]))
            for yy in range(y, y + s, 4):
                for xx in range(x, x + s, 4):
                    z = maps_ref.xy_to_z((xx - x0) // 4, (yy - y0) // 4)
                    depth[z], ps[z] = d, size

        grow(x0, y0, 0)
        inside = depth != POISON["depth"]
        for name, lim in rngs.items():
            v = depth if name == "depth" else (ps.view(np.uint8) if name == "part_size" else
                                               np.where(inside, rng.integers(lim[0], lim[1], 256), POISON["other"]).astype(np.int64).astype(np.uint8))
            r[a, off[name]:off[name] + 256] = v
        mv = np.where(inside[:, None], rng.integers(-2000, 2000, (256, 2)), POISON["mv"]).astype("<i2")
        r[a, mv_off:mv_off + 1024] = mv.view(np.uint8).reshape(-1)
        # the arrays no map names (width, height, tq_bypass, chroma_qp_adj, ipcm, mvd) and the coefficients stay arbitrary
        for name in ("width", "height", "tq_bypass", "chroma_qp_adj", "ipcm"):
            o = getattr(e.CtuOut, name).offset
            r[a, o:o + 256] = rng.integers(0, 256, 256, dtype=np.uint8)
    return r


def obf_map(w, h, seed):
    """int16 [h/4, w/4]: about half the counts zero, a few negative (never counted), the others positive"""
    rng = np.random.default_rng(seed)
    v = rng.integers(-1, 40, (h // 4, w // 4))
    return np.where(rng.random(v.shape) < 0.5, 0, v).astype(np.int16)


def inside_entries(w, h):
    """bool [n_ctu, 256]: partition z of CTU a lies inside the picture"""
    w_ctu, h_ctu = (w + 63) // 64, (h + 63) // 64
    xy = [maps_ref.z_to_xy(z) for z in range(256)]
    return np.array([[(a % w_ctu) * 64 + 4 * x < w and (a // w_ctu) * 64 + 4 * y < h for x, y in xy] for a in range(w_ctu * h_ctu)])


@functools.lru_cache(maxsize=None)
def case(w, h, seed):
    """(records, obf map, reference of every output with all fields) -- computed once, never modified"""
    r, obf = records(w, h, seed), obf_map(w, h, seed + 500)
    want = maps_ref.picture_maps(_pkg(), r, w, h, ALL_FIELDS, mv=True, labels=True, obf=obf)
    for a in [r, obf, want["bytes"], want["mv"]] + want["labels"] + want["n_obf"]:
        a.setflags(write=False)
    return r, obf, want


def select(want, fields, mv=True, labels=True, n_obf=True):
    """the reference of a case narrowed to a field list (in that order) and to the outputs asked for"""
    out = {"bytes": np.stack([want["bytes"][ALL_FIELDS.index(f)] for f in fields]) if fields else None}
    for k, on in (("mv", mv), ("labels", labels), ("n_obf", n_obf)):
        if on:
            out[k] = want[k]
    return out


@functools.lru_cache(maxsize=None)
def match_case(w, h, seed_a, seed_b):
    ref = maps_ref.split_match(_pkg(), case(w, h, seed_a)[0], case(w, h, seed_b)[0], w, h)
    return case(w, h, seed_a)[0], case(w, h, seed_b)[0], ref
