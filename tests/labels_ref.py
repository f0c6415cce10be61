"""Reference of caller-supplied split labels in plain numpy: the label array an OBF map expresses (the Naive rule N_OBF > 0 written
as labels, what fcu_chain_set_labels must then decide bit for bit as the oracle decides with that OBF map), the synthetic OBF maps
the label tests use, and the label array of depth / part_size rasters (fcu_labels_from_rasters).  Built on tests/maps_ref.py."""
import numpy as np

import maps_ref
from maps_ref import ABSENT, FORCED, NOT_SPLIT, SPLIT  # noqa: F401  (the codes, for the tests)


def flatten(levels):
    """four [BH(d), BW(d)] maps -> the int8 [NL] array, levels one after the other"""
    return np.concatenate([np.asarray(m, np.int8).reshape(-1) for m in levels])


def label_count(w, h):
    return sum(a * b for a, b in maps_ref.level_shapes(w, h))


def whole_mask(w, h, d):
    """[BH(d), BW(d)] bool: the block lies wholly inside the picture"""
    s = 64 >> d
    bh, bw = maps_ref.level_shapes(w, h)[d]
    return ((np.arange(bh)[:, None] + 1) * s <= h) & ((np.arange(bw)[None, :] + 1) * s <= w)


def obf_labels(obf, w, h):
    """the labels an OBF map expresses: N_OBF > 0 -> SPLIT, else NOT_SPLIT; FORCED on the blocks the picture edge cuts"""
    out = []
    for d, n in enumerate(maps_ref.nobf_maps(np.asarray(obf), w, h)):
        m = np.where(n > 0, SPLIT, NOT_SPLIT).astype(np.int8)
        m[~whole_mask(w, h, d)] = FORCED
        out.append(m)
    return flatten(out)


def raster_labels(depth_map, part_size_map, w, h):
    """fcu_labels_from_rasters: maps_ref.label_maps, with no part_size raster read as "never NxN\""""
    ps = np.zeros_like(depth_map, dtype=np.int8) if part_size_map is None else part_size_map
    return flatten(maps_ref.label_maps(depth_map, ps, w, h))


def reached_labels(obf, w, h):
    """per depth the set of Naive labels (0 / 1) of the whole blocks a Testing-state search with every switch on visits: a block is
    visited when every ancestor holds an outlier (is labelled SPLIT) or is cut by the picture edge"""
    n = maps_ref.nobf_maps(np.asarray(obf), w, h)
    seen = []
    for d in range(4):
        vals = set()
        for by in range(n[d].shape[0]):
            for bx in range(n[d].shape[1]):
                if not whole_mask(w, h, d)[by, bx]:
                    continue
                if all(n[e][by >> (d - e), bx >> (d - e)] > 0 or not whole_mask(w, h, e)[by >> (d - e), bx >> (d - e)] for e in range(d)):
                    vals.add(int(n[d][by, bx] > 0))
        seen.append(vals)
    return seen


def _random_obf(w, h, rng):
    obf = np.zeros((h // 4, w // 4), np.int16)

    def fill(x4, y4, s4):
        if x4 >= w // 4 or y4 >= h // 4 or rng.random() < 0.35:
            return
        if s4 == 2:                                           # an 8x8 CU: one to four of its 4x4 blocks are outliers
            k = rng.permutation(4)[:rng.integers(1, 5)]
            for j in k:
                if y4 + j // 2 < h // 4 and x4 + j % 2 < w // 4:
                    obf[y4 + j // 2, x4 + j % 2] = rng.integers(1, 6)
            return
        for j in range(4):
            fill(x4 + (j % 2) * s4 // 2, y4 + (j // 2) * s4 // 2, s4 // 2)
    for cy in range((h + 63) // 64):
        for cx in range((w + 63) // 64):
            fill(cx * 16, cy * 16, 16)
    return obf


def random_obf(w, h, seed):
    """Seeded random blocks: a quadtree walk that leaves a block empty with probability 0.35 at every level and marks one to four
    outliers in every 8x8 CU it reaches.  The first seed from `seed` on is taken whose map makes both Naive labels occur at every
    depth among the CUs a Testing-state search visits (reached_labels): Skip2Nx2N and TerminateCU then both fire at every depth."""
    for s in range(seed, seed + 200):
        obf = _random_obf(w, h, np.random.default_rng(s))
        if all(v == {0, 1} for v in reached_labels(obf, w, h)):
            return obf
    raise AssertionError("no seed gives both labels at every depth")


def obf_maps(w, h, seed=41):
    """the three synthetic OBF maps of the label tests"""
    return {"random": random_obf(w, h, seed), "zero": np.zeros((h // 4, w // 4), np.int16), "positive": np.full((h // 4, w // 4), 3, np.int16)}
