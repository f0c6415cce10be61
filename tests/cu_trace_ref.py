"""Reference of fcu_label_score and fcu_trace_maps in plain numpy, written from the definitions in include/fcu.h over a host copy
of a picture's CU trace (fcu_cu_trace records, [n_ctu][85]).  It shares nothing with the kernel source.  The double sums are added
in the order the header makes part of the interface: per CTU and depth the CUs in z-order, one term after the other from 0.0; per
picture the CTU records in raster order from 0.0."""
import numpy as np

import maps_ref

CUS_PER_CTU = 85
MAX_DOUBLE = 1.7e+308
CU_TRACE = np.dtype([("j0", np.float64), ("j1", np.float64), ("valid", np.uint8), ("split_won", np.uint8), ("whole_tried", np.uint8),
                     ("split_tried", np.uint8), ("pad", np.uint8, (4,))])
CTU_SCORE = np.dtype([("n", np.uint16, (4, 4)), ("open", np.uint16, (4,)), ("pad", np.uint16, (12,)), ("loss", np.float64, (4, 2))])
PIC_SCORE = np.dtype([("v", np.float64, (4, 6)), ("open", np.uint32, (4,)), ("scored", np.uint32, (4,))])
assert CU_TRACE.itemsize == 24 and CTU_SCORE.itemsize == 128 and PIC_SCORE.itemsize == 224
LEVEL_FIRST = (0, 1, 5, 21)
SPLIT, NOT_SPLIT, ABSENT, FORCED = 1, 0, -1, 2


def cu_index(depth, zidx):
    """fcu_cu_index: zidx = z-order index of the CU's first 4x4 partition inside its CTU"""
    return LEVEL_FIRST[depth] + (zidx >> (8 - 2 * depth))


def node_xy(d, j):
    """CU j (z-order) of depth d inside its CTU: position in units of its own size"""
    x = y = 0
    for b in range(d):
        x |= ((j >> (2 * b)) & 1) << b
        y |= ((j >> (2 * b + 1)) & 1) << b
    return x, y


def nodes(w, h):
    """every node of every CTU of a w x h picture: (ctu, record index, depth, x, y in luma samples, element of the label layout,
    wholly inside), CTUs in raster order, inside a CTU the records in index order -- depth by depth, each depth in z-order"""
    shapes = maps_ref.level_shapes(w, h)
    off = np.concatenate([[0], np.cumsum([a * b for a, b in shapes])])
    w_ctu, h_ctu = (w + 63) // 64, (h + 63) // 64
    for a in range(w_ctu * h_ctu):
        cx, cy = a % w_ctu, a // w_ctu
        for d in range(4):
            s = 64 >> d
            for j in range(4 ** d):
                nx, ny = node_xy(d, j)
                x, y = cx * 64 + nx * s, cy * 64 + ny * s
                if x >= w or y >= h:
                    continue
                yield a, LEVEL_FIRST[d] + j, d, x, y, int(off[d]) + (y // s) * shapes[d][1] + x // s, x + s <= w and y + s <= h


def score(trace, labels, w, h):
    """(per-CTU records [n_ctu] of CTU_SCORE, one PIC_SCORE record) of one picture's trace against one label array"""
    trace = np.asarray(trace).reshape(-1, CUS_PER_CTU)
    labels = np.asarray(labels, np.int8)
    ctu = np.zeros(trace.shape[0], CTU_SCORE)
    for a, t, d, x, y, idx, whole in nodes(w, h):
        r = trace[a, t]
        if not (whole and r["valid"] and r["split_tried"]):
            continue
        v, truth = int(labels[idx]), bool(r["split_won"])
        loss = np.float64(abs(np.float64(r["j0"]) - np.float64(r["j1"])))
        if v == SPLIT:
            ctu["n"][a, d, 0 if truth else 1] += 1
            if not truth:
                ctu["loss"][a, d, 0] = np.float64(ctu["loss"][a, d, 0]) + loss
        elif v == NOT_SPLIT:
            ctu["n"][a, d, 3 if truth else 2] += 1
            if truth:
                ctu["loss"][a, d, 1] = np.float64(ctu["loss"][a, d, 1]) + loss
        else:
            ctu["open"][a, d] += 1
    pic = np.zeros((), PIC_SCORE)
    for a in range(trace.shape[0]):                            # raster order, one record after the other
        for d in range(4):
            for k in range(2):
                pic["v"][d, 4 + k] = np.float64(pic["v"][d, 4 + k]) + np.float64(ctu["loss"][a, d, k])
    pic["v"][:, :4] = ctu["n"].astype(np.float64).sum(axis=0)
    pic["open"] = ctu["open"].astype(np.uint32).sum(axis=0)
    pic["scored"] = ctu["n"].astype(np.uint32).sum(axis=(0, 2))
    return ctu, pic


def maps(trace, w, h):
    """(labels int8 [NL], j0 float64 [NL], j1 float64 [NL]) of one picture's trace"""
    trace = np.asarray(trace).reshape(-1, CUS_PER_CTU)
    NL = sum(a * b for a, b in maps_ref.level_shapes(w, h))
    lab, j0, j1 = np.full(NL, 99, np.int8), np.zeros(NL, np.float64), np.zeros(NL, np.float64)
    for a, t, d, x, y, idx, whole in nodes(w, h):
        r = trace[a, t]
        assert lab[idx] == 99                                  # every element has one block
        if d < 3 and not whole:
            lab[idx] = FORCED
        elif not (r["valid"] and r["split_tried"]):
            lab[idx] = ABSENT
        else:
            lab[idx], j0[idx], j1[idx] = (SPLIT if r["split_won"] else NOT_SPLIT), r["j0"], r["j1"]
    assert not (lab == 99).any()
    return lab, j0, j1
