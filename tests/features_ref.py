"""Plain-numpy reference of the feature maps (fcu_feature_maps), written from the fork's lines as literally as numpy allows:
getTMVFeature (tools_YS.cpp:1682-1839) with T3x3Filter::filter (:1659-1672) and getSubBlockMean / getSubBlockVariance
(tools_YS.h:106-126) -- float64 means, np.trunc for the double -> Int conversion, the zero ring of every CU, the triangle loops
whose "variance" is ASSIGNED, so that only the last element of the loop order counts -- and FormFeatureVector, Type SOC
(tools_YS.cpp:379-396) on the Outlier plane of getOutlierWithDCT (TEncSlice.cpp:944-1132, REVERSETRANSFORM_OUTLIER 0,
BINARIZE_OUTLIER 0).  It does NOT use the integer identity of the kernel (|trunc(q - S/N)| = |q N - S| >> log2 N): the tests
are that the two agree.

Not pinned by a build of the reference: tools_YS.cpp does not compile on its own (it needs OpenCV and the fork's globals) and the
recipe that builds reference pieces is fixed; like tests/maps_ref.py this reading is pinned by the properties it must satisfy on its
own (tests/test_features.py: a hand-computed block, constant pictures, the transpose, the triangle rule, the SOC sums against
the oracle's OBF map)."""
import numpy as np

TMV, SOC = 130, 16
# aiOrigMask, aiHorMask, aiVerMask, aiDiagMask, aiAntDMask (tools_YS.cpp:1693-1697)
MASKS = [np.array(m).reshape(3, 3) for m in ([0, 0, 0, 0, 1, 0, 0, 0, 0], [0, 0, 0, 1, 0, -1, 0, 0, 0], [0, 1, 0, 0, 0, 0, 0, -1, 0],
                                              [0, 0, 1, 0, 0, 0, -1, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0, -1])]
# partialButterfly4's matrix (g_aiT4)
T4 = np.array([[64, 64, 64, 64], [83, 36, -36, -83], [64, -64, -64, 64], [36, -83, 83, -36]], np.int64)


def level_shapes(w, h):
    return [((h + (64 >> d) - 1) // (64 >> d), (w + (64 >> d) - 1) // (64 >> d)) for d in range(4)]


def level_offsets(w, h):
    o = [0]
    for a, b in level_shapes(w, h):
        o.append(o[-1] + a * b)
    return o


def filter_plane(p, mask):
    """T3x3Filter::filter: zeros, then for 1 <= y, x <= W - 2 the 3x3 correlation with the mask"""
    W = p.shape[0]
    q = np.zeros((W, W), np.int64)
    for i in range(3):
        for j in range(3):
            q[1:W - 1, 1:W - 1] += int(mask[i][j]) * p[i:W - 2 + i, j:W - 2 + j]
    return q


def sub_mean(q, i0, i1, j0, j1):
    return float(q[i0:i1, j0:j1].sum()) / (i1 - i0) / (j1 - j0)


def sub_var(q, mean, i0, i1, j0, j1):
    tmp = np.trunc(q[i0:i1, j0:j1].astype(np.float64) - mean)            # Int tmp = pBlock[..] - iMean
    return float(np.abs(tmp).sum()) / (i1 - i0) / (j1 - j0)


def tmv_block(p):
    """the 5 x 26 doubles of getTMVFeature for one W x W block of samples"""
    p = p.astype(np.int64)
    W = p.shape[0]
    H = W >> 1
    i, j = np.mgrid[0:W, 0:W]
    out = np.zeros((5, 26), np.float64)
    for f, mask in enumerate(MASKS):
        q = filter_plane(p, mask)
        d = out[f]
        d[0] = sub_mean(q, 0, W, 0, W); d[1] = sub_var(q, d[0], 0, W, 0, W)
        d[2] = sub_mean(q, 0, H, 0, W); d[4] = sub_var(q, d[2], 0, H, 0, W)
        d[3] = sub_mean(q, H, W, 0, W); d[5] = sub_var(q, d[3], H, W, 0, W)
        d[6] = sub_mean(q, 0, W, 0, H); d[8] = sub_var(q, d[6], 0, W, 0, H)
        d[7] = sub_mean(q, 0, W, H, W); d[9] = sub_var(q, d[7], 0, W, H, W)
        # the triangles: boolean indexing walks the elements in the order of the fork's loops (i outer, j inner)
        for km, kv, tri in ((10, 12, j < W - i), (11, 13, j >= W - i - 1), (14, 16, j >= i), (15, 17, j < i + 1)):
            el = q[tri]
            mean = float(el.sum()) / (W * W >> 1)
            d[km] = mean
            last = np.trunc(float(el[-1]) - mean)                          # iVariance = ..., not +=: the last element stays
            d[kv] = abs(last) / (W * W >> 1)
        d[18] = sub_mean(q, 0, H, 0, H); d[22] = sub_var(q, d[18], 0, H, 0, H)
        d[19] = sub_mean(q, 0, H, H, W); d[23] = sub_var(q, d[19], 0, H, H, W)
        d[20] = sub_mean(q, H, W, 0, W); d[24] = sub_var(q, d[20], H, W, 0, W)   # (uiCuWidth >> 1, uiCuWidth, 0, uiCuWidth): :1823-1825
        d[21] = sub_mean(q, H, W, H, W); d[25] = sub_var(q, d[21], H, W, H, W)
    return out


def dct4_blocks(Y):
    """partialButterfly x 2 (shift 1, then 8) of every 4x4 block: int64 [h/4, w/4, 16], index k2 * 4 + k1 (TEncSlice.cpp:944-966)"""
    h, w = Y.shape
    B = Y.astype(np.int64).reshape(h // 4, 4, w // 4, 4).transpose(0, 2, 1, 3)      # [by, bx, y, x]
    tmp = (np.einsum("kx,abyx->abky", T4, B) + 1) >> 1                                # tmp[k1][y]
    coef = (np.einsum("jy,abky->abjk", T4, tmp) + 128) >> 8                           # coef[k2][k1]
    return coef.reshape(h // 4, w // 4, 16)


def outlier_plane(Y, yc):
    """pDst of getOutlierWithDCT with REVERSETRANSFORM_OUTLIER 0: |coef| / 100 of the coefficients the thresholds leave, at the
    coefficient's position inside its block; DC cleared (StartFreq 1)"""
    h, w = Y.shape
    c = dct4_blocks(Y)
    c[:, :, 0] = 0
    for x in range(1, 16):
        cx = c[:, :, x]
        cx[(cx < yc[x] * 8.0) & (cx > -yc[x] * 8.0)] = 0
    a = np.abs(c) // 100
    return a.reshape(h // 4, w // 4, 4, 4).transpose(0, 2, 1, 3).reshape(h, w)


def soc_block(o):
    """FormFeatureVector, Type SOC, of one s x s crop of the Outlier plane"""
    s = o.shape[0]
    f = np.zeros(16, np.float64)
    for y in range(4):
        for x in range(4):
            f[y * 4 + x] = o[y:s:4, x:s:4].sum()
    return f


def feature_maps(Y, sets=("tmv", "soc"), yc=None):
    """float32 [NL, F] of one picture; blocks that are not wholly inside get zeros"""
    h, w = Y.shape
    F = (TMV if "tmv" in sets else 0) + (SOC if "soc" in sets else 0)
    off = level_offsets(w, h)
    out = np.zeros((off[4], F), np.float64)
    O = outlier_plane(Y, yc) if "soc" in sets else None
    for d, (bh, bw) in enumerate(level_shapes(w, h)):
        s = 64 >> d
        for by in range(bh):
            for bx in range(bw):
                if bx * s + s > w or by * s + s > h:
                    continue
                row, c = out[off[d] + by * bw + bx], 0
                if "tmv" in sets:
                    row[:TMV] = tmv_block(Y[by * s:by * s + s, bx * s:bx * s + s]).ravel()
                    c = TMV
                if "soc" in sets:
                    row[c:] = soc_block(O[by * s:by * s + s, bx * s:bx * s + s])
    res = out.astype(np.float32)
    assert np.array_equal(res.astype(np.float64), out), "every value is exact in float32"
    return res
