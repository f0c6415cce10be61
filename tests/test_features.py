"""The feature-map kernel (csrc/fcu_features.h: feat_ctu) on the CPU (tests/emu/features_emu.cpp: the kernel source with the HIP
keywords defined away, the grid run as a loop with the LDS poisoned before every workgroup, behind features_args_check of
fcu_host.h) against the numpy reference tests/features_ref.py: every value of every case equal as float32, no tolerance; the
properties the reference must have on its own; the refusals; the column names."""
import ctypes as C
import os

import numpy as np
import pytest

import features_cases as FC
import features_ref as FR
import hmo_py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -2
MASK = {"tmv": 1, "soc": 2}


def lib():
    L = C.CDLL(os.path.join(ROOT, "tests", "emu", "libfeatures_emu.so"))
    L.features_emu.argtypes = [C.c_int] * 4 + [C.c_void_p] * 3
    L.features_emu_last_error.restype = C.c_char_p
    return L


def at_offset(a, offset):
    """a copy of the array whose first byte sits `offset` bytes past a 16-byte boundary"""
    raw = np.zeros(a.nbytes + 48, np.uint8)
    start = (-raw.ctypes.data) % 16 + offset
    v = raw[start:start + a.nbytes].view(a.dtype).reshape(a.shape)
    v[...] = a
    assert v.ctypes.data % 16 == offset % 16
    return v


def emu(w, h, lumas, sets, ycs=None, offset=0, out=None, fill=0xaa):
    """lumas: list of planes.  Returns float32 [n, NL, F] (a view of `out`, or of a new buffer of stale bytes)"""
    n, NL = len(lumas), FR.level_offsets(w, h)[4]
    F = sum({"tmv": FR.TMV, "soc": FR.SOC}[s] for s in sets)
    keep = [at_offset(np.ascontiguousarray(y), offset) for y in lumas]
    ptrs = (C.c_void_p * n)(*[y.ctypes.data for y in keep])
    yc = np.ascontiguousarray(np.stack(ycs), np.float64) if ycs is not None else None
    if out is None:
        out = at_offset(np.full(n * NL * F * 4, fill, np.uint8), 4)        # 4-byte aligned and no more
    rc = lib().features_emu(w, h, n, sum(MASK[s] for s in sets), ptrs, yc.ctypes.data if yc is not None else None, out.ctypes.data)
    assert rc == 0, lib().features_emu_last_error()
    return out.view(np.float32).reshape(n, NL, F)


@pytest.mark.parametrize("sets", [("tmv",), ("soc",), ("tmv", "soc")])
@pytest.mark.parametrize("kind", FC.KINDS)
@pytest.mark.parametrize("w,h", FC.SIZES)
def test_every_value_equals_the_reference(w, h, kind, sets, built):
    Y, yc, yh, want, want_hand = FC.case(w, h, kind)
    got = emu(w, h, [Y], sets, [yc] if "soc" in sets else None)
    assert np.array_equal(got[0], FC.select(want, sets)), (w, h, kind, sets, np.argwhere(got[0] != FC.select(want, sets))[:5])


@pytest.mark.parametrize("w,h", FC.SIZES)
def test_coefficients_exactly_on_the_threshold(w, h, built):
    Y, yc, yh, want, want_hand = FC.case(w, h, "textured")
    c = np.abs(FR.dct4_blocks(Y))
    assert any(yh[k] > 0 and (c[:, :, k] == yh[k] * 8).any() for k in range(1, 16))     # the case holds what it is for
    got = emu(w, h, [Y], ("soc",), [yh])
    assert np.array_equal(got[0], want_hand)


@pytest.mark.parametrize("offset", [1, 3, 4, 7, 9])
def test_planes_at_odd_byte_offsets(offset, built):
    """the 8-byte loads are taken for planes on 8 bytes only; every other base goes byte by byte"""
    w, h = 208, 136
    Y, yc, _, want, _ = FC.case(w, h, "textured")
    assert np.array_equal(emu(w, h, [Y], FC.ALL, [yc], offset=offset)[0], want)


def test_batch_of_two_keeps_the_pictures_apart(built):
    w, h = 72, 200
    a, b = FC.case(w, h, "textured"), FC.case(w, h, "textured", 22)
    got = emu(w, h, [a[0], b[0]], FC.ALL, [a[1], b[1]])
    assert np.array_equal(got[0], a[3]) and np.array_equal(got[1], b[3]) and not np.array_equal(a[3], b[3])
    assert not np.array_equal(a[1], b[1]) or not np.array_equal(a[3][:, FR.TMV:], b[3][:, FR.TMV:])


def test_stale_buffer_is_fully_overwritten_and_a_second_call_changes_nothing(built):
    w, h = 208, 136
    Y, yc, _, want, _ = FC.case(w, h, "textured")
    n = want.size * 4
    buf = at_offset(np.full(n, 0xaa, np.uint8), 4)
    got = emu(w, h, [Y], FC.ALL, [yc], out=buf)
    assert np.array_equal(got[0], want)
    first = buf.tobytes()
    emu(w, h, [Y], FC.ALL, [yc], out=buf)
    assert buf.tobytes() == first
    other = emu(w, h, [Y], FC.ALL, [yc], fill=0x55)         # (0x55 underneath instead of 0xaa: no byte left unwritten)
    assert other.tobytes() == first


# ---- the reference pinned by what it must satisfy on its own ------------------------------------------------------------------

# p[i][j] = 8 i + 3 j, with 40 added at (2, 5).  Interior 6 x 6; by hand, filter 0: the interior sum is
# sum(8 i + 3 j, 1 <= i, j <= 6) + 40 = 8 * 21 * 6 + 3 * 21 * 6 + 40 = 1426, so the mean is 1426 / 64 = 22.28125; filter 1 is -6
# everywhere inside but at (2, 4): -46 and (2, 6): +34, sum 36 * -6 - 40 + 40 = -216, mean -3.375; filter 2 is -16 but at (1, 5): -56 and
# (3, 5): +24, sum -576, mean -9.0.
HAND_P = np.array([[8 * i + 3 * j + (40 if (i, j) == (2, 5) else 0) for j in range(8)] for i in range(8)], np.uint8)
HAND_VALUES = np.array([
    [22.28125, 19.96875, 16.15625, 28.40625, 14.09375, 24.34375, 19.125, 25.4375, 17.25, 22.25, 20.5, 32.53125, 0.625, 1.0, 23.78125, 28.0, 0.71875, 0.875, 12.375, 19.9375, 28.40625, 30.9375, 10.5, 17.0, 24.34375, 26.625],
    [-3.375, 3.609375, -3.375, -3.375, 4.78125, 2.4375, -3.375, -3.375, 2.4375, 4.78125, -5.1875, -2.6875, 0.15625, 0.0625, -3.9375, -3.9375, 0.09375, 0.09375, -3.375, -3.375, -3.375, -3.375, 2.4375, 7.125, 2.4375, 2.4375],
    [-9.0, 8.90625, -9.0, -9.0, 9.9375, 7.875, -9.0, -9.0, 7.875, 9.9375, -11.75, -9.25, 0.34375, 0.28125, -10.5, -10.5, 0.3125, 0.3125, -9.0, -9.0, -9.0, -9.0, 7.875, 12.0, 7.875, 7.875],
    [-5.625, 5.546875, -5.625, -5.625, 6.65625, 4.4375, -5.625, -5.625, 4.4375, 6.65625, -6.5625, -6.5625, 0.1875, 0.1875, -6.5625, -6.5625, 0.1875, 0.1875, -5.625, -5.625, -5.625, -5.625, 4.4375, 8.875, 4.4375, 4.4375],
    [-12.375, 11.265625, -12.375, -12.375, 12.21875, 10.3125, -12.375, -12.375, 10.3125, 12.21875, -15.6875, -13.1875, 0.46875, 0.40625, -14.4375, -14.4375, 0.4375, 0.4375, -12.375, -12.375, -12.375, -12.375, 10.3125, 14.125, 10.3125, 10.3125]])


def test_hand_computed_block():
    got = FR.tmv_block(HAND_P)
    assert got[0][0] == 1426 / 64 and got[1][0] == -216 / 64 and got[2][0] == -576 / 64
    assert np.array_equal(got, HAND_VALUES), np.argwhere(got != HAND_VALUES)
    Y = np.zeros((8, 8), np.uint8)
    Y[...] = HAND_P
    assert np.array_equal(FR.feature_maps(Y, ("tmv",))[-1].astype(np.float64), HAND_VALUES.ravel())      # the one 8x8 block of an 8x8 picture


@pytest.mark.parametrize("value", [0, 1, 117, 255])
def test_constant_picture(value):
    """filter 0 sees value * (share of the region that is not ring), the difference filters see nothing"""
    Y = np.full((64, 64), value, np.uint8)
    f = FR.feature_maps(Y, ("tmv",)).astype(np.float64)
    off = FR.level_offsets(64, 64)
    for d in range(4):
        W = 64 >> d
        H = W // 2
        row = f[off[d]]
        assert not row[26:].any()
        inner, half, quad = (W - 2) ** 2, (W - 2) * (H - 1), (H - 1) ** 2
        tri = (W - 2) * (W - 3) // 2                                        # interior elements of a triangle that holds its diagonal...
        assert row[0] == value * inner / W ** 2
        assert all(row[k] == value * half / (W * H) for k in (2, 3, 6, 7, 20))
        assert all(row[k] == value * quad / (H * H) for k in (18, 19, 21))
        # j < W - i and j >= W - i - 1 hold the anti-diagonal, whose interior has W - 2 elements; likewise the diagonal
        assert all(row[k] == value * (tri + (W - 2)) / (W * W // 2) for k in (10, 11, 14, 15))


@pytest.mark.parametrize("w,h", [(64, 64), (72, 200)])
def test_transpose_swaps_rows_with_columns_and_filter_1_with_2(w, h):
    Y = FC.case(w, h, "textured")[0]
    a, b = FR.feature_maps(Y, ("tmv",)), FR.feature_maps(np.ascontiguousarray(Y.T), ("tmv",))
    oa, ob = FR.level_offsets(w, h), FR.level_offsets(h, w)
    for d, (bh, bw) in enumerate(FR.level_shapes(w, h)):
        A = a[oa[d]:oa[d + 1]].reshape(bh, bw, 5, 26)
        B = b[ob[d]:ob[d + 1]].reshape(bw, bh, 5, 26).transpose(1, 0, 2, 3)
        # rows <-> columns of the same filter for the symmetric filters 0 and 4 (the anti-diagonal mask is its own transpose);
        # hor <-> ver (same sign: p[i][j-1] - p[i][j+1] becomes p[i-1][j] - p[i+1][j]); the diagonal filter changes sign
        for fa, fb, sign in ((0, 0, 1), (1, 2, 1), (2, 1, 1), (4, 4, 1), (3, 3, -1)):
            for ka, kb in ((0, 0), (2, 6), (3, 7), (6, 2), (7, 3), (18, 18), (21, 21)):
                assert np.array_equal(A[:, :, fa, ka], sign * B[:, :, fb, kb]), (d, fa, ka)
            for ka, kb in ((1, 1), (4, 8), (5, 9), (8, 4), (9, 5), (22, 22), (25, 25)):
                assert np.array_equal(A[:, :, fa, ka], B[:, :, fb, kb]), (d, fa, ka)
            # the top-right quadrant becomes the bottom-left one, which the fork does not emit: only its mean can be rebuilt
            assert np.array_equal(2 * A[:, :, fa, 3] - A[:, :, fa, 21], sign * B[:, :, fb, 19]), (d, fa)


@pytest.mark.parametrize("w,h", FC.SIZES)
def test_triangle_variance_is_floor_of_abs_mean(w, h):
    want = FC.case(w, h, "textured")[3].astype(np.float64)
    off = FR.level_offsets(w, h)
    for d in range(4):
        half = (64 >> d) ** 2 // 2
        rows = want[off[d]:off[d + 1], :FR.TMV].reshape(-1, 5, 26)
        for km, kv in ((10, 12), (11, 13), (14, 16), (15, 17)):
            assert np.array_equal(rows[:, :, kv], np.floor(np.abs(rows[:, :, km])) / half)
        assert np.array_equal(rows[:, :, 20], rows[:, :, 3]) and np.array_equal(rows[:, :, 24], rows[:, :, 5])


def _soc_levels(soc, w, h):
    off = FR.level_offsets(w, h)
    return [soc[off[d]:off[d + 1]].reshape(bh, bw, 16).astype(np.int64) for d, (bh, bw) in enumerate(FR.level_shapes(w, h))]


@pytest.mark.parametrize("w,h", FC.SIZES)
def test_soc_of_a_level_is_the_sum_of_its_children(w, h):
    lv = _soc_levels(FC.case(w, h, "textured")[3][:, FR.TMV:], w, h)
    n = 0
    for d in range(3):
        s = 64 >> d
        for by in range(h // s):                               # the blocks wholly inside
            for bx in range(w // s):
                assert np.array_equal(lv[d][by, bx], lv[d + 1][2 * by:2 * by + 2, 2 * bx:2 * bx + 2].sum(axis=(0, 1)))
                n += 1
    assert n > 0 or min(w, h) < 16
    assert not any(l[:, :, 0].any() for l in lv)              # DC


@pytest.mark.parametrize("w,h", FC.SIZES)
def test_soc_is_zero_where_n_obf_is_zero(w, h):
    """N_OBF from the oracle's OBF map, as tests/test_obf.py takes it: a block without an outlier block has no outlier coefficient"""
    # (8x8: the flat picture, whose fit is quick -- features_cases.case)
    Y, yc, _, want, _ = FC.case(w, h, "textured" if w * h >= 64 * 64 else "flat")
    obf, yc2 = hmo_py.obf_prepass(Y)
    assert np.array_equal(yc, yc2)
    lv = _soc_levels(want[:, FR.TMV:], w, h)
    zero = some = 0
    for d in range(4):
        s = 64 >> d
        for by in range(h // s):
            for bx in range(w // s):
                n_obf = int((obf[by * s // 4:(by + 1) * s // 4, bx * s // 4:(bx + 1) * s // 4] > 0).sum())
                if n_obf == 0:
                    assert not lv[d][by, bx].any()
                    zero += 1
                elif lv[d][by, bx].any():
                    some += 1
    assert some > 0
    # the restated DCT is the oracle's leaf-pinned transform
    lo = hmo_py.load()
    blk, coef = np.zeros(16, np.int16), np.zeros(16, np.int32)
    mine = FR.dct4_blocks(Y)
    for by, bx in ((0, 0), (h // 4 - 1, w // 4 - 1), (h // 8, w // 8)):
        blk[:] = Y[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4].astype(np.int16).ravel()
        lo.hmo_fwd_transform(C.c_void_p(blk.ctypes.data), 4, C.c_void_p(coef.ctypes.data), 2, 0)
        assert np.array_equal(mine[by, bx], coef)


def test_soc_with_zero_thresholds_counts_every_nonzero_ac_coefficient():
    w, h = 72, 200
    Y = FC.case(w, h, "textured")[0]
    soc = FR.feature_maps(Y, ("soc",), np.zeros(16))
    c = np.abs(FR.dct4_blocks(Y)) // 100
    c[:, :, 0] = 0
    lv = _soc_levels(soc, w, h)
    assert np.array_equal(lv[3][:h // 8, :w // 8], c.reshape(h // 8, 2, w // 8, 2, 16).sum(axis=(1, 3)))
    assert lv[3].sum() == c.sum() and lv[3].sum() > 0


# ---- refusals and names -------------------------------------------------------------------------------------------------------

def test_refusals_name_the_argument(built):
    """features_args_check of fcu_host.h: the code and text fcu_feature_maps returns"""
    L = lib()
    Y = np.ascontiguousarray(FC.case(64, 64, "flat")[0])
    ys, hole = (C.c_void_p * 1)(Y.ctypes.data), (C.c_void_p * 1)(None)
    yc = np.zeros(16, np.float64)
    out = at_offset(np.zeros(85 * 146 * 4, np.uint8), 0)
    p = out.ctypes.data
    err = lambda: L.features_emu_last_error().decode()
    call = lambda n, sets, y, t, o: L.features_emu(64, 64, n, sets, y, t, o)
    assert call(1, 3, ys, yc.ctypes.data, p) == 0 and call(1, 1, ys, None, p) == 0 and call(1, 2, ys, yc.ctypes.data, p) == 0
    assert call(0, 3, ys, yc.ctypes.data, p) == ARG and "n_pics" in err()
    assert call(1, 0, ys, None, p) == ARG and "sets" in err()
    assert call(1, 4, ys, None, p) == ARG and "sets" in err()
    assert call(1, 7, ys, yc.ctypes.data, p) == ARG and "sets" in err()
    assert call(1, 1, None, None, p) == ARG and "dev_y is null" in err()
    assert call(1, 1, hole, None, p) == ARG and "dev_y[0]" in err()
    assert call(1, 2, ys, None, p) == ARG and "host_yc is null" in err()
    assert call(1, 1, ys, yc.ctypes.data, p) == ARG and "host_yc is given" in err()
    assert call(1, 1, ys, None, None) == ARG and "dev_features is null" in err()
    for k in (1, 2, 3):
        assert call(1, 1, ys, None, p + k) == ARG and "dev_features" in err() and "4" in err()
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        yb = yc.copy()
        yb[5] = bad
        assert call(1, 3, ys, yb.ctypes.data, p) == ARG and "host_yc[0][5]" in err()
    assert [L.features_emu_count(s) for s in (1, 2, 3)] == [130, 16, 146] and [L.features_emu_count(s) for s in (0, 4, 5, -1)] == [ARG] * 4


def test_feature_names(pkg):
    e = pkg.engine
    assert len(e.FEATURE_NAMES) == 146 and len(set(e.FEATURE_NAMES)) == 146
    assert e.FEATURE_NAMES[1 * 26 + 4] == "tmv_hor_var_top" and e.FEATURE_NAMES[130 + 5] == "soc_5" and e.FEATURE_NAMES[0] == "tmv_org_mean_all"
    assert e.FEATURE_NAMES[4 * 26 + 25] == "tmv_antd_var_q_br" and e.FEATURE_NAMES[2 * 26 + 20] == "tmv_ver_mean_q_bottom"
    assert e.feature_columns(("tmv", "soc")) == e.FEATURE_NAMES and e.feature_columns(("soc", "tmv")) == e.FEATURE_NAMES
    assert e.feature_columns("tmv") == e.FEATURE_NAMES[:130] and e.feature_columns(("soc",)) == e.FEATURE_NAMES[130:]
    with pytest.raises(ValueError):
        e.feature_columns(("tmv", "obf"))
    assert (e.FEATURE_SETS, e.FEATURE_COUNTS) == ({"tmv": 1, "soc": 2}, {"tmv": FR.TMV, "soc": FR.SOC})


def test_library_exports_the_entry_points(built, pkg):
    L = pkg.load_lib()
    assert [L.fcu_feature_count(s) for s in (1, 2, 3)] == [130, 16, 146] and L.fcu_feature_count(0) == ARG and L.fcu_feature_count(4) == ARG
    assert L.fcu_feature_maps(None, 1, 3, None, None, None, None, None) == ARG and b"fcu_feature_maps" in L.fcu_last_error()


def test_driver_keeps_its_keys_without_the_option(pkg):
    import inspect
    assert inspect.signature(pkg.sequence.SequenceDecider.__init__).parameters["features"].default is None
    assert "feature_maps" in dir(pkg.CuEngine)
