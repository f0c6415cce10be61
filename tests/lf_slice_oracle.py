"""Reference for the loop filters of a picture of SliceMode 1 slices (LFCrossSliceBoundaryFlag 0 and 1), what the CPU tests
(tests/test_lf_slices.py) and the GPU tests (tests/test_gpu_lf_slices.py) share: the reference itself, the ctypes binding of the
emulator driver (tests/emu/lf_slices_emu.cpp), and the cases with their references computed once.

The reference is tests/emu/lf_slice_ref.c: oracle/hmo_deblock.c's hmo_deblock_pic and oracle/hmo_sao.c's hmo_sao_picture with the
slice rules of the flag 0 added and every function below them the oracle's own --
  deblocking   a partition on the left / top edge of its CTU gets no edge flag when the CTU to the left / above lies in another
               slice (TComLoopFilter.cpp:369-411, getPULeft / getPUAbove), as on the picture border;
  offset pass  a neighbour CTU is available iff it is inside the picture and in the CTU's slice, eight directions of their own
               (TComPicSym.cpp:357-447, TComSampleAdaptiveOffset.cpp:577);
  statistics   left, above and above-left by that rule, right and below -- with the margins they skip -- by the picture border
               (TEncSampleAdaptiveOffset.cpp:327-336);
  decision     unchanged: merge candidates inside the slice, the walk and the coder across slices.

Not pinned by an HM run: no run of HM with slices and LFCrossSliceBoundaryFlag 0 has recorded results to compare with, and the
recorded goldens cannot be extended.  The reference rests on reading the HM lines cited.  What pins it instead, each point a test
of tests/test_lf_slices.py:
  1. one slice, or the flag 1, equals hmo_py.deblock_pic / hmo_py.sao_picture, which the HM goldens pin;
  2. slices of whole CTU rows with the flag 0: deblocking equals the unchanged oracle on every slice's crop, pasted
     (deblock_stitched); and the crop's statistics (hmo_py.sao_picture(..., want_stats=True) on the crop of the deblocked picture)
     equal the picture's for every CTU that is not in the last CTU row of its slice, and for the picture's last CTU row: there
     left / above / above-left of the crop are the slice's and right / below are the picture border in both.  The last CTU row of
     a slice that is not the picture's last has the picture border below it in the crop and a CTU row in the picture -- the
     statistics keep `below` at the picture border -- and is not compared;
  3. slice independence with the flag 0, the definition of the flag, for every slice of every slice length of the cases: with the
     samples outside the slice replaced by seeded random bytes, the deblocked samples inside it, the statistics of its CTUs and,
     with the SAO parameters held fixed, the offset-pass output inside it do not change.  This pins the staircase diagonals;
  4. locality: the flag changes deblocked samples only within 4 luma / 2 chroma samples (Chebyshev) of the slice boundary line;
  5. the offset pass against the specification's rule sample by sample (sao_apply_spec below, plain numpy, no eight flags): a
     sample keeps its value when either neighbour along its edge class lies outside the picture or in another slice;
  6. with the diagonals set to the conjunctions of their sides, the eight-flag block functions of lf_slice_ref.c reproduce the
     oracle's four-flag ones."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import hmo_py
from tile_oracle import CTU_BYTES

_HERE = os.path.dirname(os.path.abspath(__file__))
_P = C.c_void_p
SHIFT = (0, 1, 1)


def dims(w, h):
    return (w + 63) // 64, (h + 63) // 64


def slice_len(n, slice_ctus):
    return n if slice_ctus <= 0 or slice_ctus > n else slice_ctus


def slice_ranges(w, h, slice_ctus):
    """[(first, end)] CTU address ranges of the slices"""
    W, H = dims(w, h)
    S = slice_len(W * H, slice_ctus)
    return [(a, min(a + S, W * H)) for a in range(0, W * H, S)]


def slice_map(w, h, slice_ctus, comp):
    """slice index of every sample of a plane"""
    W, H = dims(w, h)
    S, s = slice_len(W * H, slice_ctus), SHIFT[comp]
    ys, xs = np.mgrid[0:h >> s, 0:w >> s]
    return (((ys << s) // 64) * W + ((xs << s) // 64)) // S


# ---- the reference ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_lib():
    lib = C.CDLL(os.path.join(_HERE, "emu", "liblf_slice_ref.so"))
    lib.lf_ref_deblock_slices.argtypes = [_P, C.c_int, C.c_int, _P, _P, _P] + [C.c_int] * 4
    lib.lf_ref_sao_slices.argtypes = [C.c_int] * 6 + [_P] * 8
    lib.lf_ref_sao_apply_slices.argtypes = [C.c_int] * 4 + [_P, _P]
    lib.lf_ref_slice_avail8.argtypes = [C.c_int] * 4 + [_P]
    lib.lf_ref_blk_stats4.argtypes = [_P, _P, _P] + [C.c_int] * 8
    lib.lf_ref_blk_stats8.argtypes = [_P, _P, _P] + [C.c_int] * 9
    lib.lf_ref_offset_block4.argtypes = [C.c_int, _P, _P, _P] + [C.c_int] * 7
    lib.lf_ref_offset_block8.argtypes = [C.c_int, _P, _P, _P] + [C.c_int] * 3 + [_P]
    for f in ("lf_ref_deblock_slices", "lf_ref_sao_slices", "lf_ref_sao_apply_slices", "lf_ref_slice_avail8", "lf_ref_blk_stats4", "lf_ref_blk_stats8",
              "lf_ref_offset_block4", "lf_ref_offset_block8"):
        getattr(lib, f).restype = None
    return lib


def deblock_slices(ctus, w, h, rec, slice_ctus, cross):
    """new planes: rec deblocked with LFCrossSliceBoundaryFlag = cross"""
    buf = np.frombuffer(ctus, np.uint8).copy()
    out = [np.ascontiguousarray(p).copy() for p in rec]
    ref_lib().lf_ref_deblock_slices(buf.ctypes.data, w, h, *[p.ctypes.data for p in out], 0, 0, int(slice_ctus), int(cross))
    return out


def sao_slices(org, rec, qp, slice_type, lam, slice_ctus, cross, enabled=(1, 1, 1)):
    """hmo_py.sao_picture with LFCrossSliceBoundaryFlag = cross: in place on `rec`; returns (params int32 [n_ctu, 3, 35],
    off_count[3], stats int64 [n_ctu, 3, 2, 5, 32], reconstructed parameters int32 [n_ctu, 3, 35])"""
    h, w = org[0].shape
    n = np.prod(dims(w, h))
    for a in list(org) + list(rec):
        assert a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"]
    po = (C.c_void_p * 3)(*[a.ctypes.data for a in org])
    pr = (C.c_void_p * 3)(*[a.ctypes.data for a in rec])
    lams = (C.c_double * 3)(*hmo_py.slice_lambdas(qp, lam))
    en = (C.c_int * 3)(*[int(v) for v in enabled])
    params, recon = np.zeros((n, 3, 35), np.int32), np.zeros((n, 3, 35), np.int32)
    stats = np.zeros((n, 3, 2, 5, 32), np.int64)
    off = (C.c_int * 3)()
    ref_lib().lf_ref_sao_slices(w, h, int(slice_ctus), int(cross), qp, slice_type, C.cast(lams, _P), C.cast(en, _P), C.cast(po, _P), C.cast(pr, _P),
                                params.ctypes.data, stats.ctypes.data, C.cast(off, _P), recon.ctypes.data)
    return params, list(off), stats, recon


def sao_apply_slices(rec, recon, slice_ctus, cross):
    """the offset pass alone with the reconstructed parameters `recon` (int32 [n_ctu, 3, 35]); returns new planes"""
    h, w = rec[0].shape
    out = [np.ascontiguousarray(p).copy() for p in rec]
    pr = (C.c_void_p * 3)(*[a.ctypes.data for a in out])
    recon = np.ascontiguousarray(recon, np.int32)
    ref_lib().lf_ref_sao_apply_slices(w, h, int(slice_ctus), int(cross), recon.ctypes.data, C.cast(pr, _P))
    return out


def slice_avail8(a, w, h, slice_ctus):
    """dict L, R, A, B, AL, AR, BL, BR of CTU a with the flag 0"""
    v = (C.c_int * 8)()
    ref_lib().lf_ref_slice_avail8(a, *dims(w, h), int(slice_ctus), v)
    return dict(zip(("L", "R", "A", "B", "AL", "AR", "BL", "BR"), [int(x) for x in v]))


EO_STEP = ((1, 0), (0, 1), (1, 1), (-1, 1))                    # (dx, dy) of the second neighbour of EO_0, EO_90, EO_135, EO_45; the first is its opposite


def sao_apply_spec(rec, recon, slice_ctus, cross):
    """The specification's SAO sample process (H.265 8.7.5.2) on whole planes in numpy, no eight flags: edgeIdx stays 0 -- the
    sample keeps its value -- when the sample at either location (x + hPos[k], y + vPos[k]) lies outside the picture or in a
    different slice (with the flag 1: outside the picture); else the offset of 2 + sign(c - a) + sign(c - b).  Band offset: every
    sample.  recon: reconstructed parameters int32 [n_ctu, 3, 35] (mode 0 = off).  Returns new planes."""
    h, w = rec[0].shape
    W, _ = dims(w, h)
    out = []
    for comp, src in enumerate(rec):
        s = SHIFT[comp]
        ph, pw = src.shape
        ys, xs = np.mgrid[0:ph, 0:pw]
        ctu = ((ys << s) // 64) * W + ((xs << s) // 64)
        sl = slice_map(w, h, slice_ctus, comp) if not cross else np.zeros((ph, pw), np.int64)
        mode, typ, offs = recon[ctu, comp, 0], recon[ctu, comp, 1], recon[:, comp, 3:]
        c = src.astype(np.int32)
        pad = np.pad(c, 1, mode="edge")
        pads = np.pad(sl, 1, mode="constant", constant_values=-1)           # outside the picture: no slice
        res = c.copy()
        for t, (dx, dy) in enumerate(EO_STEP):
            a, b = pad[1 - dy:1 - dy + ph, 1 - dx:1 - dx + pw], pad[1 + dy:1 + dy + ph, 1 + dx:1 + dx + pw]
            sa, sb = pads[1 - dy:1 - dy + ph, 1 - dx:1 - dx + pw], pads[1 + dy:1 + dy + ph, 1 + dx:1 + dx + pw]
            k = 2 + np.sign(c - a) + np.sign(c - b)
            ok = (mode != 0) & (typ == t) & (sa == sl) & (sb == sl)
            res = np.where(ok, c + offs[ctu, k], res)
        res = np.where((mode != 0) & (typ == 4), c + offs[ctu, c >> 3], res)
        out.append(np.clip(res, 0, 255).astype(np.uint8))
    return out


def crop_rows(planes, y0, y1, h):
    """CTU rows [y0, y1) of the planes (a copy)"""
    return [p[(y0 * 64) >> s:min(y1 * 64, h) >> s].copy() for p, s in zip(planes, SHIFT)]


def deblock_stitched(ctus, w, h, rec, slice_ctus):
    """slices of whole CTU rows, the flag 0: every slice's crop deblocked on its own by the unchanged oracle, pasted"""
    W, _ = dims(w, h)
    assert slice_ctus % W == 0
    out = [p.copy() for p in rec]
    for first, end in slice_ranges(w, h, slice_ctus):
        part = crop_rows(rec, first // W, end // W, h)
        hmo_py.deblock_pic(ctus[first * CTU_BYTES:end * CTU_BYTES], w, part[0].shape[0], part)
        for p, q, s in zip(out, part, SHIFT):
            p[(first // W * 64) >> s:((first // W * 64) >> s) + q.shape[0]] = q
    return out


def randomised_outside(planes, w, h, slice_ctus, s, seed):
    """copies of the planes with every sample outside slice s replaced by seeded random bytes"""
    rng = np.random.default_rng(seed)
    out = []
    for comp, p in enumerate(planes):
        m = slice_map(w, h, slice_ctus, comp) == s
        out.append(np.where(m, p, rng.integers(0, 256, p.shape, dtype=np.uint8)).astype(np.uint8))
    return out


def all_new_params(n, typ, seed):
    """reconstructed parameters that switch every CTU and component to type `typ` (0..3 edge classes, 4 band offset)"""
    rng = np.random.default_rng(seed)
    r = np.zeros((n, 3, 35), np.int32)
    r[:, :, 0], r[:, :, 1] = 1, typ
    if typ == 4:
        band = rng.integers(0, 32, (n, 3))
        r[:, :, 2] = band
        for i in range(4):
            np.put_along_axis(r[:, :, 3:], ((band + i) % 32)[..., None], rng.integers(-7, 8, (n, 3, 1)), axis=2)
    else:
        r[:, :, 3:5] = rng.integers(1, 8, (n, 3, 2))
        r[:, :, 6:8] = -rng.integers(1, 8, (n, 3, 2))
    return r


def params_to_sao_ctu(recon):
    """int32 [n, 3, 35] -> the fcu_sao_ctu array as uint8 [n, 108]"""
    n = recon.shape[0]
    a = np.zeros((n, 3, 36), np.int8)
    a[:, :, :3], a[:, :, 4:] = recon[:, :, :3], recon[:, :, 3:]
    return np.ascontiguousarray(a.view(np.uint8).reshape(n, 108))


# ---- the emulator driver ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def load_emu():
    lib = C.CDLL(os.path.join(_HERE, "emu", "liblf_slices_emu.so"))
    lib.lf_slices_emu_variant.argtypes = [C.c_int] * 4 + [_P]
    lib.lf_slices_emu_deblock.argtypes = [_P] * 4 + [C.c_int] * 6
    lib.lf_slices_emu_sao.argtypes = [C.c_int] * 4 + [_P, _P] + [C.c_int] * 2 + [_P] * 10
    lib.lf_slices_emu_apply.argtypes = [C.c_int] * 4 + [_P] * 4
    return lib


@pytest.fixture(scope="session")
def lf_emu(built):
    return load_emu()


def emu_deblock(lib, ctus, w, h, rec, slice_ctus, cross):
    """new planes"""
    buf = np.frombuffer(ctus, np.uint8).copy()
    out = [np.ascontiguousarray(p).copy() for p in rec]
    assert lib.lf_slices_emu_deblock(buf.ctypes.data, *[a.ctypes.data for a in out], w, h, 0, 0, int(slice_ctus), int(cross)) == 1
    return out


def emu_sao(lib, org, rec, qp, slice_type, lam, slice_ctus, cross, enabled=(1, 1, 1)):
    """in place on rec; returns (coded uint8 [n, 108], off_count int32 [3], stats int64 in the reference's layout [n, 3, 2, 5, 32])"""
    h, w = org[0].shape
    n = np.prod(dims(w, h))
    lams, en = np.array(hmo_py.slice_lambdas(qp, lam), np.float64), np.array(enabled, np.int32)
    coded, off = np.zeros((n, 108), np.uint8), np.zeros(3, np.int32)
    stats = np.zeros((n, 3, 5, 2, 32), np.int32)
    assert lib.lf_slices_emu_sao(w, h, slice_type, qp, lams.ctypes.data, en.ctypes.data, int(slice_ctus), int(cross), *[a.ctypes.data for a in org],
                                 *[a.ctypes.data for a in rec], coded.ctypes.data, off.ctypes.data, stats.ctypes.data, None) == 1
    return coded, off, np.ascontiguousarray(stats.astype(np.int64).transpose(0, 1, 3, 2, 4))


def emu_apply(lib, rec, recon, slice_ctus, cross):
    """the offset pass alone; returns new planes"""
    h, w = rec[0].shape
    out = [np.ascontiguousarray(p).copy() for p in rec]
    r = params_to_sao_ctu(recon)
    assert lib.lf_slices_emu_apply(w, h, int(slice_ctus), int(cross), r.ctypes.data, *[a.ctypes.data for a in out]) == 1
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------------
# 208 x 136 = 4 x 3 CTUs whose last column (16 samples) and last row (8 samples) are partial: the picture of the tile cases.
# slice_ctus 4: every row a slice; 8: two rows plus one; 5: a staircase {0-4 | 5-9 | 10, 11} -- CTUs 9, 8, 6 and 5 are the four
# cases in which a diagonal is not the conjunction of its sides (AL, AR, BL, BR); 3: slices starting at columns 3, 2, 1; 1: every
# CTU a slice; 12 and 0: one slice.
W, H = 208, 136
N_CTU = 12
CUTS = (4, 8, 5, 3, 1)                                         # more than one slice
ONE = (12, 0)                                                  # one slice
ROW_CUTS = (4, 8)                                              # slices of whole CTU rows
P_CUTS = (5, 4)                                                # the slice lengths the P picture is decided with
QP, CONTENT, SEED = 32, "textured", 7
LAMBDA = 0.57 * 2.0 ** ((QP - 12) / 3.0)
SLICE_TYPES = (hmo_py.SLICE_I, hmo_py.SLICE_P)                 # the slice type SAO is told: the initial state of its two contexts


def frame(pkg):
    return [np.ascontiguousarray(a) for a in getattr(pkg.synth, CONTENT)(W, H, seed=SEED)]


class Decided:
    """a decided picture: ctus (bytes of the Ctu array), rec (planes before the loop filters), the frame"""

    def __init__(self, enc, f):
        enc.compress_frame()
        self.ctus, self.rec, self.frame = enc.all_ctus_bytes(), [p.copy() for p in enc.rec], f
        enc.close()


@functools.lru_cache(maxsize=None)
def decided(pkg, slice_ctus):
    """the picture decided by the oracle as an I picture of slices of slice_ctus CTUs"""
    f = frame(pkg)
    return Decided(hmo_py.Encoder(*f, QP, slice_ctus=slice_ctus), f)


@functools.lru_cache(maxsize=None)
def decided_p(pkg, slice_ctus):
    """one P picture referencing the I picture's reconstruction: every CTU shows the I frame moved by a vector of its own (and a
    little noise), so that neighbouring CTUs differ in motion and boundary strengths from motion and from coded residuals occur at
    the slice edges"""
    src, rng = frame(pkg), np.random.default_rng(11)
    f = [p.copy() for p in src]
    Wc, Hc = dims(W, H)
    for cy in range(Hc):
        for cx in range(Wc):
            dx, dy = 2 * (((cx * 3 + cy * 5) % 5) - 2), 2 * (((cx * 2 + cy * 3) % 3) - 1)
            for p, q, s in zip(f, src, SHIFT):
                y0, x0 = (cy * 64) >> s, (cx * 64) >> s
                p[y0:y0 + (64 >> s), x0:x0 + (64 >> s)] = np.roll(q, (dy >> s, dx >> s), axis=(0, 1))[y0:y0 + (64 >> s), x0:x0 + (64 >> s)]
    f[0] = np.clip(f[0].astype(np.int16) + rng.integers(-2, 3, f[0].shape), 0, 255).astype(np.uint8)
    f = [np.ascontiguousarray(p) for p in f]
    _, qp, lam = hmo_py.ldp_slice(1, QP)
    return Decided(hmo_py.Encoder(*f, qp, slice_ctus=slice_ctus, ref=decided(pkg, slice_ctus).rec, lambda_override=lam, search_range=8, fast_search=1), f)


@functools.lru_cache(maxsize=None)
def filtered(pkg, slice_ctus, cross, slice_type, enabled=(1, 1, 1)):
    """decide -> deblock -> SAO by the reference: dict dbk (planes after deblocking), params, off, stats, recon, rec (after SAO)"""
    d = decided(pkg, slice_ctus)
    dbk = deblock_slices(d.ctus, W, H, d.rec, slice_ctus, cross)
    rec = [p.copy() for p in dbk]
    params, off, stats, recon = sao_slices(d.frame, rec, QP, slice_type, LAMBDA, slice_ctus, cross, enabled=enabled)
    return dict(dbk=dbk, params=params, off=off, stats=stats, recon=recon, rec=rec)
