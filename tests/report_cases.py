"""Inputs of the picture-report tests, shared by the emulator tests (test_report.py) and the GPU tests (test_gpu_report.py):
seeded planes and fcu_ctu_out records, with the numpy reference (report_ref.py) computed once per case."""
import functools

import numpy as np

import report_ref

HEAD_BYTES = 32 * 256                  # the per-partition arrays in front of the coefficients
# 64x64: one full CTU; 72x40: a partial CTU in both directions, chroma stride 36; 136x72: 3 x 2 CTUs, the last column 8 wide
# and the last row 8 high; 320x256: 5 x 4 full CTUs; 176x88: 3 x 2 CTUs whose partial column (48) and row (24) still allow the
# wide loads; 128x64: two full CTUs (the size of the misaligned-plane test)
SIZES = [(64, 64), (72, 40), (136, 72), (320, 256), (176, 88), (128, 64)]


def _pkg():
    import __graft_entry__ as g
    return g.load_package()


def aligned(a, offset=0):
    """a copy of the uint8 array `a` whose first byte sits `offset` bytes past a 16-byte boundary"""
    buf = np.zeros(a.size + 32, np.uint8)
    start = (-buf.ctypes.data) % 16 + offset
    v = buf[start:start + a.size].reshape(a.shape)
    v[...] = a
    assert v.ctypes.data % 16 == offset % 16
    return v


def planes(w, h, seed, kind="noise"):
    """(org, rec): two (Y, U, V) triples of uint8 arrays on 16-byte boundaries"""
    rng = np.random.default_rng(seed)
    shapes = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    if kind == "saturated":                                   # every sample at the largest error: org 0, rec 255
        return [aligned(np.zeros(s, np.uint8)) for s in shapes], [aligned(np.full(s, 255, np.uint8)) for s in shapes]
    org = [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]
    rec = [np.clip(o.astype(np.int32) + rng.integers(-40, 41, o.shape), 0, 255).astype(np.uint8) for o in org]
    return [aligned(o) for o in org], [aligned(r) for r in rec]


def inside_mask(w, h):
    """bool [n_ctu, 256]: is 4x4 partition z of CTU a inside a w x h picture"""
    w_ctu, h_ctu = (w + 63) // 64, (h + 63) // 64
    xy = [report_ref.z_to_xy(z) for z in range(256)]
    return np.array([[(a % w_ctu) * 64 + 4 * x < w and (a // w_ctu) * 64 + 4 * y < h for x, y in xy] for a in range(w_ctu * h_ctu)])


def records(w, h, seed, outside_seed=None):
    """fcu_ctu_out records [n_ctu, sizeof] whose head bytes are random over their full range (part_size 8..255, pred_mode 2,
    depth > 3 among them: values that must be counted nowhere), total_bits near 2^32 - 1 (the picture sum passes 32 bits from the
    second CTU on), total_bins / total_dist random.  outside_seed: the entries of partitions outside the picture are drawn
    again from that seed -- they must not influence any count."""
    e = _pkg().engine
    rng = np.random.default_rng(seed)
    n_ctu = ((w + 63) // 64) * ((h + 63) // 64)
    r = np.zeros((n_ctu, e.CTU_OUT_BYTES), np.uint8)
    r[:, :HEAD_BYTES] = rng.integers(0, 256, (n_ctu, HEAD_BYTES), dtype=np.uint8)
    # bias some arrays towards the values that ARE counted, so that every counter sees hits as well as misses
    lo = rng.integers(0, 256, (n_ctu, 256)) < 160
    for name, top in (("depth", 6), ("part_size", 10), ("pred_mode", 3)):
        o = getattr(e.CtuOut, name).offset
        r[:, o:o + 256] = np.where(lo, rng.integers(0, top, (n_ctu, 256)), r[:, o:o + 256]).astype(np.uint8)
    tot = np.stack([rng.integers(0, 1 << 32, n_ctu), (1 << 32) - 1 - rng.integers(0, 1 << 20, n_ctu), rng.integers(0, 1 << 32, n_ctu)], 1).astype("<u4")
    o = e.CtuOut.total_dist.offset
    r[:, o:o + 12] = tot.view(np.uint8).reshape(n_ctu, 12)
    if outside_seed is not None:
        rng2 = np.random.default_rng(outside_seed)
        out = ~inside_mask(w, h)
        head = r[:, :HEAD_BYTES].reshape(n_ctu, 32, 256)
        other = rng2.integers(0, 256, head.shape, dtype=np.uint8)
        head[...] = np.where(out[:, None, :] & (np.arange(32) < 24)[None, :, None], other, head)      # the 24 byte-per-partition arrays
    return r


@functools.lru_cache(maxsize=None)
def case(w, h, seed, kind="noise"):
    """(org, rec, records, reference picture report, reference CTU records) -- computed once, never modified"""
    org, rec = planes(w, h, seed, kind)
    r = records(w, h, seed + 1000)
    pic, ctu = report_ref.picture_report(_pkg(), org, rec, r)
    for a in org + rec + [r, ctu]:
        a.setflags(write=False)
    return org, rec, r, pic, ctu
