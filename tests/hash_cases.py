"""Inputs of the picture-hash tests, shared by the emulator tests (test_hash.py) and the GPU tests (test_gpu_hash.py): seeded
planes placed as report_cases.aligned places them, with the reference (hash_ref.py) computed once per case."""
import ctypes as C
import functools
import os

import numpy as np

import hash_ref
from report_cases import aligned

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASKS = {"md5": 1, "crc": 2, "checksum": 4}


def emu_lib():
    L = C.CDLL(os.path.join(ROOT, "tests", "emu", "libhash_emu.so"))
    L.hash_emu.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    L.hash_emu_plane.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_void_p]
    L.hash_emu_md5.argtypes = [C.c_char_p, C.c_ulonglong, C.c_void_p]
    L.hash_emu_md5.restype = None
    L.hash_emu_string.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int]
    return L


def chunk():
    """bytes of a plane one workgroup of the first kernel folds (HASH_CHUNK of csrc/fcu_hash.h)"""
    return emu_lib().hash_emu_chunk()


# 8x8: luma exactly one MD5 block, chroma 16 bytes; 24x8: chroma 48 bytes, luma 192; 16x16: chroma exactly 64 bytes; 72x40 and
# 176x88: chroma lengths 16 and 32 mod 64, chroma stride no multiple of 16; 320x264: x and y pass 255 (both high terms of the mask)
FIXED = [(8, 8), (24, 8), (16, 16), (72, 40), (176, 88), (320, 264)]


def chunk_sizes():
    """the three cases in which the fold's lengths differ, from the chunk constant (16 KiB: 64x64, 256x128, 264x128), and one
    plane of more than 256 chunks, so that the second kernel's threads fold more than one partial each (2048x2056)"""
    c = chunk()
    assert c % 4096 == 0
    short = (64, 64)                                          # every plane shorter than one chunk
    exact = (c // 64, 128)                                    # luma = 2 chunks exactly, chroma = half a chunk
    tail = (c // 64 + 8, 128)                                 # luma = 2 chunks + 1024 bytes, chroma = 8448 bytes
    rows = (256 * c) // 2048 + 1
    many = (2048, (rows + 7) // 8 * 8)                        # luma just past 256 chunks, chroma past 64
    assert 64 * 64 < c and exact[0] * exact[1] == 2 * c and 0 < tail[0] * tail[1] - 2 * c < c and many[0] * many[1] > 256 * c
    return [short, exact, tail, many]


def sizes():
    return FIXED + chunk_sizes()


def planes(w, h, seed, kind="noise"):
    """(Y, U, V) uint8 arrays on 16-byte boundaries"""
    shapes = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    if kind == "zero":
        return [aligned(np.zeros(s, np.uint8)) for s in shapes]
    if kind == "ones":
        return [aligned(np.full(s, 255, np.uint8)) for s in shapes]
    rng = np.random.default_rng(seed)
    return [aligned(rng.integers(0, 256, s, dtype=np.uint8)) for s in shapes]


@functools.lru_cache(maxsize=None)
def case(w, h, seed, kind="noise"):
    """(planes, reference dict of all three kinds) -- computed once, never modified"""
    p = planes(w, h, seed, kind)
    for a in p:
        a.setflags(write=False)
    return p, hash_ref.picture(p)


# (w, h, seed, content): noise at every size; all-zero (every CRC partial is 0) and all-255 where the lengths of the fold differ
def all_cases():
    cs = [(w, h, 11, "noise") for w, h in sizes()]
    for w, h in [(8, 8), (72, 40)] + chunk_sizes()[:3]:
        cs += [(w, h, 0, "zero"), (w, h, 0, "ones")]
    return cs


def wrap_plane():
    """4096x4160 luma of 255 ^ mask: every term of the checksum is 255 and the sum 255 * 17 039 360 passes 2^32"""
    w, h = 4096, 4160
    return aligned(255 ^ hash_ref.checksum_mask(w, h)), (255 * w * h) & 0xffffffff


def select(ref, kinds):
    """the reference restricted to `kinds`, as CuEngine.picture_hash returns it"""
    d = {k: ref[k] for k in kinds}
    d["line"] = {k: ref["line"][k] for k in kinds}
    return d
