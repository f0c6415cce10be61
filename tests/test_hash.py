"""The picture-hash kernels (csrc/fcu_hash.h: hash_chunk, hash_fold, hash_md5) on the CPU (tests/emu/hash_emu.cpp: the kernel source
with the HIP keywords defined away, every grid run as a loop) against tests/hash_ref.py (hashlib and the definitions of
TComPicYuvMD5.cpp): every digest byte, exact, for every case, kind, kind combination and both load paths."""
import ctypes as C
import hashlib
import inspect
import itertools

import numpy as np
import pytest

import hash_cases as HC
import hash_ref

KIND_SETS = [ks for n in (1, 2, 3) for ks in itertools.combinations(hash_ref.KINDS, n)]


def mask_of(kinds):
    return sum(HC.MASKS[k] for k in kinds)


def to_dict(rec, kinds):
    d = {k: [bytes(rec[k][c]).hex() for c in range(3)] for k in kinds}
    d["line"] = {k: ",".join(d[k]) for k in kinds}
    return d


def emu_hash(pkg, pictures, kinds=hash_ref.KINDS, wide=1, buf=None):
    """pictures: list of (Y, U, V).  Returns (PIC_HASH_DTYPE array [n], path taken: 1 = 16-byte loads)"""
    L = HC.emu_lib()
    n = len(pictures)
    h, w = pictures[0][0].shape
    ptr = (C.c_void_p * (3 * n))()
    for i, p in enumerate(pictures):
        for k in range(3):
            assert p[k].flags.c_contiguous and p[k].shape == ((h, w) if k == 0 else (h // 2, w // 2))
            ptr[3 * i + k] = p[k].ctypes.data
    out = np.zeros(n, pkg.engine.PIC_HASH_DTYPE) if buf is None else buf
    path = L.hash_emu(w, h, n, mask_of(kinds), wide, ptr, out.ctypes.data, None, 0)
    assert path in (0, 1)
    return out, path


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("w,h,seed,content", HC.all_cases())
def test_cases_on_both_load_paths(w, h, seed, content, wide, built, pkg):
    planes, ref = HC.case(w, h, seed, content)
    got, path = emu_hash(pkg, [planes], wide=wide)
    assert path == wide                                        # the planes sit on 16-byte boundaries
    assert to_dict(got[0], hash_ref.KINDS) == ref, (w, h, content, wide)
    assert not got[0]["pad"].any()


@pytest.mark.parametrize("kinds", KIND_SETS)
@pytest.mark.parametrize("w,h", [(72, 40), (264, 128)])
def test_kinds_and_combinations(w, h, kinds, built, pkg):
    """only the kinds asked for are computed; the fields of the others come back as zero, whatever the buffer held"""
    planes, ref = HC.case(w, h, 11)
    buf = np.frombuffer(b"\xaa" * pkg.engine.PIC_HASH_DTYPE.itemsize, pkg.engine.PIC_HASH_DTYPE).copy()
    got, _ = emu_hash(pkg, [planes], kinds, buf=buf)
    assert to_dict(got[0], kinds) == HC.select(ref, kinds)
    for k in hash_ref.KINDS:
        assert got[0][k].any() == (k in kinds), k
    assert not got[0]["pad"].any()


def test_all_zero_planes_differ_by_length_only(built, pkg):
    """every CRC partial of an all-zero plane is 0: only the initial state's term tells 64 zero bytes (8x8 luma) from 128 (16x8)"""
    for (w, h), want in (((8, 8), "d5b6"), ((16, 8), "b28b")):
        planes, ref = HC.case(w, h, 0, "zero")
        assert ref["crc"][0] == want
        got, _ = emu_hash(pkg, [planes], ("crc",))
        assert to_dict(got[0], ("crc",))["crc"] == ref["crc"] and ref["crc"][1] != want


@pytest.mark.parametrize("offset", [1, 4])
@pytest.mark.parametrize("w,h", [(72, 40), (264, 128)])
def test_planes_at_any_byte_offset(w, h, offset, built, pkg):
    planes, ref = HC.case(w, h, 11)
    got, path = emu_hash(pkg, [[HC.aligned(p, offset) for p in planes]])
    assert path == 0
    assert to_dict(got[0], hash_ref.KINDS) == ref, (w, h, offset)


def test_batch_of_three_equals_three_calls(built, pkg):
    cases = [HC.case(264, 128, s) for s in (11, 12, 13)]
    got, _ = emu_hash(pkg, [c[0] for c in cases])
    for i, c in enumerate(cases):
        one, _ = emu_hash(pkg, [c[0]])
        assert got[i].tobytes() == one[0].tobytes()
        assert to_dict(got[i], hash_ref.KINDS) == c[1]
    for k in hash_ref.KINDS:
        assert len({got[i][k].tobytes() for i in range(3)}) == 3, k


def test_second_call_gives_the_same_bytes(built, pkg):
    """nothing is accumulated into memory: a buffer full of stale bytes ends up the same as after a second call"""
    planes, ref = HC.case(264, 128, 11)
    buf = np.frombuffer(b"\xaa" * pkg.engine.PIC_HASH_DTYPE.itemsize, pkg.engine.PIC_HASH_DTYPE).copy()
    emu_hash(pkg, [planes], buf=buf)
    first = buf.tobytes()
    emu_hash(pkg, [planes], buf=buf)
    assert buf.tobytes() == first and to_dict(buf[0], hash_ref.KINDS) == ref


RFC1321 = {b"": "d41d8cd98f00b204e9800998ecf8427e", b"a": "0cc175b9c0f1b6a831c399e269772661", b"abc": "900150983cd24fb0d6963f7d28e17f72",
           b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789": "d174ab98d277d9f5a5611c2c9f419d9f",
           b"1234567890" * 8: "57edf4a22be3c955ac49da2e2107b67a"}


def test_md5_vectors_of_rfc_1321(built):
    L = HC.emu_lib()

    def md5(msg):
        out = C.create_string_buffer(16)
        L.hash_emu_md5(msg, len(msg), out)
        return out.raw.hex()

    assert [len(m) for m in RFC1321] == [0, 1, 3, 62, 80]
    for msg, want in RFC1321.items():
        assert md5(msg) == want == hashlib.md5(msg).hexdigest(), msg
    data = bytes(np.random.default_rng(1321).integers(0, 256, 200, dtype=np.uint8))
    for n in (55, 56, 63, 64, 65, 119, 120, 128, 200):        # the padding fits the last block up to 55 bytes, not from 56 on
        assert md5(data[:n]) == hashlib.md5(data[:n]).hexdigest(), n


def test_checksum_wraps_at_32_bits(built, pkg):
    """4096x4160 of 255 ^ mask: every term is 255 and the sum passes 2^32 (luma only, through the plane-level entry)"""
    plane, want = HC.wrap_plane()
    assert 255 * 4096 * 4160 > (1 << 32) and want == hash_ref.checksum(plane)
    L = HC.emu_lib()
    for wide in (0, 1):
        out = np.zeros(1, pkg.engine.PIC_HASH_DTYPE)
        assert L.hash_emu_plane(4096, 4160, HC.MASKS["checksum"] | HC.MASKS["crc"], wide, plane.ctypes.data, out.ctypes.data) == wide
        assert bytes(out[0]["checksum"][0]) == want.to_bytes(4, "big")
        assert bytes(out[0]["crc"][0]) == hash_ref.plane_digest(plane, "crc")      # 1040 chunks: every thread of the fold takes several


def test_hash_string_and_its_errors(built, pkg):
    e = pkg.engine
    planes, ref = HC.case(72, 40, 11)
    got, _ = emu_hash(pkg, [planes])
    L = HC.emu_lib()
    lib = C.CDLL(pkg.lib_path())
    lib.fcu_hash_string.argtypes = L.hash_emu_string.argtypes
    for f in (L.hash_emu_string, lib.fcu_hash_string):        # the emulator's entry and the library's: pure host code, no device
        for k in hash_ref.KINDS:
            buf = C.create_string_buffer(128)
            n = f(got.ctypes.data, HC.MASKS[k], buf, 128)
            assert n == len(ref["line"][k]) and buf.value.decode() == ref["line"][k]
            assert f(got.ctypes.data, HC.MASKS[k], buf, n + 1) == n and f(got.ctypes.data, HC.MASKS[k], buf, n) == -2
        for bad in (0, 3, 7, 8, -1):
            assert f(got.ctypes.data, bad, C.create_string_buffer(128), 128) == -2
    assert [len(ref["line"][k]) for k in hash_ref.KINDS] == [98, 14, 26]
    assert e.hash_string(got[0], "crc") == ref["line"]["crc"]
    assert e.hash_line("md5", "x") == hash_ref.line("md5", "x") == " [MD5:x]" and e.hash_line("checksum", "y") == " [Checksum:y]" and e.hash_line("crc", "z") == " [CRC:z]"


def test_hash_layout_matches_the_library(built, pkg):
    e = pkg.engine
    lib = C.CDLL(pkg.lib_path())
    assert lib.fcu_abi_sizeof(10) == C.sizeof(e.PicHash) == e.PIC_HASH_DTYPE.itemsize == 68
    for name, _ in e.PicHash._fields_:                       # no implicit padding: the numpy and ctypes offsets agree field by field
        assert getattr(e.PicHash, name).offset == e.PIC_HASH_DTYPE.fields[name][1], name
    assert [e.PIC_HASH_DTYPE.fields[n][1] for n in ("md5", "crc", "checksum", "pad")] == [0, 48, 54, 66]
    assert e.HASH_KINDS == HC.MASKS


def test_drivers_keep_their_keys_without_the_option(pkg):
    """pic_hash=None is the default of both drivers (the GPU tests check the result dicts)"""
    for cls in (pkg.lowdelay.LowDelayPDecider, pkg.sequence.SequenceDecider):
        assert inspect.signature(cls.__init__).parameters["pic_hash"].default is None
