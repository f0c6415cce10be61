"""The host arithmetic of the picture CRC (csrc/fcu_host.h: crc_mul, crc_xpow, crc_adv, the byte table, crc_bytes) on the CPU,
through the test-only driver tests/emu/hash_emu.cpp: the algebra in GF(2)[x] mod x^16 + x^12 + x^5 + 1 that the fold of the
kernels (csrc/fcu_hash.h) and the initial-state term 0xffff x^(8 n) of fcu_picture_hash rest on, against the bit-by-bit
definition of tests/hash_ref.py."""
import ctypes as C

import numpy as np
import pytest

import hash_cases as HC
import hash_ref


@pytest.fixture(scope="module")
def emu(built):
    L = HC.emu_lib()
    for name, args in (("crc_mul", [C.c_uint, C.c_uint]), ("crc_xpow", [C.c_ulonglong]), ("crc_adv", [C.c_uint, C.c_ulonglong]),
                       ("crc_bytes", [C.c_uint, C.c_char_p, C.c_ulonglong]), ("crc_digest", [C.c_char_p, C.c_ulonglong])):
        f = getattr(L, "hash_emu_" + name)
        f.argtypes, f.restype = args, C.c_uint
    return L


def shift_bits(s, bits):
    """the update of compCRC (TComPicYuvMD5.cpp:100-105) for a sequence of message bits"""
    for b in bits:
        s = (((s << 1) + b) & 0xffff) ^ (((s >> 15) & 1) * 0x1021)
    return s


def test_byte_table_comes_from_the_polynomial(emu):
    tab = np.zeros(256, np.uint16)
    emu.hash_emu_crc_tab(C.c_void_p(tab.ctypes.data))
    for h in range(256):                                       # entry h: what the high byte h of a state turns into over eight shifts
        assert int(tab[h]) == shift_bits(h << 8, [0] * 8), h
    assert int(tab[1]) == 0x1021 and len(set(tab.tolist())) == 256


def test_adv_feeds_zero_bits(emu):
    rng = np.random.default_rng(5)
    for s in [0, 1, 0x8000, 0xffff] + rng.integers(0, 1 << 16, 20).tolist():
        for n in (0, 1, 7, 8, 15, 16, 17, 128, 1000):
            assert emu.hash_emu_crc_adv(s, n) == shift_bits(s, [0] * n), (s, n)
    assert all(emu.hash_emu_crc_adv(0, n) == 0 for n in (1, 16, 8 * 16384))      # state 0 stays 0 under zero input
    assert emu.hash_emu_crc_xpow(0) == 1 and emu.hash_emu_crc_xpow(15) == 0x8000 and emu.hash_emu_crc_xpow(16) == 0x1021
    # x^n for the lengths of real planes: against repeated squaring done here, and additive in the exponent
    for n in (8 * 3840 * 2160, 8 * 1920 * 1080, 8 * 4096 * 4160, (1 << 40) + 5):
        a, b = n // 3, n - n // 3
        assert emu.hash_emu_crc_xpow(n) == emu.hash_emu_crc_mul(emu.hash_emu_crc_xpow(a), emu.hash_emu_crc_xpow(b))
    assert emu.hash_emu_crc_xpow(1 << 20) == shift_bits(1, [0] * (1 << 20))


def test_mul_is_the_product_mod_p(emu):
    rng = np.random.default_rng(6)
    for a, b, c in rng.integers(0, 1 << 16, (50, 3)).tolist():
        m = emu.hash_emu_crc_mul
        assert m(a, b) == m(b, a) and m(a, 1) == a and m(a, 0) == 0
        assert m(a, b ^ c) == m(a, b) ^ m(a, c) and m(m(a, b), c) == m(a, m(b, c))
        assert m(a, 2) == shift_bits(a, [0])


def test_fold_identity_with_uneven_cuts(emu):
    """state(AB, s) = adv(state(A, s), 8 |B|) ^ state(B, 0), and the digest = the bit-by-bit definition"""
    data = bytes(np.random.default_rng(7).integers(0, 256, 3000, dtype=np.uint8))
    whole = emu.hash_emu_crc_bytes(0xffff, data, len(data))
    assert whole == shift_bits(0xffff, [(v >> (7 - i)) & 1 for v in data for i in range(8)])
    for cut in (0, 1, 16, 17, 1000, 2999, 3000):
        a, b = data[:cut], data[cut:]
        sa = emu.hash_emu_crc_bytes(0xffff, a, len(a))
        assert whole == emu.hash_emu_crc_adv(sa, 8 * len(b)) ^ emu.hash_emu_crc_bytes(0, b, len(b)), cut
    # the initial state's term on its own, as hash_fold adds it: state(M, 0xffff) = adv(0xffff, 8 |M|) ^ state(M, 0)
    assert whole == emu.hash_emu_crc_adv(0xffff, 8 * len(data)) ^ emu.hash_emu_crc_bytes(0, data, len(data))
    for n in (0, 1, 64, 128, 1500, 3000):
        assert emu.hash_emu_crc_digest(data[:n], n) == hash_ref.crc_bitwise(data[:n]) == hash_ref.crc(data[:n]), n
    assert emu.hash_emu_crc_digest(bytes(64), 64) == 0xd5b6 and emu.hash_emu_crc_digest(bytes(128), 128) == 0xb28b
    # zeros in front of a message are neutral from state 0, zeros behind it are not
    assert emu.hash_emu_crc_bytes(0, bytes(100) + data, 100 + len(data)) == emu.hash_emu_crc_bytes(0, data, len(data))
    assert emu.hash_emu_crc_bytes(0, data + bytes(1), len(data) + 1) != emu.hash_emu_crc_bytes(0, data, len(data))


def test_argument_rule_names_the_argument(emu):
    """hash_args_check, the first thing fcu_picture_hash calls (the GPU tests assert the same on the library)"""
    planes, _ = HC.case(8, 8, 11)
    ptr = (C.c_void_p * 3)(*[p.ctypes.data for p in planes])
    out = np.zeros(68, np.uint8)

    def call(n, kinds, pl, o):
        err = C.create_string_buffer(256)
        return emu.hash_emu(8, 8, n, kinds, 1, pl, o, err, 256), err.value.decode()

    assert call(1, 7, ptr, out.ctypes.data)[0] == 1
    for args, name in (((0, 7, ptr, out.ctypes.data), "n_pics"), ((1, 0, ptr, out.ctypes.data), "kinds"), ((1, 8, ptr, out.ctypes.data), "kinds"),
                       ((1, 7, None, out.ctypes.data), "dev_planes"), ((1, 7, ptr, None), "host_hashes"),
                       ((1, 7, (C.c_void_p * 3)(ptr[0], None, ptr[2]), out.ctypes.data), "dev_planes[1]")):
        rc, err = call(*args)
        assert rc == -2 and name in err and err.startswith("fcu_picture_hash: "), (name, err)
