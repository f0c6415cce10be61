"""Reference of the picture hash (csrc/fcu_hash.h): HM's calcMD5 / calcCRC / calcChecksum and digestToString
(TComPicYuvMD5.cpp:44-225) of 8-bit planes, from the definitions.  MD5 is hashlib's; the checksum is numpy from the definition; the
CRC runs through binascii.crc_hqx (table-driven, polynomial 0x1021), which this file asserts once against the bit-by-bit loop."""
import binascii
import hashlib

import numpy as np

KINDS = ("md5", "crc", "checksum")
LABELS = {"md5": "MD5", "crc": "CRC", "checksum": "Checksum"}


def crc_bitwise(data):
    """compCRC (:89-127) bit by bit: 16 bits, polynomial 0x1021, state 0xffff, message bits shifted in at the low end MSB first,
    sixteen zero bits flushed at the end"""
    crc = 0xffff
    for byte in bytes(data):
        for bit in range(8):
            msb = (crc >> 15) & 1
            crc = (((crc << 1) + ((byte >> (7 - bit)) & 1)) & 0xffff) ^ (msb * 0x1021)
    for _ in range(16):
        msb = (crc >> 15) & 1
        crc = ((crc << 1) & 0xffff) ^ (msb * 0x1021)
    return crc


# crc_hqx shifts a byte in sixteen bits ahead of compCRC (its state after a message M from state s is s x^8|M| + M x^16): started
# from 0xffff advanced by the sixteen flushed bits, it ends where compCRC ends after its flush
_HQX_INIT = 0xffff
for _ in range(16):
    _HQX_INIT = ((_HQX_INIT << 1) & 0xffff) ^ (((_HQX_INIT >> 15) & 1) * 0x1021)


def crc(data):
    return binascii.crc_hqx(bytes(data), _HQX_INIT)


_probe = np.random.default_rng(1021).integers(0, 256, 1500, dtype=np.uint8).tobytes()
assert all(crc(_probe[:n]) == crc_bitwise(_probe[:n]) for n in (0, 1, 2, 15, 16, 17, 64, 1000, 1500))
assert (crc(bytes(64)), crc(bytes(128))) == (0xd5b6, 0xb28b)      # all-zero planes: only the initial state's term tells lengths apart


def checksum(plane):
    """compChecksum (:141-165): sum mod 2^32 of sample ^ (uint8)((x & 255) ^ (y & 255) ^ (x >> 8) ^ (y >> 8))"""
    h, w = plane.shape
    return int((np.asarray(plane, np.uint8) ^ checksum_mask(w, h)).sum(dtype=np.uint64) & 0xffffffff)


def checksum_mask(w, h):
    x, y = np.arange(w, dtype=np.uint32)[None, :], np.arange(h, dtype=np.uint32)[:, None]
    return (((x & 255) ^ (y & 255) ^ (x >> 8) ^ (y >> 8)) & 255).astype(np.uint8)


def plane_digest(plane, kind):
    """the digest bytes of one plane in HM's order (crc and checksum high byte first)"""
    plane = np.ascontiguousarray(plane, np.uint8)
    if kind == "md5":
        return hashlib.md5(plane.tobytes()).digest()
    if kind == "crc":
        return crc(plane.tobytes()).to_bytes(2, "big")
    return checksum(plane).to_bytes(4, "big")


def picture(planes, kinds=KINDS):
    """{kind: [hex of Y, Cb, Cr]} and under "line" HM's strings (digestToString, :209-225: the planes' digests joined by ',')"""
    d = {k: [plane_digest(p, k).hex() for p in planes] for k in kinds}
    d["line"] = {k: ",".join(d[k]) for k in kinds}
    return d


def line(kind, string):
    """the end of the encoder's picture line (TEncGOP.cpp:1746-1754)"""
    return " [%s:%s]" % (LABELS[kind], string)
