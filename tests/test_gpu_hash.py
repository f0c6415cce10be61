"""GPU tests of the picture hash through the C ABI (fcu_picture_hash): the emulator's cases with uploaded planes (no decision is
run), planes at odd byte offsets, a batch against single calls, a decided + deblocked picture against hashlib and the definitions
(tests/hash_ref.py) on the device's own planes and on the oracle's, the survey frame after SAO, both host drivers with pic_hash,
and the argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

import hash_cases as HC
import hash_ref
import hmo_py

pytestmark = pytest.mark.gpu


def up(a, offset=0):
    """the uint8 array on the device, its first byte `offset` bytes into a fresh allocation"""
    buf = torch.zeros(a.size + 64, dtype=torch.uint8, device="cuda")
    v = buf[offset:offset + a.size].view(a.shape)
    v.copy_(torch.from_numpy(np.array(a)))            # (a writable copy: the cases are read-only)
    assert v.data_ptr() % 16 == offset % 16
    return v


def host(planes):
    return [p.cpu().numpy() for p in planes]


@pytest.mark.parametrize("w,h,seed,content", HC.all_cases())
def test_emulator_cases_through_the_library(w, h, seed, content, pkg):
    planes, ref = HC.case(w, h, seed, content)
    eng = pkg.CuEngine(w, h, max_chains=1)
    dev = [up(p) for p in planes]
    got, ms = eng.picture_hash([dev], kinds=hash_ref.KINDS, timed=True)
    assert got[0] == ref, (w, h, content)
    assert len(ms) == 3 and all(m >= 0 for m in ms)
    got, ms = eng.picture_hash([{"rec": dev}], kinds=("crc",), timed=True)      # only the kinds asked for are computed
    assert got[0] == HC.select(ref, ("crc",)) and ms[0] >= 0 and ms[1] >= 0 and ms[2] == 0
    got, ms = eng.picture_hash([dev], kinds=("md5",), timed=True)
    assert got[0] == HC.select(ref, ("md5",)) and ms[0] == 0 and ms[1] == 0 and ms[2] >= 0
    assert eng.picture_hash([dev], kinds="checksum")[0] == HC.select(ref, ("checksum",))
    eng.destroy()


def test_fields_not_asked_for_are_zero(pkg):
    e = pkg.engine
    planes, ref = HC.case(72, 40, 11)
    eng = pkg.CuEngine(72, 40, max_chains=1)
    dev = [up(p) for p in planes]
    ptr = (C.c_void_p * 3)(*[t.data_ptr() for t in dev])
    eng.picture_hash([dev], kinds=hash_ref.KINDS)            # the context's record now holds all three
    for kinds in (("md5",), ("crc",), ("checksum", "md5")):
        buf = np.frombuffer(b"\xaa" * 68, e.PIC_HASH_DTYPE).copy()
        assert eng.lib.fcu_picture_hash(eng.h, 1, sum(e.HASH_KINDS[k] for k in kinds), ptr, buf.ctypes.data, None, None) == 0
        for k in hash_ref.KINDS:
            assert buf[0][k].any() == (k in kinds), (kinds, k)
            if k in kinds:
                assert [bytes(buf[0][k][c]).hex() for c in range(3)] == ref[k]
        assert not buf[0]["pad"].any()
    eng.destroy()


@pytest.mark.parametrize("offset", [1, 4])
@pytest.mark.parametrize("w,h", [(72, 40), (264, 128)])
def test_planes_at_any_byte_offset(w, h, offset, pkg):
    """views that start 1 and 4 bytes into a larger allocation: the byte-exact load path"""
    planes, ref = HC.case(w, h, 11)
    eng = pkg.CuEngine(w, h, max_chains=1)
    assert eng.picture_hash([[up(p, offset) for p in planes]], kinds=hash_ref.KINDS)[0] == ref
    eng.destroy()


def test_batch_of_three_equals_three_calls(pkg):
    cases = [HC.case(264, 128, s) for s in (11, 12, 13)]
    eng = pkg.CuEngine(264, 128, max_chains=1)
    pics = [[up(p) for p in c[0]] for c in cases]
    got = eng.picture_hash(pics, kinds=hash_ref.KINDS)
    for i, c in enumerate(cases):
        assert got[i] == eng.picture_hash([pics[i]], kinds=hash_ref.KINDS)[0] == c[1], i
    assert eng.picture_hash(pics, kinds=hash_ref.KINDS) == got                  # a repeated call: the same digests
    for k in hash_ref.KINDS:
        assert len({g["line"][k] for g in got}) == 3
    eng.destroy()


def test_decided_and_deblocked_picture(pkg):
    """128x64 synth.mixed seed 3 at QP 32, decide -> deblock: the device digests == the reference on copies of the device's planes
    == the reference on the oracle's deblocked planes"""
    f = pkg.synth.mixed(128, 64, seed=3)
    eng = pkg.CuEngine(128, 64, max_chains=1)
    rec, out = eng.init_chain(0, f, 32)
    eng.compress_chains(0, 1, eng.n_ctu)
    eng.deblock(0)
    got = eng.picture_hash([{"rec": rec}], kinds=hash_ref.KINDS)[0]
    assert got == hash_ref.picture(host(rec))
    ref = hmo_py.Encoder(*f, 32)
    ref.compress_frame()
    ref.deblock()
    assert got == hash_ref.picture(ref.rec)
    eng.destroy()


def test_survey_frame_after_sao(pkg):
    """decide -> deblock -> SAO of the survey's 416x240 frame: the digests of the final planes"""
    f = pkg.synth.survey_frame(416, 240, 1234)
    eng = pkg.CuEngine(416, 240, max_chains=1)
    rec, out = eng.init_chain(0, f, 32)
    eng.compress_chains(0, 1, eng.n_ctu)
    eng.deblock(0)
    eng.sao([{"org": eng._keep[0][0], "rec": rec, "qp": 32, "lambda_": 0.57 * 2.0 ** ((32 - 12) / 3.0)}])
    assert eng.picture_hash([rec], kinds=hash_ref.KINDS)[0] == hash_ref.picture(host(rec))
    eng.destroy()


def test_lowdelay_driver_hashes_every_clip(pkg):
    import search_trace as st
    w, h = 128, 64
    dec = pkg.lowdelay.LowDelayPDecider(w, h, 30, n_clips=2, search_range=8, pic_hash="md5")
    for poc in range(2):
        frames = [st.moving_frame(pkg.synth, "mixed", w, h, 9 + s, poc) for s in range(2)]
        res = dec.decide_picture(frames)
        for r in res:
            assert r["hash"] == hash_ref.picture(host(r["rec"]), ("md5",))["line"]["md5"], poc
        assert res[0]["hash"] != res[1]["hash"]
    dec.close()
    dec = pkg.lowdelay.LowDelayPDecider(w, h, 30, n_clips=2, search_range=8)
    res = dec.decide_picture(frames)
    assert all(sorted(r) == ["first", "lambda", "out", "poc", "qp", "rec", "rec_unfiltered", "slice_type"] for r in res)
    dec.close()


def test_sequence_driver_hashes(pkg):
    f = pkg.synth.mixed(128, 64, seed=3)
    dec = pkg.sequence.SequenceDecider(128, 64, 32, fast=False, pic_hash="crc")
    r = dec.decide(f)
    assert r["hash"] == hash_ref.picture(host(r["rec"]), ("crc",))["line"]["crc"] and len(r["hash"]) == 14
    keys = sorted(r)
    dec.close()
    dec = pkg.sequence.SequenceDecider(128, 64, 32, fast=False)
    r = dec.decide(f)
    assert "hash" not in r and sorted(list(r) + ["hash"]) == keys      # without the option: exactly the keys there were
    dec.close()
    with pytest.raises(ValueError):
        pkg.sequence.SequenceDecider(128, 64, 32, pic_hash="sha1")


def test_bad_arguments_name_the_argument(pkg):
    e = pkg.engine
    planes, _ = HC.case(64, 64, 11)
    eng = pkg.CuEngine(64, 64, max_chains=1)
    dev = [up(p) for p in planes]
    lib = eng.lib
    ptr = (C.c_void_p * 3)(*[t.data_ptr() for t in dev])
    hashes = np.zeros(1, e.PIC_HASH_DTYPE)
    call = lambda n, kinds, pl, out: lib.fcu_picture_hash(eng.h, n, kinds, pl, out, None, None)
    err = lambda: lib.fcu_last_error().decode()
    assert call(1, 7, ptr, hashes.ctypes.data) == 0
    assert call(0, 7, ptr, hashes.ctypes.data) == -2 and "n_pics" in err()
    assert call(1, 0, ptr, hashes.ctypes.data) == -2 and "kinds" in err()
    assert call(1, 8, ptr, hashes.ctypes.data) == -2 and "kinds" in err()
    assert call(1, 7, None, hashes.ctypes.data) == -2 and "dev_planes" in err()
    assert call(1, 7, ptr, None) == -2 and "host_hashes" in err()
    assert call(1, 7, (C.c_void_p * 3)(ptr[0], None, ptr[2]), hashes.ctypes.data) == -2 and "dev_planes[1]" in err()
    buf = C.create_string_buffer(128)
    assert lib.fcu_hash_string(hashes.ctypes.data, 3, buf, 128) == -2 and "kind" in err()
    eng.destroy()
