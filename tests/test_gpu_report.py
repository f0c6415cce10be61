"""GPU tests of the picture report through the C ABI (fcu_picture_report): the emulator's cases with uploaded planes and
records (no decision is run), planes at odd byte offsets on both load paths, a decided + deblocked picture against the numpy
reference on the device's own data and on the oracle's, the PSNR the reference encoder printed for the survey frame, both
host drivers with report=True, and the argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

import hmo_py
import report_cases as RC
import report_ref

pytestmark = pytest.mark.gpu


def up(a, offset=0):
    """the uint8 array on the device, its first byte `offset` bytes into a fresh allocation"""
    buf = torch.zeros(a.size + 64, dtype=torch.uint8, device="cuda")
    v = buf[offset:offset + a.size].view(a.shape)
    v.copy_(torch.from_numpy(np.array(a)))            # (a writable copy: the cases are read-only)
    assert v.data_ptr() % 16 == offset % 16
    return v


def picture(c, offset=0):
    org, rec, records = c[:3]
    return {"org": [up(p, offset) for p in org], "rec": [up(p, offset) for p in rec], "out": up(records.reshape(-1))}


def host(planes):
    return [p.cpu().numpy() for p in planes]


@pytest.mark.parametrize("w,h,kind", [(w, h, "noise") for w, h in RC.SIZES] + [(320, 256, "saturated")])
def test_emulator_cases_through_the_library(w, h, kind, pkg):
    c = RC.case(w, h, 6 if kind == "saturated" else 5, kind)
    eng = pkg.CuEngine(w, h, max_chains=1)
    got, ctu, ms = eng.report([picture(c)], ctu=True, timed=True)
    report_ref.assert_equal(got[0], ctu[0], c[3], c[4], (w, h, kind))
    if kind == "saturated":
        assert int(got[0]["ssd"][0]) == 5326848000
    assert len(ms) == 2 and all(m >= 0 for m in ms)
    again = eng.report([picture(c)])                          # the context's own CTU buffer instead of the caller's
    report_ref.assert_equal(again[0], None, c[3], c[4])
    eng.destroy()


def test_batch_of_three_equals_three_calls(pkg):
    cases = [RC.case(136, 72, s) for s in (5, 8, 9)]
    eng = pkg.CuEngine(136, 72, max_chains=1)
    pics = [picture(c) for c in cases]
    got, ctu = eng.report(pics, ctu=True)
    for i, c in enumerate(cases):
        one, one_ctu = eng.report([pics[i]], ctu=True)
        report_ref.assert_equal(got[i], ctu[i], one[0], one_ctu[0], i)
        report_ref.assert_equal(got[i], ctu[i], c[3], c[4], i)
    eng.destroy()


@pytest.mark.parametrize("offset", [1, 4])
@pytest.mark.parametrize("w,h", [(72, 40), (128, 64)])
def test_planes_at_any_byte_offset(w, h, offset, pkg):
    """views that start 1 and 4 bytes into a larger allocation: the byte-exact load path (128x64 takes the wide one when its
    planes are aligned, test_emulator_cases_through_the_library)"""
    c = RC.case(w, h, 5)
    eng = pkg.CuEngine(w, h, max_chains=1)
    got, ctu = eng.report([picture(c, offset)], ctu=True)
    report_ref.assert_equal(got[0], ctu[0], c[3], c[4], (w, h, offset))
    eng.destroy()


def test_decided_and_deblocked_picture(pkg):
    """128x64 synth.mixed seed 3 at QP 32, decide -> deblock: the device report == the reference on copies of the device's planes
    and records == the reference on the oracle's records and deblocked planes"""
    f = pkg.synth.mixed(128, 64, seed=3)
    eng = pkg.CuEngine(128, 64, max_chains=1)
    rec, out = eng.init_chain(0, f, 32)
    eng.compress_chains(0, 1, eng.n_ctu)
    eng.deblock(0)
    got, ctu = eng.report([{"org": eng._keep[0][0], "rec": rec, "out": out}], ctu=True)
    report_ref.assert_equal(got[0], ctu[0], *report_ref.picture_report(pkg, f, host(rec), out.cpu().numpy()))
    ref = hmo_py.Encoder(*f, 32)
    ref.compress_frame()
    ref.deblock()
    want = report_ref.picture_report(pkg, f, ref.rec, np.frombuffer(ref.all_ctus_bytes(), np.uint8))
    report_ref.assert_equal(got[0], ctu[0], *want)
    assert int(got[0]["n_part"]) == 2 * 256 and int(got[0]["intra_part"]) == 512 and int(got[0]["bits"]) > 0
    eng.destroy()


def test_psnr_of_the_survey_frame(pkg):
    """decide -> deblock -> SAO of the survey's 416x240 frame: the report's PSNR is what the reference encoder printed"""
    f = pkg.synth.survey_frame(416, 240, 1234)
    eng = pkg.CuEngine(416, 240, max_chains=1)
    rec, out = eng.init_chain(0, f, 32)
    eng.compress_chains(0, 1, eng.n_ctu)
    eng.deblock(0)
    eng.sao([{"org": eng._keep[0][0], "rec": rec, "qp": 32, "lambda_": 0.57 * 2.0 ** ((32 - 12) / 3.0)}])
    got = eng.report([{"org": eng._keep[0][0], "rec": rec, "out": out}])[0]
    assert ["%.4f" % v for v in got["psnr"]] == ["32.3524", "41.0897", "41.1974"]
    report_ref.assert_equal(got, None, *report_ref.picture_report(pkg, f, host(rec), out.cpu().numpy()))
    eng.destroy()


def test_lowdelay_driver_reports_every_clip(pkg):
    import search_trace as st
    w, h = 128, 64
    dec = pkg.lowdelay.LowDelayPDecider(w, h, 30, n_clips=2, search_range=8, report=True)
    for poc in range(2):
        frames = [st.moving_frame(pkg.synth, "mixed", w, h, 9 + s, poc) for s in range(2)]
        res = dec.decide_picture(frames)
        for f, r in zip(frames, res):
            want, _ = report_ref.picture_report(pkg, f, host(r["rec"]), r["out"].cpu().numpy())
            report_ref.assert_equal(r["report"], None, want, None, poc)
    dec.close()
    dec = pkg.lowdelay.LowDelayPDecider(w, h, 30, n_clips=2, search_range=8)
    res = dec.decide_picture(frames)
    assert all(sorted(r) == ["first", "lambda", "out", "poc", "qp", "rec", "rec_unfiltered", "slice_type"] for r in res)
    dec.close()


def test_sequence_driver_reports(pkg):
    f = pkg.synth.mixed(128, 64, seed=3)
    dec = pkg.sequence.SequenceDecider(128, 64, 32, fast=False, report=True)
    r = dec.decide(f)
    want, _ = report_ref.picture_report(pkg, f, host(r["rec"]), r["out"].cpu().numpy())
    report_ref.assert_equal(r["report"], None, want, None)
    assert np.array_equal(np.bincount(r["depth"].ravel(), minlength=4)[:4], np.asarray(r["report"]["depth_part"]).astype(np.int64))
    dec.close()
    dec = pkg.sequence.SequenceDecider(128, 64, 32, fast=False)
    assert "report" not in dec.decide(f)
    dec.close()


def test_bad_arguments_name_the_argument(pkg):
    e = pkg.engine
    c = RC.case(64, 64, 5)
    eng = pkg.CuEngine(64, 64, max_chains=1)
    p = picture(c)
    lib = eng.lib
    org, rec, out = (C.c_void_p * 3)(*[t.data_ptr() for t in p["org"]]), (C.c_void_p * 3)(*[t.data_ptr() for t in p["rec"]]), (C.c_void_p * 1)(p["out"].data_ptr())
    reports = np.zeros(1, e.PIC_REPORT_DTYPE)
    call = lambda n, o, r, u, rep: lib.fcu_picture_report(eng.h, n, o, r, u, rep, None, None, None)
    err = lambda: lib.fcu_last_error().decode()
    assert call(1, org, rec, out, reports.ctypes.data) == 0
    assert call(0, org, rec, out, reports.ctypes.data) == -2 and "n_pics" in err()
    assert call(1, None, rec, out, reports.ctypes.data) == -2 and "dev_org" in err()
    assert call(1, org, None, out, reports.ctypes.data) == -2 and "dev_rec" in err()
    assert call(1, org, rec, None, reports.ctypes.data) == -2 and "dev_out" in err()
    assert call(1, org, rec, out, None) == -2 and "host_reports" in err()
    hole = (C.c_void_p * 3)(org[0], None, org[2])
    assert call(1, hole, rec, out, reports.ctypes.data) == -2 and "dev_org[1]" in err()
    assert call(1, org, hole, out, reports.ctypes.data) == -2 and "dev_rec[1]" in err()
    assert call(1, org, rec, (C.c_void_p * 1)(None), reports.ctypes.data) == -2 and "dev_out[0]" in err()
    eng.destroy()
