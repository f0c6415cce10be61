"""The picture-report kernels (csrc/fcu_report.h: report_ctu, report_pic) on the CPU (tests/emu/report_emu.cpp: the kernel
source with the HIP keywords defined away, every grid run as a loop) against the numpy reference tests/report_ref.py: every
field of both records, exact.  Every comparison also checks the per-CTU records against the picture sums."""
import ctypes as C
import os

import numpy as np
import pytest

import report_cases as RC
import report_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def emu_report(pkg, pictures, wide=1, ctu_buf=None):
    """pictures: list of (org, rec, records).  Returns (list of report dicts, CTU records [n, n_ctu], path taken: 1 = wide loads)"""
    e = pkg.engine
    L = C.CDLL(os.path.join(ROOT, "tests", "emu", "libreport_emu.so"))
    L.report_emu.argtypes = [C.c_int] * 4 + [C.c_void_p] * 5
    n = len(pictures)
    h, w = pictures[0][0][0].shape
    n_ctu = ((w + 63) // 64) * ((h + 63) // 64)
    org, rec, out = (C.c_void_p * (3 * n))(), (C.c_void_p * (3 * n))(), (C.c_void_p * n)()
    keep = []
    for i, (o, r, records) in enumerate(pictures):
        for k in range(3):
            assert o[k].flags.c_contiguous and r[k].flags.c_contiguous
            org[3 * i + k], rec[3 * i + k] = o[k].ctypes.data, r[k].ctypes.data
        records = np.ascontiguousarray(records)
        keep.append(records)
        out[i] = records.ctypes.data
    reports = np.zeros(n, e.PIC_REPORT_DTYPE)
    ctu = np.zeros((n, n_ctu), e.CTU_REPORT_DTYPE) if ctu_buf is None else ctu_buf
    path = L.report_emu(w, h, n, wide, org, rec, out, reports.ctypes.data, ctu.ctypes.data)
    return [e.pic_report_to_dict(reports[i]) for i in range(n)], ctu, path


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("w,h", RC.SIZES)
def test_sizes_on_both_load_paths(w, h, wide, built, pkg):
    org, rec, records, pic, ctu = RC.case(w, h, 5)
    got, got_ctu, path = emu_report(pkg, [(org, rec, records)], wide)
    assert path == (1 if wide and w % 16 == 0 else 0)         # the planes sit on 16-byte boundaries: the width decides
    assert int(pic["bits"]) > (1 << 32) or len(ctu) == 1
    report_ref.assert_equal(got[0], got_ctu[0], pic, ctu, (w, h, wide))


@pytest.mark.parametrize("wide", [0, 1])
def test_saturated_picture_passes_32_bits(wide, built, pkg):
    org, rec, records, pic, ctu = RC.case(320, 256, 6, "saturated")
    assert int(pic["ssd"][0]) == 5326848000 > (1 << 32) and all(int(v) == 4096 * 255 * 255 for v in ctu["ssd"][:, 0])
    got, got_ctu, path = emu_report(pkg, [(org, rec, records)], wide)
    assert path == wide
    report_ref.assert_equal(got[0], got_ctu[0], pic, ctu)
    assert int(got[0]["ssd"][0]) == 5326848000 and got[0]["psnr"][0] == 0.0


@pytest.mark.parametrize("w,h", [(72, 40), (136, 72), (176, 88)])
def test_entries_outside_the_picture_do_not_count(w, h, built, pkg):
    """the same records with the entries of partitions outside the picture drawn again: every count stays"""
    org, rec, records, pic, ctu = RC.case(w, h, 5)
    other = RC.records(w, h, 5 + 1000, outside_seed=77)
    out = ~RC.inside_mask(w, h)
    assert out.any() and not np.array_equal(other, records)
    assert np.array_equal(other[:, :256][~out], records[:, :256][~out])      # (depth: inside entries untouched)
    got, got_ctu, _ = emu_report(pkg, [(org, rec, other)])
    report_ref.assert_equal(got[0], got_ctu[0], pic, ctu, (w, h))
    want2 = report_ref.picture_report(pkg, org, rec, other)
    report_ref.assert_equal(got[0], got_ctu[0], *want2)


@pytest.mark.parametrize("offset", [1, 4])
@pytest.mark.parametrize("w,h", [(72, 40), (128, 64)])
def test_planes_at_any_byte_offset(w, h, offset, built, pkg):
    org, rec, records, pic, ctu = RC.case(w, h, 5)
    got, got_ctu, path = emu_report(pkg, [([RC.aligned(p, offset) for p in org], [RC.aligned(p, offset) for p in rec], records)])
    assert path == 0
    report_ref.assert_equal(got[0], got_ctu[0], pic, ctu, (w, h, offset))


def test_batch_of_three_equals_three_calls(built, pkg):
    cases = [RC.case(136, 72, s) for s in (5, 8, 9)]
    got, got_ctu, _ = emu_report(pkg, [c[:3] for c in cases])
    for i, c in enumerate(cases):
        one, one_ctu, _ = emu_report(pkg, [c[:3]])
        report_ref.assert_equal(got[i], got_ctu[i], one[0], one_ctu[0], i)
        report_ref.assert_equal(got[i], got_ctu[i], c[3], c[4], i)
    assert len({int(g["ssd"][0]) for g in got}) == 3


def test_second_call_gives_the_same_bytes(built, pkg):
    """nothing is accumulated into memory: a buffer full of stale bytes ends up the same as after a second call"""
    org, rec, records, pic, ctu = RC.case(136, 72, 5)
    buf = np.frombuffer(b"\xaa" * (6 * pkg.engine.CTU_REPORT_DTYPE.itemsize), pkg.engine.CTU_REPORT_DTYPE).reshape(1, 6).copy()
    got1, _, _ = emu_report(pkg, [(org, rec, records)], ctu_buf=buf)
    first = buf.tobytes()
    got2, _, _ = emu_report(pkg, [(org, rec, records)], ctu_buf=buf)
    assert buf.tobytes() == first
    report_ref.assert_equal(got2[0], buf[0], pic, ctu)
    report_ref.assert_equal(got1[0], None, got2[0], None)


def test_report_layouts_match_the_library(built, pkg):
    e = pkg.engine
    lib = C.CDLL(pkg.lib_path())
    assert lib.fcu_abi_sizeof(8) == C.sizeof(e.PicReport) == e.PIC_REPORT_DTYPE.itemsize == 176
    assert lib.fcu_abi_sizeof(9) == C.sizeof(e.CtuReport) == e.CTU_REPORT_DTYPE.itemsize == report_ref.CTU_REPORT.itemsize == 64
    for name, _ in e.PicReport._fields_:                      # no implicit padding: the numpy and ctypes offsets agree field by field
        assert getattr(e.PicReport, name).offset == e.PIC_REPORT_DTYPE.fields[name][1], name
    for name, _ in e.CtuReport._fields_:
        assert getattr(e.CtuReport, name).offset == e.CTU_REPORT_DTYPE.fields[name][1], name
    assert lib.fcu_abi_sizeof(99) == -1


def test_drivers_keep_their_keys_without_the_option(pkg):
    """report=False is the default of both drivers (the GPU tests check the result dicts)"""
    import inspect
    for cls in (pkg.lowdelay.LowDelayPDecider, pkg.sequence.SequenceDecider):
        assert inspect.signature(cls.__init__).parameters["report"].default is False
