"""The decision-map and split-match kernels (csrc/fcu_maps.h: maps_ctu, match_ctu, match_pic) on the CPU (tests/emu/maps_emu.cpp:
the kernel source with the HIP keywords defined away, every grid run as a loop, behind the argument rules of fcu_host.h) against
the numpy reference tests/maps_ref.py: every output of every case byte for byte, both store paths, the properties the reference
must have on its own, the refusals, and a repeated call into a buffer of stale bytes."""
import ctypes as C
import os

import numpy as np
import pytest

import maps_cases as MC
import maps_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -2


def lib():
    L = C.CDLL(os.path.join(ROOT, "tests", "emu", "libmaps_emu.so"))
    L.maps_emu.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_int] + [C.c_void_p] * 6
    L.match_emu.argtypes = [C.c_int] * 3 + [C.c_void_p] * 4
    L.maps_emu_last_error.restype = C.c_char_p
    return L


def buffer(nbytes, offset=0, fill=0xaa):
    """nbytes stale bytes whose first one sits `offset` bytes past a 16-byte boundary"""
    buf = np.full(nbytes + 48, fill, np.uint8)
    start = (-buf.ctypes.data) % 16 + offset
    v = buf[start:start + nbytes]
    assert v.ctypes.data % 16 == offset % 16
    return v


def emu_maps(w, h, recs, fields=("depth",), mv=False, labels=False, obfs=None, wide=1, offset=0, out=None):
    """recs: list of record arrays.  Returns (list of per-picture dicts as maps_ref.picture_maps gives them, alignment of the store
    path taken, the raw output buffers)"""
    n, H4, W4 = len(recs), h // 4, w // 4
    NL = sum(a * b for a, b in maps_ref.level_shapes(w, h))
    keep = [np.ascontiguousarray(r) for r in recs]
    outp = (C.c_void_p * n)(*[r.ctypes.data for r in keep])
    ids = (C.c_int * max(len(fields), 1))(*[maps_ref.FIELDS[f][0] for f in fields])
    obfk = [np.ascontiguousarray(o) for o in obfs] if obfs is not None else None
    obfp = (C.c_void_p * n)(*[o.ctypes.data for o in obfk]) if obfs is not None else None
    bufs = out or {"bytes": buffer(n * len(fields) * H4 * W4, offset) if fields else None, "mv": buffer(n * H4 * W4 * 4, offset) if mv else None,
                   "labels": buffer(n * NL) if labels else None, "n_obf": buffer(n * NL * 2, offset) if obfs is not None else None}
    ptr = lambda k: bufs[k].ctypes.data if bufs[k] is not None else None
    rc = lib().maps_emu(w, h, n, wide, outp, len(fields), ids, ptr("bytes"), ptr("mv"), ptr("labels"), obfp, ptr("n_obf"))
    assert rc > 0, lib().maps_emu_last_error()
    pics = []
    for i in range(n):
        d = {"bytes": bufs["bytes"].reshape(n, len(fields), H4, W4)[i] if fields else None}
        if mv:
            d["mv"] = bufs["mv"].view(np.int16).reshape(n, H4, W4, 2)[i]
        if labels:
            d["labels"] = maps_ref.split_levels(bufs["labels"].view(np.int8).reshape(n, NL)[i], w, h)
        if obfs is not None:
            d["n_obf"] = maps_ref.split_levels(bufs["n_obf"].view(np.uint16).reshape(n, NL)[i], w, h)
        pics.append(d)
    return pics, rc, bufs


def emu_match(pkg, w, h, recs_a, recs_b, ctu=None):
    e = pkg.engine
    n = len(recs_a)
    n_ctu = ((w + 63) // 64) * ((h + 63) // 64)
    ka, kb = [np.ascontiguousarray(r) for r in recs_a], [np.ascontiguousarray(r) for r in recs_b]
    pa, pb = (C.c_void_p * n)(*[r.ctypes.data for r in ka]), (C.c_void_p * n)(*[r.ctypes.data for r in kb])
    rec = np.zeros(n, e.PIC_MATCH_DTYPE)
    ctu = np.zeros((n, n_ctu), e.CTU_MATCH_DTYPE) if ctu is None else ctu
    assert lib().match_emu(w, h, n, pa, pb, rec.ctypes.data, ctu.ctypes.data) == 0
    return [e.pic_match_to_dict(rec[i]) for i in range(n)], ctu


@pytest.mark.parametrize("fields", sorted(MC.FIELD_LISTS))
@pytest.mark.parametrize("w,h", MC.SIZES)
def test_every_output_equals_the_reference(w, h, fields, built, pkg):
    r, obf, want = MC.case(w, h, 11)
    got, path, _ = emu_maps(w, h, [r], MC.FIELD_LISTS[fields], mv=True, labels=True, obfs=[obf])
    assert path == (16 if w % 64 == 0 else 2)                 # the buffers sit on 16-byte boundaries: the width decides
    maps_ref.assert_maps_equal(got[0], MC.select(want, MC.FIELD_LISTS[fields]), (w, h, fields))


@pytest.mark.parametrize("offset", [0, 2, 1])
def test_store_paths_give_the_same_maps(offset, built, pkg):
    """256x128 takes 16-byte rows when its bases are aligned (test above); here the 2-byte path is forced, then every base is moved
    by 2 bytes, then the byte maps to an odd address (the motion and N_OBF maps stay even: their element types ask for it)"""
    w, h = 256, 128
    r, obf, want = MC.case(w, h, 11)
    if offset == 1:
        got, path, _ = emu_maps(w, h, [r], MC.ALL_FIELDS, offset=1)
        assert path == 1
        maps_ref.assert_maps_equal(got[0], MC.select(want, MC.ALL_FIELDS, False, False, False))
        return
    got, path, _ = emu_maps(w, h, [r], MC.ALL_FIELDS, mv=True, labels=True, obfs=[obf], wide=1 if offset else 0, offset=offset)
    assert path == 2
    maps_ref.assert_maps_equal(got[0], MC.select(want, MC.ALL_FIELDS), offset)


def test_single_outputs(built, pkg):
    """every output on its own: nothing depends on another one being asked for"""
    w, h = 208, 136
    r, obf, want = MC.case(w, h, 11)
    for kw, sel in ((dict(fields=(), mv=True), (True, False, False)), (dict(fields=(), labels=True), (False, True, False)),
                    (dict(fields=(), obfs=[obf]), (False, False, True)), (dict(fields=("skip",)), (False, False, False))):
        got, _, _ = emu_maps(w, h, [r], **kw)
        maps_ref.assert_maps_equal(got[0], MC.select(want, kw["fields"], *sel), kw)


def test_batch_of_three_keeps_the_pictures_apart(built, pkg):
    w, h = 208, 136
    cases = [MC.case(w, h, s) for s in (11, 12, 13)]
    got, _, _ = emu_maps(w, h, [c[0] for c in cases], MC.MIXED_FIELDS, mv=True, labels=True, obfs=[c[1] for c in cases])
    for i, c in enumerate(cases):
        maps_ref.assert_maps_equal(got[i], MC.select(c[2], MC.MIXED_FIELDS), i)
    assert not np.array_equal(got[0]["bytes"], got[1]["bytes"]) and not np.array_equal(got[1]["labels"][3], got[2]["labels"][3])


def test_repeated_call_gives_identical_bytes(built, pkg):
    """buffers of stale bytes: after one call every byte is defined, and a second call changes none"""
    w, h = 208, 136
    r, obf, want = MC.case(w, h, 11)
    got, _, bufs = emu_maps(w, h, [r], MC.ALL_FIELDS, mv=True, labels=True, obfs=[obf])
    first = {k: v.tobytes() for k, v in bufs.items()}
    other, _, _ = emu_maps(w, h, [r], MC.ALL_FIELDS, mv=True, labels=True, obfs=[obf], out={k: buffer(v.size, fill=0x55) for k, v in bufs.items()})
    maps_ref.assert_maps_equal(other[0], MC.select(want, MC.ALL_FIELDS))       # (0x55 underneath instead of 0xaa: no byte left unwritten)
    again, _, bufs2 = emu_maps(w, h, [r], MC.ALL_FIELDS, mv=True, labels=True, obfs=[obf], out=bufs)
    assert {k: v.tobytes() for k, v in bufs2.items()} == first


@pytest.mark.parametrize("w,h", MC.SIZES)
def test_reference_properties(w, h, pkg):
    """what the reference must satisfy by itself: the labels rebuild the depth map, a decision matches itself, no poison anywhere"""
    r, obf, want = MC.case(w, h, 11)
    depth = want["bytes"][MC.ALL_FIELDS.index("depth")]
    assert np.array_equal(maps_ref.depth_from_labels(want["labels"], w, h), depth)
    m = maps_ref.split_match(pkg, r, r, w, h)
    assert m["part_equal"] == m["part_total"] == (w // 4) * (h // 4)
    assert not m["only_a"].any() and not m["only_b"].any() and not m["node"][:, 0, 1].any() and not m["node"][:, 1, 0].any()
    assert m["node"].sum() > 0
    if (w, h) == (208, 136):
        assert all((want["labels"][d] == maps_ref.FORCED).any() for d in range(3)) and not (want["labels"][3] == maps_ref.FORCED).any()
        assert all(v in np.unique(np.concatenate([l.ravel() for l in want["labels"]])) for v in (-1, 0, 1, 2))
    for k, f in enumerate(MC.ALL_FIELDS):
        poison = MC.POISON.get(f, MC.POISON["other"])
        assert not (want["bytes"][k] == poison).any(), f
    assert not (want["mv"] == MC.POISON["mv"]).any()
    inside = MC.inside_entries(w, h)
    if not inside.all():                                       # ... although the records are full of it
        assert (r[:, :256][~inside] == MC.POISON["depth"]).all()
    total = (np.asarray(obf) > 0).sum()                        # every level of N_OBF partitions the same set of blocks
    assert all(int(want["n_obf"][d].astype(np.int64).sum()) == total for d in range(4))


@pytest.mark.parametrize("w,h", MC.SIZES)
def test_split_match_equals_the_reference(w, h, built, pkg):
    a, b, want = MC.match_case(w, h, 11, 12)
    got, ctu = emu_match(pkg, w, h, [a, a], [b, a])
    maps_ref.assert_match_equal(got[0], want, (w, h))
    same = maps_ref.split_match(pkg, a, a, w, h)
    maps_ref.assert_match_equal(got[1], same, (w, h, "self"))
    for k in maps_ref.MATCH_KEYS:                              # the per-CTU records add up to the picture's
        assert np.array_equal(ctu[0][k].astype(np.int64).sum(axis=0), np.asarray(got[0][k]).astype(np.int64)), k
    assert not ctu["pad"].any()
    if (w, h) == (208, 136):
        assert want["only_a"].any() and want["only_b"].any() and want["node"][:, 0, 1].any() and 0 < want["part_equal"] < want["part_total"]


def test_split_match_second_call_gives_the_same_bytes(built, pkg):
    a, b, want = MC.match_case(208, 136, 11, 12)
    ctu = np.frombuffer(b"\xaa" * (12 * pkg.engine.CTU_MATCH_DTYPE.itemsize), pkg.engine.CTU_MATCH_DTYPE).reshape(1, 12).copy()
    emu_match(pkg, 208, 136, [a], [b], ctu)
    first = ctu.tobytes()
    got, _ = emu_match(pkg, 208, 136, [a], [b], ctu)
    assert ctu.tobytes() == first
    maps_ref.assert_match_equal(got[0], want)


def test_refusals_name_the_argument(built, pkg):
    """the host rules of fcu_host.h (maps_args_check, match_args_check): the code and text fcu_decision_maps / fcu_split_match return"""
    L = lib()
    r = np.ascontiguousarray(MC.case(64, 64, 11)[0])
    obf = np.ascontiguousarray(MC.case(64, 64, 11)[1])
    out, hole = (C.c_void_p * 1)(r.ctypes.data), (C.c_void_p * 1)(None)
    obfp = (C.c_void_p * 1)(obf.ctypes.data)
    b = buffer(4096)
    p = b.ctypes.data
    ids = lambda *v: (C.c_int * len(v))(*v)
    err = lambda: L.maps_emu_last_error().decode()
    call = lambda n, o, nf, f, by, mv, lab, ob, nobf: L.maps_emu(64, 64, n, 1, o, nf, f, by, mv, lab, ob, nobf)
    assert call(1, out, 1, ids(0), p, None, None, None, None) == 16
    assert call(0, out, 1, ids(0), p, None, None, None, None) == ARG and "n_pics" in err()
    assert call(1, None, 1, ids(0), p, None, None, None, None) == ARG and "dev_out is null" in err()
    assert call(1, hole, 1, ids(0), p, None, None, None, None) == ARG and "dev_out[0]" in err()
    assert call(1, out, 1, None, p, None, None, None, None) == ARG and "field_ids is null" in err()
    assert call(1, out, 20, ids(*range(20)), p, None, None, None, None) == ARG and "n_fields" in err()
    assert call(1, out, 2, ids(0, 19), p, None, None, None, None) == ARG and "field_ids[1] = 19" in err()
    assert call(1, out, 2, ids(0, -1), p, None, None, None, None) == ARG and "field_ids[1] = -1" in err()
    assert call(1, out, 3, ids(4, 0, 4), p, None, None, None, None) == ARG and "field_ids[2] repeats field_ids[0]" in err()
    assert call(1, out, 1, ids(0), None, None, p, None, None) == ARG and "dev_bytes is null" in err()
    assert call(1, out, 0, None, p, None, None, None, None) == ARG and "dev_bytes is given" in err()
    assert call(1, out, 0, None, None, None, None, None, None) == ARG and "no output" in err()
    assert call(1, out, 0, None, None, None, None, None, p) == ARG and "dev_obf is null" in err()
    assert call(1, out, 0, None, None, None, None, obfp, None) == ARG and "dev_nobf is null" in err()
    assert call(1, out, 0, None, None, None, None, hole, p) == ARG and "dev_obf[0]" in err()
    assert call(1, out, 0, None, None, p + 1, None, None, None) == ARG and "even" in err()
    assert call(1, out, 0, None, None, p, None, None, None) == 16
    rec, ctu = np.zeros(1, pkg.engine.PIC_MATCH_DTYPE), np.zeros(1, pkg.engine.CTU_MATCH_DTYPE)
    m = lambda n, a, b_, rp: L.match_emu(64, 64, n, a, b_, rp, ctu.ctypes.data)
    assert m(1, out, out, rec.ctypes.data) == 0
    assert m(0, out, out, rec.ctypes.data) == ARG and "n_pics" in err()
    assert m(1, None, out, rec.ctypes.data) == ARG and "dev_out_a is null" in err()
    assert m(1, out, None, rec.ctypes.data) == ARG and "dev_out_b is null" in err()
    assert m(1, out, hole, rec.ctypes.data) == ARG and "dev_out_b[0]" in err()
    assert m(1, hole, out, rec.ctypes.data) == ARG and "dev_out_a[0]" in err()
    assert m(1, out, out, None) == ARG and "host_matches" in err()


def test_layouts_match_the_library(built, pkg):
    e = pkg.engine
    L = C.CDLL(pkg.lib_path())
    assert L.fcu_abi_sizeof(11) == C.sizeof(e.CtuMatch) == e.CTU_MATCH_DTYPE.itemsize == 64
    assert L.fcu_abi_sizeof(12) == C.sizeof(e.PicMatch) == e.PIC_MATCH_DTYPE.itemsize == 208
    for cls, dt in ((e.CtuMatch, e.CTU_MATCH_DTYPE), (e.PicMatch, e.PIC_MATCH_DTYPE)):
        for name, _ in cls._fields_:                          # no implicit padding: the numpy and ctypes offsets agree field by field
            assert getattr(cls, name).offset == dt.fields[name][1], name
    emu = lib()
    for name, (fid, _, _, _) in maps_ref.FIELDS.items():     # the field table of fcu_host.h against the binding's structure
        assert emu.maps_emu_field_offset(fid) == maps_ref.field_offset(pkg, name) and e.MAP_FIELDS[name] == fid, name
    assert emu.maps_emu_field_offset(19) == -1 and emu.maps_emu_field_offset(-1) == -1 and len(e.MAP_FIELDS) == 19
    assert (e.LABEL_ABSENT, e.LABEL_NOT_SPLIT, e.LABEL_SPLIT, e.LABEL_FORCED) == (maps_ref.ABSENT, maps_ref.NOT_SPLIT, maps_ref.SPLIT, maps_ref.FORCED)


def test_drivers_keep_their_keys_without_the_option(pkg):
    """maps=None is the default of both drivers (the GPU tests check the result dicts)"""
    import inspect
    for cls in (pkg.lowdelay.LowDelayPDecider, pkg.sequence.SequenceDecider):
        assert inspect.signature(cls.__init__).parameters["maps"].default is None
