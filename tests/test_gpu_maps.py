"""GPU tests of the decision maps and the split match through the C ABI (fcu_decision_maps, fcu_split_match) and through CuEngine:
the emulator's cases with uploaded records (no decision is run), both store paths and bases moved by 2 bytes, a batch, stale
output buffers, the argument errors -- and real records: an I picture decided by SequenceDecider, a two-picture LowDelayPDecider
clip for the motion and ref_idx maps, and a Testing-state picture matched against its exhaustive decision."""
import ctypes as C

import numpy as np
import pytest
import torch

import maps_cases as MC
import maps_ref

pytestmark = pytest.mark.gpu
ARG = -2


def up(a, offset=0, fill=0):
    """the array's bytes on the device, the first one `offset` bytes into a fresh allocation (16-byte aligned itself)"""
    a = np.ascontiguousarray(a)
    buf = torch.full((a.nbytes + 64,), fill, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[offset:offset + a.nbytes]
    v.copy_(torch.from_numpy(a.reshape(-1).view(np.uint8).copy()))
    return v


def stale(nbytes, offset=0, fill=0xaa):
    buf = torch.full((nbytes + 64,), fill, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf[offset:offset + nbytes]


def host_maps(res, i, fields):
    """picture i of what CuEngine.decision_maps returned, as maps_ref.picture_maps lays it out"""
    d = {"bytes": np.stack([res[f][i].cpu().numpy().view(np.uint8) for f in fields]) if fields else None}
    if "mv" in res:
        d["mv"] = res["mv"][i].cpu().numpy()
    for k in ("labels", "n_obf"):
        if k in res:
            d[k] = [t[i].cpu().numpy() for t in res[k]]
    return d


def lib_maps(eng, w, h, recs, fields, mv, labels, obfs, offset=0, bufs=None):
    """fcu_decision_maps itself on caller-made buffers.  Returns (per-picture dicts, the buffers)"""
    n, H4, W4 = len(recs), h // 4, w // 4
    NL = sum(a * b for a, b in maps_ref.level_shapes(w, h))
    outs = (C.c_void_p * n)(*[r.data_ptr() for r in recs])
    ids = (C.c_int * max(len(fields), 1))(*[maps_ref.FIELDS[f][0] for f in fields])
    obfp = (C.c_void_p * n)(*[o.data_ptr() for o in obfs]) if obfs is not None else None
    bufs = bufs or {"bytes": stale(n * len(fields) * H4 * W4, offset) if fields else None, "mv": stale(n * H4 * W4 * 4, offset) if mv else None,
                    "labels": stale(n * NL) if labels else None, "n_obf": stale(n * NL * 2, offset) if obfs is not None else None}
    ptr = lambda k: bufs[k].data_ptr() if bufs[k] is not None else None
    rc = eng.lib.fcu_decision_maps(eng.h, n, outs, len(fields), ids, ptr("bytes"), ptr("mv"), ptr("labels"), obfp, ptr("n_obf"), None, None)
    assert rc == 0, eng.lib.fcu_last_error()
    hb = {k: (v.cpu().numpy() if v is not None else None) for k, v in bufs.items()}
    pics = []
    for i in range(n):
        d = {"bytes": hb["bytes"].reshape(n, len(fields), H4, W4)[i] if fields else None}
        if mv:
            d["mv"] = hb["mv"].view(np.int16).reshape(n, H4, W4, 2)[i]
        if labels:
            d["labels"] = maps_ref.split_levels(hb["labels"].view(np.int8).reshape(n, NL)[i], w, h)
        if obfs is not None:
            d["n_obf"] = maps_ref.split_levels(hb["n_obf"].view(np.uint16).reshape(n, NL)[i], w, h)
        pics.append(d)
    return pics, bufs


@pytest.mark.parametrize("fields", sorted(MC.FIELD_LISTS))
@pytest.mark.parametrize("w,h", MC.SIZES)
def test_emulator_cases_through_the_library_and_the_engine(w, h, fields, pkg):
    r, obf, want = MC.case(w, h, 11)
    names = MC.FIELD_LISTS[fields]
    eng = pkg.CuEngine(w, h, max_chains=1)
    d_r, d_obf = up(r), up(obf).view(torch.int16).view(h // 4, w // 4)
    got, _ = lib_maps(eng, w, h, [d_r], names, True, True, [d_obf])
    maps_ref.assert_maps_equal(got[0], MC.select(want, names), (w, h, fields, "library"))
    res, ms = eng.decision_maps([{"out": d_r}], fields=names, mv=True, labels=True, obf=[d_obf], timed=True)
    maps_ref.assert_maps_equal(host_maps(res, 0, names), MC.select(want, names), (w, h, fields, "engine"))
    assert ms >= 0 and res["depth"].dtype == torch.uint8 and (fields == "one" or res["part_size"].dtype == torch.int8)
    eng.destroy()


@pytest.mark.parametrize("offset", [2, 1])
def test_bases_moved_off_their_alignment(offset, pkg):
    """256x128 takes 16-byte rows when its bases are aligned (test above); with every base 2 bytes further the 2-byte units must
    give the same maps, and so must byte maps at an odd address"""
    w, h = 256, 128
    r, obf, want = MC.case(w, h, 11)
    eng = pkg.CuEngine(w, h, max_chains=1)
    d_r, d_obf = up(r), up(obf)
    if offset == 2:
        got, _ = lib_maps(eng, w, h, [d_r], MC.ALL_FIELDS, True, True, [d_obf], offset=2)
        maps_ref.assert_maps_equal(got[0], MC.select(want, MC.ALL_FIELDS), offset)
    else:
        got, _ = lib_maps(eng, w, h, [d_r], MC.ALL_FIELDS, False, False, None, offset=1)
        maps_ref.assert_maps_equal(got[0], MC.select(want, MC.ALL_FIELDS, False, False, False), offset)
    eng.destroy()


def test_batch_of_three_keeps_the_pictures_apart(pkg):
    w, h = 208, 136
    cases = [MC.case(w, h, s) for s in (11, 12, 13)]
    eng = pkg.CuEngine(w, h, max_chains=1)
    pics = [up(c[0]) for c in cases]
    obf = torch.stack([up(c[1]).view(torch.int16).view(h // 4, w // 4) for c in cases])
    res = eng.decision_maps(pics, fields=MC.MIXED_FIELDS, mv=True, labels=True, obf=obf)
    for i, c in enumerate(cases):
        maps_ref.assert_maps_equal(host_maps(res, i, MC.MIXED_FIELDS), MC.select(c[2], MC.MIXED_FIELDS), i)
    eng.destroy()


def test_repeated_call_gives_identical_bytes(pkg):
    """stale bytes underneath (0xaa, then 0x55): every byte is written, and a second call into the same buffers changes none"""
    w, h = 208, 136
    r, obf, want = MC.case(w, h, 11)
    eng = pkg.CuEngine(w, h, max_chains=1)
    d_r, d_obf = up(r), up(obf)
    got, bufs = lib_maps(eng, w, h, [d_r], MC.ALL_FIELDS, True, True, [d_obf])
    first = {k: v.cpu().numpy().tobytes() for k, v in bufs.items()}
    other, b55 = lib_maps(eng, w, h, [d_r], MC.ALL_FIELDS, True, True, [d_obf], bufs={k: stale(v.numel(), fill=0x55) for k, v in bufs.items()})
    assert {k: v.cpu().numpy().tobytes() for k, v in b55.items()} == first
    _, again = lib_maps(eng, w, h, [d_r], MC.ALL_FIELDS, True, True, [d_obf], bufs=bufs)
    assert {k: v.cpu().numpy().tobytes() for k, v in again.items()} == first
    maps_ref.assert_maps_equal(got[0], MC.select(want, MC.ALL_FIELDS))
    eng.destroy()


@pytest.mark.parametrize("w,h", MC.SIZES)
def test_split_match_of_the_emulator_cases(w, h, pkg):
    a, b, want = MC.match_case(w, h, 11, 12)
    eng = pkg.CuEngine(w, h, max_chains=1)
    da, db = up(a), up(b)
    got, ctu, ms = eng.split_match([da, da], [{"out": db}, da], ctu=True, timed=True)
    maps_ref.assert_match_equal(got[0], want, (w, h))
    assert got[1]["part_equal"] == got[1]["part_total"] == (w // 4) * (h // 4) and not got[1]["only_a"].any() and not got[1]["only_b"].any()
    assert not got[1]["node"][:, 0, 1].any() and not got[1]["node"][:, 1, 0].any() and got[1]["split_match"] == 1.0
    for k in maps_ref.MATCH_KEYS:
        assert np.array_equal(ctu[0][k].astype(np.int64).sum(axis=0), np.asarray(got[0][k]).astype(np.int64)), k
    assert len(ms) == 2 and all(m >= 0 for m in ms)
    again = eng.split_match([da], [db])                        # the context's own CTU buffer instead of the caller's
    maps_ref.assert_match_equal(again[0], want)
    eng.destroy()


def test_sequence_driver_maps_of_a_decided_picture(pkg):
    """208x136 I picture at QP 32 through SequenceDecider(maps=True): every map equals the reference applied to the records
    copied back, the depth map is r["depth"] with z-order undone, and the labels rebuild it"""
    w, h = 208, 136
    f = pkg.synth.mixed(w, h, seed=3)
    dec = pkg.sequence.SequenceDecider(w, h, 32, fast=False, maps=True)
    r = dec.decide(f)
    names = ("depth", "part_size", "pred_mode", "intra_dir_luma")
    records = r["out"].cpu().numpy()
    want = maps_ref.picture_maps(pkg, records, w, h, names, labels=True)
    got = {"bytes": np.stack([r["maps"][n].cpu().numpy().view(np.uint8) for n in names]), "labels": [t.cpu().numpy() for t in r["maps"]["labels"]]}
    maps_ref.assert_maps_equal(got, want)
    assert sorted(r["maps"]) == sorted(names + ("labels",))
    depth = r["maps"]["depth"].cpu().numpy()
    assert np.array_equal(maps_ref.depth_from_labels(got["labels"], w, h), depth) and depth.max() <= 3
    inside = MC.inside_entries(w, h)
    assert np.array_equal(np.bincount(depth.ravel(), minlength=4), np.bincount(r["depth"][inside], minlength=4))
    assert (r["maps"]["pred_mode"] == 1).all()                   # an I picture: MODE_INTRA everywhere
    dec.close()
    dec = pkg.sequence.SequenceDecider(w, h, 32, fast=False)
    assert "maps" not in dec.decide(f)
    dec.close()


def test_lowdelay_driver_motion_maps(pkg):
    """two pictures of a 208x136 clip through LowDelayPDecider(maps=True): the motion and ref_idx maps (and the others) equal the
    reference on the copied-back records; the P picture has inter CUs, so the motion map is not empty"""
    import search_trace as st
    w, h = 208, 136
    dec = pkg.lowdelay.LowDelayPDecider(w, h, 30, n_clips=1, search_range=8, maps=True)
    names = ("depth", "part_size", "pred_mode", "ref_idx")
    for poc in range(2):
        r = dec.decide_picture([st.moving_frame(pkg.synth, "mixed", w, h, 9, poc)])[0]
        want = maps_ref.picture_maps(pkg, r["out"].cpu().numpy(), w, h, names, mv=True, labels=True)
        got = {"bytes": np.stack([r["maps"][n].cpu().numpy().view(np.uint8) for n in names]), "mv": r["maps"]["mv"].cpu().numpy(),
               "labels": [t.cpu().numpy() for t in r["maps"]["labels"]]}
        maps_ref.assert_maps_equal(got, want, poc)
    ref_idx = r["maps"]["ref_idx"].cpu().numpy()
    assert ref_idx.dtype == np.int8 and (ref_idx == 0).any() and set(np.unique(ref_idx)) <= {-1, 0}
    assert got["mv"][ref_idx == 0].any()
    dec.close()
    dec = pkg.lowdelay.LowDelayPDecider(w, h, 30, n_clips=1, search_range=8)
    res = dec.decide_picture([st.moving_frame(pkg.synth, "mixed", w, h, 9, 0)])
    assert all(sorted(r) == ["first", "lambda", "out", "poc", "qp", "rec", "rec_unfiltered", "slice_type"] for r in res)
    dec.close()


def test_testing_state_against_the_exhaustive_decision(pkg):
    """one 208x136 picture decided twice in one launch -- exhaustively and in the fork's Testing state with pruning switches on --:
    the device's counts equal the reference's on the two copied-back record arrays, part_equal / part_total is the share of
    inside partitions of equal depth, and the N_OBF maps of the picture equal the reference on the copied-back OBF map"""
    w, h = 208, 136
    f = pkg.synth.mixed(w, h, seed=3)
    eng = pkg.CuEngine(w, h, max_chains=2)
    _, out_a = eng.init_chain(0, f, 32)
    _, out_b = eng.init_chain(1, f, 32)
    obf = eng.obf_prepass(eng.org_planes(1)[0])[0][0].contiguous()
    eng.set_decision(1, pkg.engine.TESTING, obf, (1, 1, 1, 1), (1, 1, 1, 1))
    eng.compress_chains(0, 2, eng.n_ctu)
    eng.sync()
    got = eng.split_match([out_a], [out_b])[0]
    ra, rb = out_a.cpu().numpy(), out_b.cpu().numpy()
    want = maps_ref.split_match(pkg, ra, rb, w, h)
    maps_ref.assert_match_equal(got, want)
    nb, inside = pkg.engine.CTU_OUT_BYTES, MC.inside_entries(w, h)
    da, db = ra.reshape(-1, nb)[:, :256], rb.reshape(-1, nb)[:, :256]
    assert got["split_match"] == float((da[inside] == db[inside]).mean()) and got["part_total"] == int(inside.sum())
    assert got["node"].sum() > 0
    res = eng.decision_maps([out_b], fields=(), labels=True, obf=[obf])
    want_b = maps_ref.picture_maps(pkg, rb, w, h, (), labels=True, obf=obf.cpu().numpy())
    maps_ref.assert_maps_equal(host_maps(res, 0, ()), want_b)
    eng.destroy()


def test_bad_arguments_name_the_argument(pkg):
    eng = pkg.CuEngine(64, 64, max_chains=1)
    lib = eng.lib
    r = up(MC.case(64, 64, 11)[0])
    obf = up(MC.case(64, 64, 11)[1])
    out, hole, obfp = (C.c_void_p * 1)(r.data_ptr()), (C.c_void_p * 1)(None), (C.c_void_p * 1)(obf.data_ptr())
    p = stale(4096).data_ptr()
    ids = lambda *v: (C.c_int * len(v))(*v)
    err = lambda: lib.fcu_last_error().decode()
    call = lambda n, o, nf, f, by, mv, lab, ob, nobf: lib.fcu_decision_maps(eng.h, n, o, nf, f, by, mv, lab, ob, nobf, None, None)
    assert call(1, out, 1, ids(0), p, None, None, None, None) == 0
    assert call(0, out, 1, ids(0), p, None, None, None, None) == ARG and "n_pics" in err()
    assert call(1, None, 1, ids(0), p, None, None, None, None) == ARG and "dev_out is null" in err()
    assert call(1, hole, 1, ids(0), p, None, None, None, None) == ARG and "dev_out[0]" in err()
    assert call(1, out, 1, None, p, None, None, None, None) == ARG and "field_ids is null" in err()
    assert call(1, out, 2, ids(0, 19), p, None, None, None, None) == ARG and "field_ids[1] = 19" in err()
    assert call(1, out, 3, ids(4, 0, 4), p, None, None, None, None) == ARG and "field_ids[2] repeats field_ids[0]" in err()
    assert call(1, out, 1, ids(0), None, None, p, None, None) == ARG and "dev_bytes is null" in err()
    assert call(1, out, 0, None, p, None, None, None, None) == ARG and "dev_bytes is given" in err()
    assert call(1, out, 0, None, None, None, None, None, None) == ARG and "no output" in err()
    assert call(1, out, 0, None, None, None, None, None, p) == ARG and "dev_obf is null" in err()
    assert call(1, out, 0, None, None, None, None, obfp, None) == ARG and "dev_nobf is null" in err()
    assert call(1, out, 0, None, None, None, None, hole, p) == ARG and "dev_obf[0]" in err()
    assert lib.fcu_decision_maps(None, 1, out, 1, ids(0), p, None, None, None, None, None, None) == ARG and "context" in err()
    rec = np.zeros(1, pkg.engine.PIC_MATCH_DTYPE)
    m = lambda n, a, b, rp: lib.fcu_split_match(eng.h, n, a, b, rp, None, None, None)
    assert m(1, out, out, rec.ctypes.data) == 0 and int(rec[0]["part_equal"]) == 256
    assert m(0, out, out, rec.ctypes.data) == ARG and "n_pics" in err()
    assert m(1, None, out, rec.ctypes.data) == ARG and "dev_out_a is null" in err()
    assert m(1, out, hole, rec.ctypes.data) == ARG and "dev_out_b[0]" in err()
    assert m(1, out, out, None) == ARG and "host_matches" in err()
    with pytest.raises(ValueError):
        eng.decision_maps([r], fields=("depht",))
    eng.destroy()
