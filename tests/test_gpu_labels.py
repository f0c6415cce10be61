"""Caller-supplied split labels through the C ABI on the GPU (fcu_chain_set_labels, fcu_label_count, fcu_labels_from_rasters): the
cases of tests/test_labels.py -- same pictures, OBF maps, decisions and oracle references (tests/labels_testlib.py) -- with the
labels in HBM and no OBF map bound."""
import numpy as np
import pytest

import hmo_py
import labels_ref
import maps_ref
from labels_testlib import ALL_ON, CASE_QPS, CASES, DECISIONS, OBF_NAMES, P_BASE_QP, assert_verify_equal, inputs, obf_map, reference, sorted_ctx
from test_labels import I_CASE_QPS, assert_replay_equal
from tile_oracle import assert_picture_equal

pytestmark = pytest.mark.gpu


def _layout(pkg, case):
    w, h, kind, a, b, is_p = CASES[case]
    if kind == 1:
        return pkg.layout.PictureLayout(w, h, wpp=True)
    if kind == 2:
        return pkg.layout.PictureLayout(w, h, tiles=(a, b))
    return pkg.layout.PictureLayout(w, h, slice_ctus=a or None)


class Picture:
    """one case bound on the device: decide() runs it once with a state, labels (int8 array or device tensor), an OBF map or none"""

    def __init__(self, pkg, case, qp):
        import torch
        self.pkg, self.case, self.qp, self.torch = pkg, case, qp, torch
        self.w, self.h = CASES[case][:2]
        self.lo = _layout(pkg, case)
        self.eng = pkg.CuEngine(self.w, self.h, max_chains=self.lo.chains)
        self.f, self.p = inputs(pkg, case, qp)
        self.kw = {}
        if self.p is not None:
            fp = pkg.engine.ldp_slice(P_BASE_QP, 1)
            fp.search_range, fp.fast_search = self.p["sr"], self.p["fast"]
            assert fp.qp == qp
            self.kw = dict(params=fp, ref=self.eng.pad_reference([torch.as_tensor(q).cuda() for q in self.p["ref"]]))

    def decide(self, state, labels=None, obf=None, decision=None):
        eng, torch = self.eng, self.torch
        n, rec, out = eng.init_picture(0, self.f, self.qp, self.lo, **self.kw)
        sk, te, dex = decision if decision is not None else ((0,) * 4, (0,) * 4, 0)
        lab = None if labels is None else (labels if torch.is_tensor(labels) else torch.as_tensor(np.ascontiguousarray(labels, np.int8)).cuda())
        obf_dev = None if obf is None else torch.as_tensor(np.ascontiguousarray(obf, np.int16)).cuda()

        def set_decision():
            for k in range(n):
                eng.set_decision(k, state, obf_dev, sk, te, depth_exception=dex)

        def set_labels():
            if lab is not None:
                eng.set_labels(range(n), lab)
        for step in ((set_decision, set_labels) if obf is not None or state == hmo_py.TRAINING else (set_labels, set_decision)):
            step()
        eng.compress_pictures(0, 1, self.lo)
        eng.sync()
        return dict(out=out.cpu().numpy().tobytes(), out_dev=out, rec=[q.cpu().numpy() for q in rec], states=[eng.ctx_state(k, full=True) for k in range(n)],
                    verify=eng.verify_counts(0, n), trials=sum(eng.debug_counters(k)[16] for k in range(n)))

    def close(self):
        self.eng.destroy()


@pytest.fixture(params=CASE_QPS, ids=lambda c: "%s-%d" % c)
def picture(request, pkg):
    p = Picture(pkg, *request.param)
    yield p
    p.close()


@pytest.mark.parametrize("obf_name", OBF_NAMES)
def test_testing_state_from_labels_equals_the_oracle_on_the_obf_map(pkg, picture, obf_name):
    """labels bound and NO OBF map, Testing state, all switches on and two seeded per-depth patterns, depth_exception 0 and 1: every
    fcu_ctu_out field, the reconstruction and the coder state after every chain equal the oracle's run with the OBF map"""
    case, qp = picture.case, picture.qp
    lab = labels_ref.obf_labels(obf_map(case, obf_name), picture.w, picture.h)
    assert picture.eng.label_count() == lab.size
    for dec in DECISIONS:
        ref = reference(pkg, case, qp, hmo_py.TESTING, obf_name, dec)
        e = picture.decide(hmo_py.TESTING, labels=lab, decision=dec)
        assert_picture_equal(ref, e["out"], e["rec"], e["states"], sorted_ctx=sorted_ctx(case), tag=(case, qp, obf_name, dec))


@pytest.mark.parametrize("obf_name", OBF_NAMES)
def test_verifying_state_counts_the_labels_as_the_oracle_counts_the_obf_map(pkg, picture, obf_name):
    case, qp = picture.case, picture.qp
    lab = labels_ref.obf_labels(obf_map(case, obf_name), picture.w, picture.h)
    ref = reference(pkg, case, qp, hmo_py.VERIFYING, obf_name)
    e = picture.decide(hmo_py.VERIFYING, labels=lab)
    assert_picture_equal(ref, e["out"], e["rec"], e["states"], sorted_ctx=sorted_ctx(case), tag=(case, qp, obf_name))
    assert_verify_equal(e["verify"], ref.verify, (case, qp, obf_name))


def test_labels_take_the_place_of_a_bound_obf_map(pkg, picture):
    """fcu_chain_set_decision with an OBF map (all positive), then labels that say what the random map says: the labels decide"""
    case, qp = picture.case, picture.qp
    lab = labels_ref.obf_labels(obf_map(case, "random"), picture.w, picture.h)
    ref = reference(pkg, case, qp, hmo_py.TESTING, "random", DECISIONS[0])
    e = picture.decide(hmo_py.TESTING, labels=lab, obf=obf_map(case, "positive"), decision=DECISIONS[0])
    assert_picture_equal(ref, e["out"], e["rec"], e["states"], sorted_ctx=sorted_ctx(case), tag=(case, qp))


def test_no_prediction_is_the_exhaustive_search(pkg, picture):
    """all ABSENT: Testing with all switches on is the Training-state result bit for bit; Verifying counts nothing"""
    case, qp = picture.case, picture.qp
    lab = np.full(labels_ref.label_count(picture.w, picture.h), labels_ref.ABSENT, np.int8)
    ref = reference(pkg, case, qp, hmo_py.TRAINING)
    for state in (hmo_py.TESTING, hmo_py.VERIFYING):
        e = picture.decide(state, labels=lab, decision=(ALL_ON, ALL_ON, 0))
        assert_picture_equal(ref, e["out"], e["rec"], e["states"], sorted_ctx=sorted_ctx(case), tag=(case, qp, state))
        assert not e["verify"].any()


@pytest.mark.parametrize("case,qp", I_CASE_QPS)
def test_replay_of_an_i_pictures_own_labels_gives_the_exhaustive_decision(pkg, case, qp):
    """exhaustive decision -> its labels from fcu_decision_maps, never leaving the device -> Testing with all switches on: what
    tests/test_labels.py states for the emulator (every field but total_bits / total_cost, for the reason given there), and the
    split match of the two decisions is complete"""
    p = Picture(pkg, case, qp)
    try:
        ref = reference(pkg, case, qp, hmo_py.TRAINING)
        full = p.decide(hmo_py.TRAINING)
        assert_picture_equal(ref, full["out"], full["rec"], full["states"], tag=(case, qp, "exhaustive"))
        first = full["out_dev"].clone()
        lab = p.eng.decision_maps([first], fields=(), labels=True)["labels"]
        flat = p.torch.cat([m[0].reshape(-1) for m in lab]).contiguous()
        e = p.decide(hmo_py.TESTING, labels=flat, decision=(ALL_ON, ALL_ON, 0))
        assert_replay_equal(ref, e, (case, qp, "replay"))
        assert e["trials"] < full["trials"]
        m = p.eng.split_match([first], [e["out_dev"]])[0]
        assert m["part_equal"] == m["part_total"] and not m["only_a"].any() and not m["only_b"].any()
    finally:
        p.close()


@pytest.mark.parametrize("shift", [0, 1, 2])
@pytest.mark.parametrize("w,h", [(256, 128), (136, 72)])
def test_labels_from_the_rasters_of_a_decided_picture(pkg, w, h, shift):
    """fcu_labels_from_rasters on the depth / part_size maps fcu_decision_maps wrote for a decided picture equals the labels it
    wrote, and tests/labels_ref.py; all three bases moved by 0, 1 and 2 bytes; a second call over other stale bytes gives identical
    bytes and writes nothing outside; without part_size level 3 is NOT_SPLIT"""
    import torch
    eng = pkg.CuEngine(w, h, max_chains=1)
    try:
        f = pkg.synth.mixed(w, h, seed=4)
        _, out = eng.init_chain(0, f, qp=37)
        eng.compress_chains(0, 1, eng.n_ctu)
        eng.sync()
        maps = eng.decision_maps([out], fields=("depth", "part_size"), labels=True)
        want = torch.cat([m[0].reshape(-1) for m in maps["labels"]]).cpu().numpy()
        depth, part = maps["depth"][0].cpu().numpy(), maps["part_size"][0].cpu().numpy()
        assert np.array_equal(want, labels_ref.raster_labels(depth, part, w, h))
        NL, plane = eng.label_count(), (h // 4) * (w // 4)
        assert NL == labels_ref.label_count(w, h)
        depth2 = np.roll(depth, 16, axis=1)
        host_d, host_p = np.stack([depth, depth2]).reshape(-1), np.stack([part, part]).reshape(-1).view(np.uint8)

        def run(stale, with_part=True):
            bd, bp, bo = (torch.full((2 * n + shift + 8,), stale, dtype=torch.uint8, device="cuda") for n in (plane, plane, NL))
            bd[shift:shift + 2 * plane] = torch.as_tensor(host_d).cuda()
            bp[shift:shift + 2 * plane] = torch.as_tensor(host_p).cuda()
            d = bd[shift:shift + 2 * plane].view(2, h // 4, w // 4)
            ps = bp[shift:shift + 2 * plane].view(2, h // 4, w // 4) if with_part else None
            eng.labels_from_rasters(d, ps, out=bo[shift:shift + 2 * NL].view(torch.int8).view(2, NL))
            torch.cuda.synchronize()
            o = bo.cpu().numpy()
            assert np.all(o[:shift] == stale) and np.all(o[shift + 2 * NL:] == stale)
            return o[shift:shift + 2 * NL].view(np.int8).reshape(2, NL)
        got = run(0x33)
        assert np.array_equal(got[0], want) and np.array_equal(got[1], labels_ref.raster_labels(depth2, part, w, h))
        assert np.array_equal(run(0xC4), got)
        no_ps = run(0x33, with_part=False)
        assert np.array_equal(no_ps[0], labels_ref.raster_labels(depth, None, w, h))
        assert not (maps_ref.split_levels(no_ps[0], w, h)[3] == labels_ref.SPLIT).any()
    finally:
        eng.destroy()


def test_guards_through_the_abi(pkg):
    """fcu_chain_set_labels on a chain that is not bound; Verifying / Testing with neither an OBF map nor labels; unbinding the
    labels a Testing chain predicts from; NULL unbinds in Training"""
    import torch
    eng = pkg.CuEngine(128, 128, max_chains=1)
    try:
        lab = torch.zeros(eng.label_count(), dtype=torch.int8, device="cuda")
        assert eng.label_count() == 2 * 2 + 4 * 4 + 8 * 8 + 16 * 16
        with pytest.raises(pkg.FcuError, match="not bound"):
            eng.set_labels(0, lab)
        eng.init_chain(0, pkg.synth.mixed(128, 128, seed=9), qp=32)
        for state in (pkg.engine.VERIFYING, pkg.engine.TESTING):
            with pytest.raises(pkg.FcuError, match="OBF map"):
                eng.set_decision(0, state, None)
        eng.set_labels(0, None)
        eng.set_labels(0, lab)
        eng.set_decision(0, pkg.engine.TESTING, None, ALL_ON, ALL_ON)
        with pytest.raises(pkg.FcuError, match="cannot lose its labels"):
            eng.set_labels(0, None)
        eng.set_decision(0, pkg.engine.TRAINING)
        eng.set_labels(0, None)
    finally:
        eng.destroy()


def test_sequence_decider_runs_a_callers_labels(pkg):
    """SequenceDecider(labels=callable): the callable sees every Verifying and Testing picture with its planes and OBF map; labels
    that restate the Naive rule give the pictures, counters and switches of the run without labels; a callable that returns None
    leaves N_OBF in place"""
    import torch
    w, h, qp = 128, 128, 32
    frames = [pkg.synth.mixed(w, h, seed=s) for s in (9, 10, 11)]
    seen = []

    def naive(poc, planes, obf):
        assert len(planes) == 3 and planes[0].is_cuda and tuple(obf.shape) == (h // 4, w // 4)
        seen.append(poc)
        return torch.as_tensor(labels_ref.obf_labels(obf.cpu().numpy(), w, h)).cuda() if poc != 2 else None

    def run(labels):
        sched = pkg.sequence.FastDecisionSchedule(period=3, n_training=1, n_verifying=1, th_skip=(0.5,) * 4, th_term=(0.5,) * 4)
        dec = pkg.sequence.SequenceDecider(w, h, qp, fast=True, schedule=sched, labels=labels)
        try:
            res = [dec.decide(f) for f in frames]
            return [dict(r, out=r["out"].cpu().numpy().copy()) for r in res]
        finally:
            dec.close()
    a, b = run(None), run(naive)
    assert seen == [1, 2]
    assert [r["state"] for r in b] == [pkg.engine.TRAINING, pkg.engine.VERIFYING, pkg.engine.TESTING]
    assert "labels" in b[1] and "labels" not in b[0] and "labels" not in b[2]
    for x, y in zip(a, b):
        assert np.array_equal(x["out"], y["out"]) and np.array_equal(x["sw_skip"], y["sw_skip"]) and np.array_equal(x["sw_term"], y["sw_term"])
    assert np.array_equal(a[1]["verify"], b[1]["verify"]) and a[1]["verify"][:, :4].sum() > 0
