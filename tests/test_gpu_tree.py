"""The key tree through the C ABI on the GPU: the device cases of tests/tree_cases.py against the numpy reference
(tests/tree_ref.py), byte for byte.  Every output is poisoned with 0xA5, every entry point is called twice and the two results are
compared byte for byte."""
import ctypes as C

import numpy as np
import pytest

import labels_ref
import risk_ref
import tree_cases
import tree_ref

pytestmark = pytest.mark.gpu
SETS = {1: ("tmv",), 2: ("soc",), 3: ("tmv", "soc")}


def _dev(torch, a, dtype=None):
    t = torch.as_tensor(np.array(a).view(np.uint8).reshape(-1)).cuda()                 # (a writable copy: the cases are read-only)
    return t if dtype is None else t.view(dtype)


def _tree(pkg, t):
    k = pkg.engine.KeyTree()
    C.memmove(C.byref(k), np.ascontiguousarray(t).ctypes.data, 376)
    return k


def _twice(call, size, torch):
    """call(out) on two buffers poisoned with 0xA5; the two results must be the same bytes.  Returns the first as numpy uint8."""
    outs = []
    for _ in range(2):
        out = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
        call(out)
        outs.append(out.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()
    return outs[0]


def _hist(eng, torch, traces, bins, nodes, level, F, hist=None, accumulate=False):
    tr, bn = [_dev(torch, t) for t in traces], [_dev(torch, b) for b in bins]
    nd = [_dev(torch, k, torch.uint16) for k in nodes] if nodes is not None else None
    cells = 4 * (1 << level) * F * 64
    res = []
    for _ in range(1 if hist is not None else 2):
        h = hist if hist is not None else (torch.full((cells * 8,), 0xA5, dtype=torch.uint8, device="cuda").view(torch.int64).view(4, 1 << level, F, 32, 2),
                                           torch.full((cells * 4,), 0xA5, dtype=torch.uint8, device="cuda").view(torch.uint32).view(4, 1 << level, F, 32, 2))
        r, c, d = eng.tree_hist(tr, bn, level, nodes=nd, sets=SETS[3 if F == 146 else 2], hist=h, accumulate=accumulate)
        res.append((r, c, d))
    if len(res) == 2:
        assert res[0][0].cpu().numpy().tobytes() == res[1][0].cpu().numpy().tobytes() and res[0][1].cpu().numpy().tobytes() == res[1][1].cpu().numpy().tobytes() and res[0][2] == res[1][2]
    return res[0]


@pytest.mark.parametrize("size", tree_cases.BIN_SIZES, ids=lambda s: "%dx%d" % s)
def test_bins_and_keys_through_the_abi(pkg, size):
    import torch
    w, h = size
    X, E, B = tree_cases.bins_case(w, h)
    eng = pkg.CuEngine(w, h, max_chains=1)
    try:
        NL = eng.label_count()
        for name, (mask, cols) in tree_cases.SETS.items():
            Xs = torch.as_tensor(np.ascontiguousarray(np.stack([X[:, cols], X[:, cols]]))).cuda()
            Es = np.ascontiguousarray(E[:, cols])
            F = Xs.shape[2]
            want = np.ascontiguousarray(B[:, cols]).tobytes()
            for offset in (0, 1):                              # dev_bins at an even and at an odd byte
                def call(out):
                    eng.feature_bins(Xs, Es, sets=SETS[mask], out=out[offset:offset + 2 * NL * F])
                got = _twice(call, 2 * NL * F + 64, torch)
                assert np.all(got[:offset] == 0xA5) and np.all(got[offset + 2 * NL * F:] == 0xA5)
                assert got[offset:offset + NL * F].tobytes() == want and got[offset + NL * F:offset + 2 * NL * F].tobytes() == want, (name, offset)
        if size == (208, 136):
            for levels, walk in ((0, 0), (1, 1), (3, 3), (5, 5), (5, 2), (3, 0)):
                Bc, t, K = tree_cases.keys_case(w, h, levels, walk)
                db = torch.as_tensor(np.stack([Bc, Bc[::-1]])).cuda()
                k1 = eng.tree_keys(db, _tree(pkg, t), walk).cpu().numpy()
                k2 = eng.tree_keys(db, _tree(pkg, t), walk).cpu().numpy()
                assert k1.tobytes() == k2.tobytes() and k1[0].tobytes() == K.tobytes() and k1[1].tobytes() == tree_ref.keys(Bc[::-1], t, walk, w, h).tobytes(), (levels, walk)
    finally:
        eng.destroy()


@pytest.mark.parametrize("level", tree_cases.HIST_LEVELS)
@pytest.mark.parametrize("size,F", [((208, 136), 146), ((64, 64), 16)], ids=["208x136-146", "64x64-16"])
def test_hist_through_the_abi(pkg, size, F, level):
    import torch
    w, h = size
    traces, bins, nodes, risk, count, dropped = tree_cases.hist_case(w, h, 2, level, F)
    eng = pkg.CuEngine(w, h, max_chains=1)
    try:
        r, c, d = _hist(eng, torch, traces, bins, nodes, level, F)
        assert r.cpu().numpy().tobytes() == risk.tobytes() and c.cpu().numpy().tobytes() == count.tobytes() and d == dropped
        a = _hist(eng, torch, traces[:1], bins[:1], nodes[:1] if nodes else None, level, F)
        b = _hist(eng, torch, traces[1:], bins[1:], nodes[1:] if nodes else None, level, F, hist=a[:2], accumulate=True)
        assert b[0].cpu().numpy().tobytes() == risk.tobytes() and b[1].cpu().numpy().tobytes() == count.tobytes() and a[2] + b[2] == dropped
        if F == 146 and level == 2:                            # the cross-check with fcu_risk_train on the node array
            model, _ = eng.risk_train([_dev(torch, t) for t in traces], [_dev(torch, k, torch.uint16) for k in nodes])
            m = model.cpu().numpy().view(risk_ref.MODEL)[0]
            rr, cc = r.cpu().numpy(), c.cpu().numpy()
            for f in range(F):
                assert np.array_equal(rr[:, :, f].sum(axis=2), m["risk"][:, :4]) and np.array_equal(cc[:, :, f].sum(axis=2), m["count"][:, :4]), f
    finally:
        eng.destroy()


@pytest.mark.parametrize("level", (0, 4))
def test_strips_and_all_depths_through_the_abi(pkg, level):
    import torch
    for (w, h), case in ((tree_cases.STRIP, tree_cases.strip_case(level)), ((192, 128), tree_cases.all_depths_case(level))):
        traces, bins, nodes, risk, count, dropped = case
        eng = pkg.CuEngine(w, h, max_chains=1)
        try:
            r, c, d = _hist(eng, torch, traces, bins, nodes, level, 146)
            assert r.cpu().numpy().tobytes() == risk.tobytes() and c.cpu().numpy().tobytes() == count.tobytes() and d == dropped, (w, h)
        finally:
            eng.destroy()


def test_strip_bins_and_keys_through_the_abi(pkg):
    import torch
    w, h = tree_cases.STRIP
    NL = labels_ref.label_count(w, h)
    rng = np.random.default_rng(4)
    X = rng.integers(-40, 40, (2, NL, 16)).astype(np.float32)
    E = np.sort(rng.integers(-40, 40, (4, 16, 31)), axis=2).astype(np.float32)
    t = tree_cases.hand_tree(5, 16, 77)
    eng = pkg.CuEngine(w, h, max_chains=1)
    try:
        got = _twice(lambda out: eng.feature_bins(torch.as_tensor(X).cuda(), E, sets=("soc",), out=out[1:1 + X.size]), X.size + 8, torch)
        B = got[1:1 + X.size].reshape(X.shape)
        assert all(B[i].tobytes() == tree_ref.bins(X[i], E, w, h).tobytes() for i in range(2)) and got[0] == 0xA5 and np.all(got[1 + X.size:] == 0xA5)
        K = [eng.tree_keys(torch.as_tensor(B.copy()).cuda(), _tree(pkg, t), 5, sets=("soc",)).cpu().numpy() for _ in range(2)]
        assert K[0].tobytes() == K[1].tobytes() and all(K[0][i].tobytes() == tree_ref.keys(B[i], t, 5, w, h).tobytes() for i in range(2))
    finally:
        eng.destroy()


@pytest.mark.parametrize("rule", ["one", "two"])
def test_planted_rule_through_the_abi(pkg, rule):
    import torch
    w, h = tree_cases.PLANTED_SIZE[rule]
    tr, B, nobf_keys, tree, K = tree_cases.planted_case(rule)
    eng = pkg.CuEngine(w, h, max_chains=1)
    try:
        dtr, db = [_dev(torch, tr)], torch.as_tensor(np.array(B)).cuda()[None]
        t1, t2 = eng.tree_train(dtr, db, int(tree["levels"])), eng.tree_train(dtr, db, int(tree["levels"]))
        assert bytes(t1) == bytes(t2) == tree.tobytes()
        keys = eng.tree_keys(db, t1)
        assert keys.cpu().numpy()[0].tobytes() == K.tobytes()
        model, dropped = eng.risk_train(dtr, keys)
        assert dropped == 0 and sum(tree_ref.table_loss(model.cpu().numpy().view(risk_ref.MODEL)[0])) == 0
    finally:
        eng.destroy()


def test_real_picture_monotone_and_a_testing_picture_runs(pkg):
    """128 x 64 decided exhaustively with a trace bound; features, default edges, tree_train with 0..5 levels, keys, risk_train: the
    integer training loss per depth never increases; then risk_predict and the labels run a Testing picture to the end"""
    import torch
    w, h, qp = 128, 64, 32
    eng = pkg.CuEngine(w, h, max_chains=1)
    try:
        Y, U, V = pkg.synth.mixed(w, h, seed=9)
        eng.init_chain(0, (Y, U, V), qp)
        trace = eng.enable_cu_trace(0)
        eng.compress_chains(0, 1, eng.n_ctu)
        eng.sync()
        luma = eng.org_planes(0)[0]
        X = eng.feature_maps([luma], yc=eng.obf_prepass(luma)[1])
        E = pkg.engine.feature_edges(X, w, h)
        assert E.cpu().numpy().tobytes() == pkg.engine.feature_edges(X, w, h).cpu().numpy().tobytes()
        En = E.cpu().numpy()
        assert En.shape == (4, 146, 31) and np.isfinite(En).all() and np.all(np.diff(En, axis=2) >= 0)
        B = eng.feature_bins(X, E)
        assert B.cpu().numpy()[0].tobytes() == tree_ref.bins(X.cpu().numpy()[0], En, w, h).tobytes()
        host_tr, host_b = eng.cu_trace_array(trace).copy(), B.cpu().numpy()[0]
        prev = None
        for levels in range(6):
            t = eng.tree_train([trace], B, levels)
            assert bytes(t) == tree_ref.train([host_tr], [host_b], levels, 1, w, h).tobytes(), levels
            keys = eng.tree_keys(B, t)
            model, dropped = eng.risk_train([trace], keys)
            loss = tree_ref.table_loss(model.cpu().numpy().view(risk_ref.MODEL)[0])
            print("levels %d: loss per depth %s" % (levels, loss))
            m = model.cpu().numpy().view(risk_ref.MODEL)[0]
            if levels == 0:
                assert loss == [int(min(m["risk"][d, 0, 0], m["risk"][d, 0, 1])) for d in range(4)]
            else:
                assert all(a <= b for a, b in zip(loss, prev)), (levels, loss, prev)
            prev = loss
        assert dropped == 0
        Y2, U2, V2 = pkg.synth.mixed(w, h, seed=10)
        eng.init_chain(0, (Y2, U2, V2), qp)
        luma2 = eng.org_planes(0)[0]
        obf, yc, _ = eng.obf_prepass(luma2)
        k2 = eng.tree_keys(eng.feature_bins(eng.feature_maps([luma2], yc=yc), E), t)
        lab = eng.risk_predict(k2, model, 1)[0]
        eng.set_decision(0, pkg.engine.TESTING, obf[0].contiguous(), (1, 1, 1, 1), (1, 1, 1, 1))
        eng.set_labels([0], lab)
        eng.compress_chains(0, 1, eng.n_ctu)
        eng.sync()
        assert eng.position(0) == eng.n_ctu
    finally:
        eng.destroy()


def test_guards_through_the_abi(pkg):
    import torch
    w, h = 64, 64
    eng = pkg.CuEngine(w, h, max_chains=1)
    try:
        L, hd = eng.lib, eng.h
        NL = eng.label_count()
        assert L.fcu_abi_sizeof(18) == C.sizeof(pkg.engine.KeyTree) == 376
        traces, bins, nodes, _, _, _ = tree_cases.hist_case(w, h, 2, 2, 16)
        tr, bn, nd = _dev(torch, traces[0]), _dev(torch, bins[0]), _dev(torch, nodes[0], torch.uint16)
        X, E = torch.zeros((NL, 16), dtype=torch.float32, device="cuda"), torch.zeros((4, 16, 31), dtype=torch.float32, device="cuda")
        out = torch.zeros(NL * 16 + 16, dtype=torch.uint8, device="cuda")
        xp, ep, op, bp = X.data_ptr(), E.data_ptr(), out.data_ptr(), bn.data_ptr()
        for args, word in (((0, 2, xp, ep, op), b"n_pics"), ((1, 4, xp, ep, op), b"sets"), ((1, 2, None, ep, op), b"dev_features is null"), ((1, 2, xp + 2, ep, op), b"dev_features starts"),
                           ((1, 2, xp, None, op), b"dev_edges is null"), ((1, 2, xp, ep, None), b"dev_bins is null"), (((1 << 22) // NL + 1, 2, xp, ep, op), b"2^22")):
            assert L.fcu_feature_bins(hd, *args, None, None) == -2 and word in L.fcu_last_error(), word
        t = _tree(pkg, tree_cases.hand_tree(3, 16, 1))
        bad = _tree(pkg, tree_cases.hand_tree(3, 16, 1))
        bad.feature[2][5] = 16
        tp, kp = C.addressof(t), out.data_ptr()
        for args, word in (((0, 2, bp, tp, 3, kp), b"n_pics"), ((1, 2, None, tp, 3, kp), b"dev_bins is null"), ((1, 2, bp, None, 3, kp), b"host_tree is null"), ((1, 2, bp, C.addressof(bad), 3, kp), b"feature"),
                           ((1, 2, bp, tp, 4, kp), b"levels is 0"), ((1, 2, bp, tp, 3, None), b"dev_keys is null"), ((1, 2, bp, tp, 3, kp + 1), b"even byte")):
            assert L.fcu_tree_keys(hd, *args, None, None) == -2 and word in L.fcu_last_error(), word
        one, b1, n1, none = (C.c_void_p * 1)(tr.data_ptr()), (C.c_void_p * 1)(bp), (C.c_void_p * 1)(nd.data_ptr()), (C.c_void_p * 1)(None)
        r, c = torch.zeros((4, 4, 16, 32, 2), dtype=torch.int64, device="cuda"), torch.zeros((4, 4, 16, 32, 2), dtype=torch.uint32, device="cuda")
        rp, cp = r.data_ptr(), c.data_ptr()
        for args, word in (((0, 2, 2, one, b1, n1, rp, cp, 0), b"n_pics"), ((1, 2, 5, one, b1, n1, rp, cp, 0), b"level is"), ((1, 2, 2, None, b1, n1, rp, cp, 0), b"dev_trace is null"),
                           ((1, 2, 2, one, b1, None, rp, cp, 0), b"dev_nodes is null"), ((1, 2, 2, none, b1, n1, rp, cp, 0), b"dev_trace[0]"), ((1, 2, 2, one, none, n1, rp, cp, 0), b"dev_bins[0]"),
                           ((1, 2, 2, one, b1, n1, rp + 4, cp, 0), b"dev_risk starts"), ((1, 2, 2, one, b1, n1, rp, cp + 2, 0), b"dev_count starts"), ((1, 2, 2, one, b1, n1, rp, cp, 2), b"accumulate")):
            assert L.fcu_tree_hist(hd, *args, None, None, None) == -2 and word in L.fcu_last_error(), word
        for args, word in (((0, 2, 2, 1, one, b1, tp), b"n_pics"), ((1, 2, 6, 1, one, b1, tp), b"levels is"), ((1, 2, 2, -1, one, b1, tp), b"min_count"), ((1, 2, 2, 1, one, none, tp), b"dev_bins[0]"),
                           ((1, 2, 2, 1, one, b1, None), b"host_tree is null")):
            assert L.fcu_tree_train(hd, *args, None, None) == -2 and word in L.fcu_last_error(), word
        bad_e = np.zeros((4, 16, 31), np.float32)
        bad_e[1, 2, 3] = np.nan
        with pytest.raises(pkg.engine.FcuError, match="host_edges"):
            eng.feature_bins(X[None], bad_e, sets=("soc",))
    finally:
        eng.destroy()


def test_sequence_decider_runs_the_schedule_on_the_tree(pkg):
    """128x64, four pictures, period 4 = 2 Training + 1 Verifying + 1 Testing with risk={"tree": ...}: the labels of the Verifying
    and the Testing picture equal what the same steps give when called by hand on the Training pictures' traces"""
    import torch
    w, h, qp = 128, 64, 32
    frames = [pkg.synth.mixed(w, h, seed=s) for s in (9, 10, 11, 12)]
    sched = pkg.sequence.FastDecisionSchedule(period=4, n_training=2, n_verifying=1)
    dec = pkg.sequence.SequenceDecider(w, h, qp, fast=True, schedule=sched, risk={"tree": {"levels": 3, "min_count": 2}})
    try:
        res = [dec.decide(f) for f in frames]
        eng = dec.eng
        assert [r["state"] for r in res] == [pkg.sequence.TRAINING] * 2 + [pkg.sequence.VERIFYING, pkg.sequence.TESTING]
        assert all("labels" not in r for r in res[:2]) and all("labels" in r for r in res[2:]) and dec.key_tree.levels == 3

        def feats(f):
            luma = torch.as_tensor(f[0]).cuda()
            return eng.feature_maps([luma], yc=eng.obf_prepass(luma)[1])
        X = torch.cat([feats(f) for f in frames[:2]])
        E = pkg.engine.feature_edges(X, w, h)
        assert E.cpu().numpy().tobytes() == dec.tree_edges.cpu().numpy().tobytes()
        B = eng.feature_bins(X, E)
        traces = [r["cu_trace"] for r in res[:2]]
        tree = eng.tree_train(traces, B, 3, 2)
        assert bytes(tree) == bytes(dec.key_tree)
        host = tree_ref.train([eng.cu_trace_array(t).copy() for t in traces], list(B.cpu().numpy()), 3, 2, w, h)
        assert bytes(tree) == host.tobytes() and (host["feature"][:, 0] >= 0).any()
        model, _ = eng.risk_train(traces, eng.tree_keys(B, tree))
        assert model.cpu().numpy().tobytes() == dec.risk_model.cpu().numpy().tobytes()
        for i in (2, 3):
            lab = eng.risk_predict(eng.tree_keys(eng.feature_bins(feats(frames[i]), E), tree), model, 1)[0]
            assert lab.cpu().numpy().tobytes() == res[i]["labels"].cpu().numpy().tobytes(), i
        assert res[2]["verify"][:, :4].sum() > 0
    finally:
        dec.close()
