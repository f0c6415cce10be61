"""fcu_feature_maps on the device (libfcu.so, feat_ctu of csrc/fcu_features.h) against the numpy reference tests/features_ref.py:
the cases of tests/features_cases.py bit for bit, a stale buffer and a repeated call, a non-default stream, and the
SequenceDecider option."""
import numpy as np
import pytest

import features_cases as FC
import features_ref as FR

pytestmark = pytest.mark.gpu


def _dev(pkg, Y, offset=0):
    import torch
    raw = torch.zeros(Y.size + 64, dtype=torch.uint8, device="cuda")
    start = (-raw.data_ptr()) % 16 + offset
    t = raw[start:start + Y.size].view(Y.shape)
    t.copy_(torch.from_numpy(np.array(Y, np.uint8)))
    return t


@pytest.mark.parametrize("w,h", FC.SIZES)
def test_every_value_equals_the_reference(w, h, pkg):
    eng = pkg.CuEngine(w, h, max_chains=1)
    for kind in FC.KINDS:
        Y, yc, yh, want, want_hand = FC.case(w, h, kind)
        t = _dev(pkg, Y)
        for sets in (("tmv",), ("soc",), ("tmv", "soc")):
            got = eng.feature_maps([t], sets=sets, yc=[yc] if "soc" in sets else None)
            assert tuple(got.shape) == (1, eng.label_count(), len(pkg.engine.feature_columns(sets)))
            assert np.array_equal(got[0].cpu().numpy(), FC.select(want, sets)), (w, h, kind, sets)
        assert np.array_equal(eng.feature_maps([t], sets=("soc",), yc=[yh])[0].cpu().numpy(), want_hand), (w, h, kind, "hand-set yc")
        if kind == "textured" and w * h >= 64 * 64:           # the thresholds of the library's own pre-pass are the case's
            assert np.array_equal(eng.obf_prepass(t[None])[1][0], yc)
    eng.destroy()


def test_odd_byte_offsets_and_a_batch(pkg):
    w, h = 208, 136
    a, b = FC.case(w, h, "textured"), FC.case(w, h, "flat")
    eng = pkg.CuEngine(w, h, max_chains=1)
    for offset in (1, 4, 7):
        got = eng.feature_maps([_dev(pkg, a[0], offset), _dev(pkg, b[0], 8)], yc=[a[1], b[1]]).cpu().numpy()
        assert np.array_equal(got[0], a[3]) and np.array_equal(got[1], b[3]), offset
    eng.destroy()


def test_stale_buffer_repeat_and_stream(pkg):
    """the output tensor is torch.empty: fill the allocator's block with 0xaa first; a second call and a call on another stream give
    the same bytes"""
    import torch
    w, h = 208, 136
    Y, yc, _, want, _ = FC.case(w, h, "textured")
    eng = pkg.CuEngine(w, h, max_chains=1)
    t = _dev(pkg, Y)
    stale = torch.full((1, eng.label_count(), 146), float("nan"), dtype=torch.float32, device="cuda")
    stale.view(torch.uint8).fill_(0xaa)
    del stale                                                  # (the caching allocator hands the block to the next request of its size)
    first = eng.feature_maps([t], yc=[yc])
    assert np.array_equal(first[0].cpu().numpy(), want)
    again, ms = eng.feature_maps([t], yc=[yc], timed=True)
    assert torch.equal(first, again) and ms > 0
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        other = eng.feature_maps([t], yc=[yc], stream=st)
    st.synchronize()
    assert torch.equal(first, other)
    with pytest.raises(pkg.engine.FcuError, match="host_yc is null"):
        eng.feature_maps([t], sets=("soc",))
    eng.destroy()


def test_sequence_decider_features(pkg):
    """128 x 64 in Training with cu_trace and features: rows of the label maps, zeros where FORCED, equal to the call by hand, and the
    decision is the one of a run without the option"""
    import torch
    w, h = 128, 64
    yuv = pkg.synth.mixed(w, h, seed=3)
    dec = pkg.sequence.SequenceDecider(w, h, 32, fast=False, cu_trace=True, features=True)
    r = dec.decide(yuv)
    f = r["features"]
    assert tuple(f.shape) == (dec.eng.label_count(), 146) and f.dtype == torch.float32
    labels = dec.eng.trace_maps([r])["labels"][0]
    assert not f[labels == pkg.engine.LABEL_FORCED].any() and f[labels != pkg.engine.LABEL_FORCED].any()
    t = _dev(pkg, yuv[0])
    yc = dec.eng.obf_prepass(t[None])[1]
    assert torch.equal(f, dec.eng.feature_maps([t], yc=yc)[0])
    assert np.array_equal(f.cpu().numpy(), FR.feature_maps(yuv[0], FC.ALL, yc[0]))
    out = r["out"].cpu().numpy().copy()
    dec.close()
    plain = pkg.sequence.SequenceDecider(w, h, 32, fast=False)
    r0 = plain.decide(yuv)
    assert "features" not in r0 and np.array_equal(r0["out"].cpu().numpy(), out)
    plain.close()
    # a picture the edge cuts: its FORCED rows are zero
    w, h = 72, 40
    dec = pkg.sequence.SequenceDecider(w, h, 32, fast=False, cu_trace=True, features=("tmv",))
    r = dec.decide(pkg.synth.mixed(w, h, seed=3))
    labels = dec.eng.trace_maps([r])["labels"][0]
    assert tuple(r["features"].shape) == (dec.eng.label_count(), 130) and (labels == pkg.engine.LABEL_FORCED).any()
    assert not r["features"][labels == pkg.engine.LABEL_FORCED].any()
    dec.close()
