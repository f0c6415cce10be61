"""CuEngine.init_picture + compress_pictures against the low-level calls they are made of (init_chain per slice, set_range,
compress_chains), written out here: the fcu_ctu_out array and the three reconstruction planes byte for byte, no tolerance.
WPP and tile layouts have no second host path; the reference-parity tests of those features cover them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, QP = 256, 192, 32                                       # 4 x 3 CTUs


def _result(rec, out):
    return bytes(out.cpu().numpy()), [p.cpu().numpy() for p in rec]


def _same(got, want, what):
    assert got[0] == want[0], f"{what}: fcu_ctu_out"
    for k, (p, q) in enumerate(zip(got[1], want[1])):
        assert np.array_equal(p, q), f"{what}: reconstruction plane {k}"


def low_level(pkg, src, slice_ctus, **kw):
    """slice_ctus 0: one chain bound with slice_ctus 0; else one init_chain + set_range per slice.  kw: params / ref."""
    n_ctu = ((W + 63) // 64) * ((H + 63) // 64)
    n = (n_ctu + slice_ctus - 1) // slice_ctus if slice_ctus else 1
    eng = pkg.CuEngine(W, H, max_chains=n)
    planes = [eng.torch.as_tensor(a).cuda() for a in src]
    rec, out = eng.init_chain(0, planes, QP, slice_ctus=slice_ctus, **kw)
    for k in range(n if slice_ctus else 0):
        if k:
            eng.init_chain(k, planes, QP, slice_ctus=slice_ctus, rec=rec, out=out, **kw)
        eng.set_range(k, k * slice_ctus, min(slice_ctus, n_ctu - k * slice_ctus))
    eng.compress_chains(0, n, slice_ctus or n_ctu)
    eng.sync()
    res = _result(rec, out)
    pad = eng.pad_reference(rec)
    eng.destroy()
    return res, pad


def through_the_layout(pkg, src, slice_ctus, **kw):
    lo = pkg.layout.PictureLayout(W, H, slice_ctus=slice_ctus or None)
    eng = pkg.CuEngine(W, H, max_chains=lo.chains)
    n, rec, out = eng.init_picture(0, src, QP, lo, **kw)
    assert n == lo.chains == ((12 + slice_ctus - 1) // slice_ctus if slice_ctus else 1)
    eng.compress_pictures(0, 1, lo)
    eng.sync()
    assert all(eng.position(k) == min((k + 1) * lo.launch_ctus, 12) for k in range(n))
    res = _result(rec, out)
    eng.destroy()
    return res


@pytest.fixture(scope="module")
def src(pkg):
    return pkg.synth.mixed(W, H, seed=11)


@pytest.fixture(scope="module")
def one_slice(pkg, src):
    """the I picture through init_chain(slice_ctus=0) + compress_chains: (out bytes, rec planes), its padded reconstruction"""
    return low_level(pkg, src, 0)


def test_one_slice_i_picture(pkg, src, one_slice):
    _same(through_the_layout(pkg, src, 0), one_slice[0], "one slice")


@pytest.mark.parametrize("slice_ctus", [4, 5])                # whole rows; slices of 5, 5 and 2 CTUs that start mid-row
def test_slices_i_picture(pkg, src, slice_ctus):
    _same(through_the_layout(pkg, src, slice_ctus), low_level(pkg, src, slice_ctus)[0], f"slice_ctus {slice_ctus}")


def test_slices_p_picture(pkg, src, one_slice):
    """one reference picture: the padded reconstruction of the I picture"""
    nxt = [np.ascontiguousarray(np.roll(a, (1, 2 >> (1 if k else 0)), axis=(0, 1))) for k, a in enumerate(src)]
    kw = dict(params=pkg.engine.ldp_slice(QP, 1), ref=one_slice[1])
    want, got = low_level(pkg, nxt, 4, **kw)[0], through_the_layout(pkg, nxt, 4, **kw)
    _same(got, want, "P picture, slice_ctus 4")
    assert got[0] != one_slice[0][0]


def test_one_slice_sequence_decider(pkg, src, one_slice):
    """SequenceDecider used to bind a one-slice picture with slice_ctus = n_ctu and set_range(0, n_ctu); slice_ctus 0 decides the same"""
    dec = pkg.sequence.SequenceDecider(W, H, QP, fast=False, deblock=False)
    assert (dec.n_slices, dec.slice_ctus, dec.slice_mode) == (1, 12, "SliceMode 0 (one slice per picture)")
    r = dec.decide(src)
    _same(_result(r["rec"], r["out"]), one_slice[0], "SequenceDecider, one slice")
    dec.close()
