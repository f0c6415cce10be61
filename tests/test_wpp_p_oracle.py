"""Properties of the test-side P-slice WaveFrontSynchro reference (tests/wpp_oracle.py) on the unchanged oracle: row 0 is the
plain one-slice run, and its fixtures are sensitive to the TZ search state (m_integerMv2Nx2N) a partial bottom row takes from
the row above and a picture takes from the picture before."""
import numpy as np
import pytest

import hmo_py
from wpp_oracle import WppOracle, wpp_p_clip


def split_motion_clip(w, h, n_pic, seed, v=(14, 8), still=None):
    """noise texture in which everything moves by v samples per picture, except the rectangle still = (x0, y0, x1, y1) (luma
    samples), which stays put.  A TZ search whose predictors come from the still part starts far from the motion of the rest,
    so the carried start vector decides where it ends."""
    rng = np.random.default_rng(seed)
    m = 16 * n_pic + 16
    k = np.ones(3) / 3
    base = rng.integers(0, 256, (h + 2 * m, w + 2 * m)).astype(np.float64)
    base = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 1, base)
    base = np.clip(base, 0, 255).astype(np.uint8)
    cb = rng.integers(64, 192, ((h + 2 * m) // 2, (w + 2 * m) // 2)).astype(np.uint8)
    cr = rng.integers(64, 192, ((h + 2 * m) // 2, (w + 2 * m) // 2)).astype(np.uint8)
    frames = []
    for t in range(n_pic):
        dx, dy = v[0] * t, v[1] * t
        Y = base[m - dy:m - dy + h, m - dx:m - dx + w].copy()
        U = cb[(m - dy) // 2:(m - dy) // 2 + h // 2, (m - dx) // 2:(m - dx) // 2 + w // 2].copy()
        V = cr[(m - dy) // 2:(m - dy) // 2 + h // 2, (m - dx) // 2:(m - dx) // 2 + w // 2].copy()
        if still is not None:
            x0, y0, x1, y1 = still
            Y[y0:y1, x0:x1] = base[m + y0:m + y1, m + x0:m + x1]
            U[y0 // 2:y1 // 2, x0 // 2:x1 // 2] = cb[m // 2 + y0 // 2:m // 2 + y1 // 2, m // 2 + x0 // 2:m // 2 + x1 // 2]
            V[y0 // 2:y1 // 2, x0 // 2:x1 // 2] = cr[m // 2 + y0 // 2:m // 2 + y1 // 2, m // 2 + x0 // 2:m // 2 + x1 // 2]
        frames.append((np.ascontiguousarray(Y), np.ascontiguousarray(U), np.ascontiguousarray(V)))
    return frames


def _differs(a, b):
    return [x["ctus"] != y["ctus"] for x, y in zip(a, b)]


@pytest.mark.parametrize("gen,w,h,base_qp,fast", [("mixed", 256, 192, 32, 1), ("shear_mixed", 192, 112, 27, 1), ("textured", 192, 128, 32, 0)])
def test_row_zero_is_the_plain_one_slice_run(built, pkg, gen, w, h, base_qp, fast):
    import search_trace as st
    f0, f1 = [st.moving_frame(pkg.synth, gen, w, h, 11, poc) for poc in range(2)]
    prev = wpp_p_clip([f0], base_qp)[0]["rec"]
    _, qp, lam = hmo_py.ldp_slice(1, base_qp)
    state = [(3, -1), (0, 0), (0, 0), (0, 0)]
    kw = dict(ref=prev, lambda_override=lam, search_range=16, fast_search=fast)
    o = WppOracle(*f1, qp, int_mv=state, **kw).run()
    ref = hmo_py.Encoder(*f1, qp, **kw)
    ref.set_int_mv(state)
    for a in range(o.W):
        ref.compress_ctu(a)
        A, B = ref.ctu_arrays(a), o.enc.ctu_arrays(a)
        for k, v in A.items():
            assert np.array_equal(v, B[k]) if isinstance(v, np.ndarray) else v == B[k], (a, k)
    assert np.array_equal(ref.cabac(full=True)[0], o.row_state[0][0]) and ref.cabac(full=True)[1] == o.row_state[0][1]
    assert ref.test_int_mv() == o.row_int_mv[0]


# (w, h, still rectangle): the upper rows' left part stays put, the rest -- the end of the row above, the bottom row -- moves
BOTTOM = [(256, 112, (0, 0, 128, 64)), (192, 176, (0, 0, 128, 128))]


@pytest.mark.parametrize("w,h,still", BOTTOM)
def test_partial_bottom_row_depends_on_the_row_above(built, pkg, w, h, still):
    """the partial bottom row starts its first TZ search from the row above's final state; from a zeroed one some CTU differs"""
    frames = split_motion_clip(w, h, 3, 5, still=still)
    rp = lambda poc, n: pkg.lowdelay.ref_pocs(poc, n, "recent")
    kw = dict(ref_pocs=rp, n_refs=2, search_range=64, fast_search=1, amp=1, tmvp=0)
    carried, zeroed = wpp_p_clip(frames, 30, **kw), wpp_p_clip(frames, 30, zero_bottom=True, **kw)
    d = _differs(carried, zeroed)
    assert not d[0] and any(d[1:]), d


def test_picture_start_depends_on_the_picture_before(built, pkg):
    """192x48: one partial row, so the picture's first TZ search starts from what the picture before left"""
    frames = split_motion_clip(192, 48, 4, 3)
    kw = dict(search_range=64, fast_search=1)
    carried, zeroed = wpp_p_clip(frames, 30, **kw), wpp_p_clip(frames, 30, zero_start=(2, 3), **kw)
    assert carried[1]["int_mv"] != [(0, 0)] * 4
    d = _differs(carried, zeroed)
    assert not d[0] and not d[1] and any(d[2:]), d
