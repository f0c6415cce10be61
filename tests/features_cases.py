"""Inputs of the feature-map tests, shared by the emulator tests (test_features.py) and the GPU tests (test_gpu_features.py): seeded
luma planes at the sizes of the decision-map cases, their thresholds, and the numpy reference (features_ref.py) computed once per
case and never modified."""
import functools

import numpy as np

import features_ref as FR
import hmo_py
from maps_cases import SIZES            # (208, 136), (72, 200), (64, 64), (8, 8), (256, 128): see maps_cases.py

KINDS = ("textured", "flat")
ALL = ("tmv", "soc")


def _pkg():
    import __graft_entry__ as g
    return g.load_package()


def luma(w, h, kind, seed=21):
    """textured: the synthetic texture with a 0 / 255 checkerboard patch (the largest filter responses and coefficients) and single
    samples 0 and 255 on block corners and edges; flat: one value with a one-sample step of 0 and of 255 in it"""
    rng = np.random.default_rng(seed)
    if kind == "textured":
        Y = np.array(_pkg().synth.textured(w, h, seed=seed)[0], np.uint8)
        ph, pw = min(h // 2, 12), min(w // 2, 20)                # (never the whole picture)
        yy, xx = np.mgrid[0:ph, 0:pw]
        Y[h - ph:, w - pw:] = np.where((yy + xx) & 1, 255, 0)
        for _ in range(max(4, w * h // 256)):
            Y[rng.integers(0, h), rng.integers(0, w)] = rng.choice([0, 255])
        Y[0, 0], Y[h - 1, w - 1], Y[0, w - 1], Y[h - 1, 0] = 0, 255, 255, 0
    else:
        Y = np.full((h, w), 117, np.uint8)
        Y[h // 2, w // 3] = 0
        Y[h // 3, w // 2] = 255
    return np.ascontiguousarray(Y)


def hand_yc(Y):
    """a hand-set Yc vector (integers, as the fit gives them) that puts coefficients exactly on the threshold: per frequency the
    most frequent non-zero |coef| that is a multiple of 8, divided by 8 (0 where there is none)"""
    c = np.abs(FR.dct4_blocks(Y))
    yc = np.zeros(16, np.float64)
    for k in range(1, 16):
        v = c[:, :, k].ravel()
        v = v[(v > 0) & (v % 8 == 0)]
        if v.size:
            yc[k] = np.bincount(v).argmax() / 8.0
    return yc


@functools.lru_cache(maxsize=None)
def case(w, h, kind, seed=21):
    """(Y, yc of the real TCM fit, hand-set yc, reference [NL, 146] with the fitted yc, reference SOC [NL, 16] with the hand-set yc)"""
    Y = luma(w, h, kind, seed)
    yh = hand_yc(Y)
    # the real TCM fit -- but for the textured 8x8 picture: on its four blocks per frequency the fit's lambda iteration runs for
    # minutes, in the oracle and in the library alike, so that one case takes its hand-set vector for both
    yc = yh if (kind == "textured" and w * h < 64 * 64) else np.ascontiguousarray(hmo_py.obf_prepass(Y)[1], np.float64)
    want = FR.feature_maps(Y, ALL, yc)
    want_hand = FR.feature_maps(Y, ("soc",), yh)
    for a in (Y, yc, yh, want, want_hand):
        a.setflags(write=False)
    return Y, yc, yh, want, want_hand


def select(want, sets):
    """the reference of a case narrowed to the sets asked for"""
    cols = ([*range(FR.TMV)] if "tmv" in sets else []) + ([*range(FR.TMV, FR.TMV + FR.SOC)] if "soc" in sets else [])
    return np.ascontiguousarray(want[:, cols])
