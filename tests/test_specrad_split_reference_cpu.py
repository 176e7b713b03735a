"""The split-operand squaring (tests/specrad_split_ref.py: two float16 pieces per operand, three float32-accumulated
products per squaring) against the float64 restatement and against np.linalg.eigvals on the shared matrix set, with
no GPU.

Bounds: 5e-7 relative of the restatement at the same K (the two pieces carry 22 bits, 2^-22 = 2.4e-7, and the
2^(K-1) divisor suppresses all but the last squarings' rounding; measured 2.1e-7); 1e-6 of eigvals at K = 24, the
bound the float64 kernel is held to; and a single piece is worse than 1e-5, which is what the second piece buys."""
import numpy as np
import pytest

import specrad_ref as sr
import specrad_split_ref as ss

CASES = sr.cases()


@pytest.fixture(scope="module")
def mats():
    out = {}
    for c in CASES:
        w = sr.reference_matrix(*c)
        w.setflags(write=False)
        out[c] = (w, float(np.max(np.abs(np.linalg.eigvals(w)))))
    return out


@pytest.fixture(scope="module")
def split24(mats):
    return {c: ss.specrad_split(mats[c][0], 24) for c in CASES}


@pytest.mark.parametrize("k", [16, 24])
def test_split_emulation_matches_the_restatement_at_the_same_k(mats, split24, k):
    worst = 0.0
    for c in CASES:
        want, st_w = sr.specrad(mats[c][0], k)
        got, st = split24[c] if k == 24 else ss.specrad_split(mats[c][0], k)
        assert st == 0 and st_w == 0, c
        rel = abs(got - want) / want
        worst = max(worst, rel)
        assert rel <= 5e-7, (c, k, rel)
    print(f"split emulation vs restatement, K = {k}: worst relative {worst:.2e} over {len(CASES)} matrices")


def test_split_emulation_matches_eigvals_at_24_squarings(mats, split24):
    worst = 0.0
    for c in CASES:
        got, st = split24[c]
        assert st == 0, c
        rel = abs(got - mats[c][1]) / mats[c][1]
        worst = max(worst, rel)
        assert rel <= 1e-6, (c, rel)
    print(f"split emulation vs eigvals, K = 24: worst relative {worst:.2e}")


def test_a_single_float16_piece_is_not_enough(mats):
    worst = 0.0
    for c in CASES:
        got, st = ss.specrad_split(mats[c][0], 24, with_lo=False)
        assert st == 0, c
        worst = max(worst, abs(got - mats[c][1]) / mats[c][1])
    print(f"one float16 piece vs eigvals, K = 24: worst relative {worst:.2e}")
    assert worst > 1e-5


def test_scale_depends_on_n_alone_and_keeps_the_operands_inside_float16():
    assert [ss.scale(n) for n in (1, 5, 64, 65, 128, 130, 300, 512, 577, 4096)] == \
        [16.0, 16.0, 16.0, 32.0, 32.0, 64.0, 128.0, 128.0, 256.0, 1024.0]
    assert ss.scale(4096) < np.finfo(np.float16).max            # |b_ij| <= |B| <= 1


def test_zero_and_nilpotent_matrices_are_flagged():
    assert ss.specrad_split(np.zeros((33, 33))) == (0.0, 1)
    assert ss.specrad_split(np.triu(np.ones((33, 33)), 1)) == (0.0, 1)
