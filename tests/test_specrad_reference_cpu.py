"""The spectral radius by repeated squaring, as the device computes it (include/esn_hip.h, esn_spectral_radius_batch),
restated in NumPy (tests/specrad_ref.py) and held against max|np.linalg.eigvals| on the reference's own matrices
(rand - 0.5 with the sparsity mask, pyESN.py:96-100).  Bounds: 1e-6 relative at K = 24 -- 16 x the worst 6.3e-8 measured
over 498 such matrices (the residual is the cos(2^k theta) beat of a dominant complex pair and halves with
each squaring) -- and 1e-5 at K = 20 (measured 8.5e-7).  Every matrix is checked; none is skipped."""
import numpy as np
import pytest

import specrad_ref as sr

CASES = sr.cases()


@pytest.fixture(scope="module")
def eig_radius():
    return {c: float(np.max(np.abs(np.linalg.eigvals(sr.reference_matrix(*c))))) for c in CASES}


def test_case_set_is_the_one_the_bounds_were_stated_for():
    assert len(CASES) == len(sr.SIZES) * len(sr.SPARSITIES) * sr.N_SEEDS + 1
    assert {c[0] for c in CASES} == set(sr.SIZES) | {512}
    assert {c[1] for c in CASES} == set(sr.SPARSITIES)


@pytest.mark.parametrize("k, bound", [(24, 1e-6), (20, 1e-5)])
def test_restatement_matches_eigvals_on_every_matrix(eig_radius, k, bound):
    worst = 0.0
    for c in CASES:
        want = eig_radius[c]
        assert want > 0.0, c
        got, status = sr.specrad(sr.reference_matrix(*c), k)
        assert status == 0, c
        rel = abs(got - want) / want
        worst = max(worst, rel)
        assert rel <= bound, (c, k, rel)
    print(f"K = {k}: worst relative error against eigvals {worst:.2e} over {len(CASES)} matrices")


def test_zero_and_nilpotent_matrices_report_failure():
    assert sr.specrad(np.zeros((7, 7))) == (0.0, 1)
    assert sr.specrad(np.triu(np.ones((6, 6)), 1)) == (0.0, 1)        # strictly upper triangular: W^6 = 0
    assert not sr.has_cycle(np.triu(np.ones((6, 6)), 1)) and sr.has_cycle(np.eye(3))


def test_diagonal_matrix_returns_its_largest_modulus():
    d = np.array([0.3, -1.75, 0.9, 1.2, -0.01])
    r, status = sr.specrad(np.diag(d))
    assert status == 0 and abs(r - 1.75) <= 1e-12 * 1.75


@pytest.mark.parametrize("c", [-3.5, 0.25, 1e-3])
def test_scaling_the_matrix_scales_the_radius(c):
    w = sr.reference_matrix(33, 0.1, 7)
    r, _ = sr.specrad(w)
    rc, status = sr.specrad(c * w)
    assert status == 0 and abs(rc - abs(c) * r) <= 1e-12 * abs(c) * r
