"""The leave-one-out reference of the ridge_grid tests (tests/loo_ref.py) against its own definition: the closed forms
of DESIGN 3.3c agree with a brute-force refit that really deletes each row, and the wide and tall forms are the same
number on a square system.  No GPU: this pins what test_gpu_ridge_loo.py measures the kernel against."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loo_ref  # noqa: E402


def _case(rows, cols, n_out, seed):
    E, D, t_scale = loo_ref.make_case(rows, cols, n_out, 1, seed)
    E, Ds = E[0], D[0] * t_scale[0]
    lams = loo_ref.gram_mean_diag(E) * np.array([1e-4, 1e-2, 1.0])
    return E, Ds, lams


@pytest.mark.parametrize("rows,cols,n_out", [(24, 40, 2), (60, 17, 1), (100, 140, 4)])
def test_closed_form_is_the_brute_force_refit(rows, cols, n_out):
    E, Ds, lams = _case(rows, cols, n_out, 100 * rows + cols)
    for lam in lams:
        want = loo_ref.brute_force(E, Ds, lam)
        for form in ("wide", "tall"):
            got = loo_ref.closed_form(E, Ds, lam, form)
            rel = abs(got - want) / want
            print(f"({rows}, {cols}, {n_out}) lambda={lam:.3e} {form}: closed {got:.12e} brute {want:.12e} rel {rel:.2e}")
            assert rel <= 1e-9, (lam, form, rel)


def test_wide_and_tall_forms_agree_on_a_square_system():
    E, Ds, lams = _case(128, 128, 8, 7)
    for lam in lams:
        w, t = loo_ref.loo_wide(E, Ds, lam), loo_ref.loo_tall(E, Ds, lam)
        rel = float(np.max(np.abs(w - t)) / np.max(np.abs(w)))
        sw, st = loo_ref.closed_form(E, Ds, lam, "wide"), loo_ref.closed_form(E, Ds, lam, "tall")
        print(f"lambda={lam:.3e}: residuals rel {rel:.2e}, scores {sw:.12e} {st:.12e}")
        assert rel <= 1e-9
        assert abs(sw - st) <= 1e-9 * sw


def test_choose_takes_the_lowest_index_and_skips_bad_candidates():
    E, Ds, lams = _case(24, 40, 2, 3)
    grid = np.array([np.nan, lams[1], -1.0, lams[1], np.inf, lams[2]])
    idx, s = loo_ref.choose(E, Ds, grid)
    assert np.isinf(s[[0, 2, 4]]).all() and np.isfinite(s[[1, 3, 5]]).all()
    assert s[1] == s[3]
    assert idx == (1 if s[1] <= s[5] else 5)
    assert loo_ref.choose(E, Ds, np.array([np.nan, -2.0]))[0] == -1
