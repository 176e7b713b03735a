"""Running normal equations without a device: the NumPy restatement (tests/gram_ref.py) against the
stacked ridge solves the other references use, the forgetting recursion against the explicitly weighted stacked fit, and
the C ABI of esn_gram_accumulate[_f32] / esn_gram_solve / esn_gram_solve_workspace_bytes: declared, bound, built, and
every refused call answered -1 / -2 with the function's name before anything touches a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import c_abi
import gram_ref
import multipilot_ref
import tracking_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAM_NAMES = {"esn_gram_accumulate": 13, "esn_gram_accumulate_f32": 13, "esn_gram_solve_workspace_bytes": 3,
              "esn_gram_solve": 12}


def segments(rs, n, rows, cols, n_out):
    return [(rs.randn(rows, cols), rs.randn(rows, n_out)) for _ in range(n)]


@pytest.mark.parametrize("rows,cols", [(12, 40), (60, 24)])         # rows < cols and rows > cols
@pytest.mark.parametrize("lam", [1e-3, 1.0])
def test_primal_equals_dual_ridge(rows, cols, lam):
    rs = np.random.RandomState(rows + cols)
    segs = segments(rs, 3, rows // 3, cols, 4)
    state = None
    for E, Ds in segs:
        state = gram_ref.accumulate(E, Ds, state, 1.0)
    W = gram_ref.solve(*state, lam)
    E_all, D_all = gram_ref.weighted_stack(segs, 1.0)
    bound = gram_ref.primal_bound(E_all, lam)
    for ref in (tracking_ref.stacked_solve(segs, lam)[0], multipilot_ref.ridge(E_all, D_all, lam),
                gram_ref.stacked_ridge(E_all, D_all, lam)):
        err = np.abs(W - ref).max() / np.abs(ref).max()
        print(f"{rows}x{cols} lambda {lam}: {err:.3e} against the bound {bound:.3e}")
        assert err <= bound


@pytest.mark.parametrize("gamma", [0.0, 0.5, 0.8, 1.0])
def test_forgetting_recursion_is_the_weighted_stack(gamma):
    rs = np.random.RandomState(7)
    segs = segments(rs, 4, 9, 30, 2)
    state = None
    for E, Ds in segs:
        state = gram_ref.accumulate(E, Ds, state, gamma)
    E_w, D_w = gram_ref.weighted_stack(segs, gamma)
    assert np.allclose(state[0], E_w.T @ E_w, rtol=0, atol=1e-12 * np.abs(state[0]).max())
    assert np.allclose(state[1], D_w.T @ E_w, rtol=0, atol=1e-12 * np.abs(state[0]).max())
    lam = 1e-2
    W, ref = gram_ref.solve(*state, lam), multipilot_ref.ridge(E_w, D_w, lam)
    assert np.abs(W - ref).max() / np.abs(ref).max() <= gram_ref.primal_bound(E_w, lam)
    if gamma == 0.0:                    # only the newest segment is left
        assert E_w.shape[0] == 9 and np.array_equal(E_w, segs[-1][0])


def test_cond_aug_is_the_condition_of_the_augmented_matrix():
    rs = np.random.RandomState(3)
    for rows, cols in ((5, 9), (9, 5)):
        E = rs.randn(rows, cols)
        A = np.vstack([E, np.sqrt(0.3) * np.eye(cols)])
        assert abs(gram_ref.cond_aug(E, 0.3) / np.linalg.cond(A) - 1.0) < 1e-10


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_declared_bound_and_built():
    from esn_ofdm_mimo_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "esn_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n_args in GRAM_NAMES.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", hdr)
        assert m, f"{name} is not declared in esn_hip.h"
        assert len(m.group(1).split(",")) == n_args, name
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
    assert "esn_gram.hip" in build.SOURCES
    assert _lib.ABI_VERSION == 10


@pytest.fixture(scope="module")
def lib():
    from esn_ofdm_mimo_amd import _lib, build
    build.build_library(verbose=False)
    return _lib.load()


def refused(lib, rc, want, name, word=None):
    msg = lib.esn_last_error().decode()
    assert rc == want, (rc, msg)
    assert name in msg and (word is None or word in msg), msg


P = 64                                                  # a pointer that is never dereferenced: the checks run first


def acc_args(**kw):
    a = dict(E=P, D=P, n_groups=3, T=45, transient=5, cols=72, n_out=4, t_scale=None, t_shift=None, decay=1.0, Gm=P,
             Cm=P, stream=None)
    a.update(kw)
    return list(a.values())


def solve_args(lib, **kw):
    a = dict(Gm=P, Cm=P, n_groups=3, cols=72, n_out=4, ridge=P, n_ridge=2, W_out=P, status=P, workspace=P,
             workspace_bytes=lib.esn_gram_solve_workspace_bytes(3, 2, 72), stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("name", ["esn_gram_accumulate", "esn_gram_accumulate_f32"])
def test_accumulate_refuses_before_any_device_call(lib, name):
    fn = getattr(lib, name)
    for arg in ("E", "D", "Gm", "Cm"):
        refused(lib, fn(*acc_args(**{arg: None})), -1, name, "null")
    for bad in (dict(n_groups=0), dict(transient=45), dict(transient=-1), dict(cols=0), dict(n_out=0), dict(n_out=17),
                dict(decay=-0.1), dict(decay=1.5), dict(decay=float("nan")), dict(E=P + 8)):
        refused(lib, fn(*acc_args(**bad)), -1, name)
    refused(lib, fn(*acc_args(decay=2.0)), -1, name, "decay")
    refused(lib, fn(*acc_args(cols=545)), -2, name, "544")


def test_solve_refuses_before_any_device_call(lib):
    name, fn = "esn_gram_solve", lib.esn_gram_solve
    for arg in ("Gm", "Cm", "ridge", "W_out", "status", "workspace"):
        refused(lib, fn(*solve_args(lib, **{arg: None})), -1, name, "null")
    for bad in (dict(n_groups=0), dict(cols=0), dict(n_out=0), dict(n_out=17)):
        refused(lib, fn(*solve_args(lib, **bad)), -1, name)
    for n_ridge in (0, 17):
        refused(lib, fn(*solve_args(lib, n_ridge=n_ridge)), -1, name, "n_ridge")
    refused(lib, fn(*solve_args(lib, cols=545)), -2, name, "544")
    need = lib.esn_gram_solve_workspace_bytes(3, 2, 72)
    refused(lib, fn(*solve_args(lib, workspace_bytes=need - 1)), -1, name, "esn_gram_solve_workspace_bytes")
    refused(lib, fn(*solve_args(lib, workspace=P + 8)), -1, name, "aligned")


def test_workspace_query(lib):
    q = lib.esn_gram_solve_workspace_bytes
    assert q(3, 1, 72) == 3 * 8 * 80 * 80                               # one padded factor per group ...
    assert q(3, 16, 72) == q(3, 1, 72)                                  # ... whatever the number of candidates
    assert q(2048, 16, 528) == 2048 * 8 * 528 * 528
    assert q(1, 1, 544) == 8 * 544 * 544
    assert q(0, 1, 72) == 0 and q(3, 0, 72) == 0 and q(3, 1, 0) == 0 and q(3, 1, 545) == 0


C_SRC = r'''
#include <stdio.h>
#include <string.h>
#include "esn_hip.h"
int main(void) {
    /* never dereferenced: the checks run first */
    const double* dp = (const double*)64;
    const float* fp = (const float*)64;
    double* w = (double*)64;
    int* st = (int*)64;
    void* ws = (void*)64;
    if (esn_abi_version() != 10) return 1;
    if (esn_gram_accumulate(0, dp, 3, 45, 5, 72, 4, 0, 0, 1.0, w, w, 0) != -1) return 2;
    if (!strstr(esn_last_error(), "esn_gram_accumulate") || !strstr(esn_last_error(), "null")) return 3;
    if (esn_gram_accumulate(dp, dp, 3, 45, 45, 72, 4, 0, 0, 1.0, w, w, 0) != -1) return 4;
    if (esn_gram_accumulate_f32(fp, dp, 3, 45, 5, 72, 4, 0, 0, 1.5, w, w, 0) != -1) return 5;
    if (!strstr(esn_last_error(), "esn_gram_accumulate_f32") || !strstr(esn_last_error(), "decay")) return 6;
    if (esn_gram_accumulate_f32(fp, dp, 3, 45, 5, 545, 4, 0, 0, 0.5, w, w, 0) != -2) return 7;
    if (esn_gram_solve(dp, dp, 3, 72, 4, dp, 17, w, st, ws, (size_t)1 << 40, 0) != -1) return 8;
    if (!strstr(esn_last_error(), "esn_gram_solve") || !strstr(esn_last_error(), "n_ridge")) return 9;
    if (esn_gram_solve(dp, dp, 3, 72, 4, dp, 2, w, st, ws, esn_gram_solve_workspace_bytes(3, 2, 72) - 1, 0) != -1)
        return 10;
    if (!strstr(esn_last_error(), "workspace")) return 11;
    if (esn_gram_solve(dp, dp, 3, 545, 4, dp, 2, w, st, ws, (size_t)1 << 40, 0) != -2) return 12;
    if (esn_gram_solve_workspace_bytes(3, 16, 528) != esn_gram_solve_workspace_bytes(3, 1, 528)) return 13;
    printf("gram abi ok\n");
    return 0;
}
'''


def test_gram_entry_points_link_from_c99_and_validate_without_a_device(tmp_path):
    r = c_abi.compile_and_run(tmp_path, "gram", C_SRC)
    assert "gram abi ok" in r.stdout
