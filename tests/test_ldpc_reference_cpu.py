"""(no GPU) Is the oracle of the coded leg itself right?  oracle/ldpc_oracle.py restates pyldpc, which is absent, and its
sum-product has only ever been held against itself.  Here:

  * tests/ldpc_ref.py's bp_trace (the same message passing, no early stop) gives decode_bp's answer when read at the
    iteration decode_bp stops at, so the margins the GPU tests take from the trace are margins of decode_bp's own run;
  * on a cycle-free graph sum-product is exact: the trace's posteriors equal the bitwise MAP log-ratios obtained by
    enumerating the code (1e-10), and decode_bp decides as MAP does -- once a gadget keeps it from stopping early;
  * qam_llrs_maxlog equals a brute force over the 2-D constellation in long double for every constellation size the API
    accepts, and its signs are the uncoded detector's hard decisions."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ldpc_ref  # noqa: E402
from oracle import esn_oracle as eo  # noqa: E402
from oracle import ldpc_oracle as lo  # noqa: E402

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def code512():
    H_sys, P, k, _ = lo.systematic_code(lo.gallager_parity_check(512, 4, 8, np.random.RandomState(5)))
    return H_sys, P, k


def test_graph_arrays_list_every_edge_once_from_both_sides(code512):
    for H in (code512[0], ldpc_ref.tree_code()[0]):
        chk_ptr, edge_var, var_ptr, var_edge = ldpc_ref.graph_arrays(H)
        assert all(a.dtype == np.int32 for a in (chk_ptr, edge_var, var_ptr, var_edge))
        m, n = H.shape
        assert chk_ptr[0] == var_ptr[0] == 0 and chk_ptr[-1] == var_ptr[-1] == len(edge_var) == len(var_edge) == H.sum()
        back = np.zeros_like(H)
        for c in range(m):
            back[c, edge_var[chk_ptr[c]:chk_ptr[c + 1]]] += 1
        assert np.array_equal(back, H)
        assert sorted(var_edge.tolist()) == list(range(len(edge_var)))
        for v in range(n):
            assert np.all(edge_var[var_edge[var_ptr[v]:var_ptr[v + 1]]] == v)


@pytest.mark.parametrize("sigma,maxiter", [(0.7, 10), (0.9, 6), (1.1, 6)])
def test_trace_read_at_the_stopping_iteration_is_decode_bp(code512, sigma, maxiter):
    H, P, k = code512
    rs = np.random.RandomState(int(10 * sigma))
    u = (rs.rand(12, k) > 0.5).astype(np.uint8)
    c = lo.encode(P, u)
    llr = 2.0 * ((1.0 - 2.0 * c) + sigma * rs.randn(*c.shape)) / sigma ** 2
    y = 0.5 * np.clip(llr, -20, 20)
    L_post, margin = ldpc_ref.bp_trace(H, y, 1.0, maxiter)
    assert L_post.shape == (maxiter, 12, 512) and margin.shape == (maxiter, 12)
    x, stop = ldpc_ref.trace_decision(H, L_post)
    print(f"sigma {sigma}: stopping iteration per word {(stop + 1).tolist()}, min(1 - |X|) {margin.min():.2e}")
    np.testing.assert_array_equal(x, lo.decode_bp(H, y, 1.0, maxiter))
    if sigma == 0.7:                                    # both regimes: words that stop early and at the last sweep
        assert (stop < maxiter - 1).sum() >= 6
    else:
        assert (stop == maxiter - 1).any()
    # a shorter run is a prefix of the longer one
    np.testing.assert_array_equal(ldpc_ref.bp_trace(H, y, 1.0, 2)[0], L_post[:2])


def test_sum_product_is_exact_map_on_a_tree():
    H, y = ldpc_ref.tree_code(seed=0)
    assert H.sum(1).tolist() == [3, 4, 2, 4, 1]
    Lc = 2.0 * y / 10.0 ** (-1.0 / 10.0)
    L_map = ldpc_ref.exact_bit_llrs(H, Lc)
    assert np.all(np.isposinf(L_map[:, 10]))           # the gadget's check admits c_10 = 0 only
    L_map = L_map[:, :10]
    assert np.abs(L_map).min() >= 1e-6, np.abs(L_map).min()
    L_post, _ = ldpc_ref.bp_trace(H, y, 1.0, 8)
    for it in range(8):
        dev = np.abs(L_post[it][:, :10] - L_map).max()
        print(f"iteration {it + 1}: max |L_post - L_map| = {dev:.2e}")
        if it + 1 >= 3:                                 # the tree's longest path is covered after three sweeps
            assert dev <= 1e-10
    assert np.abs(L_post[0][:, :10] - L_map).max() > 1e-3      # one sweep has not yet seen the whole tree
    for it in (3, 4, 8):
        out = lo.decode_bp(H, y, 1.0, it)
        np.testing.assert_array_equal(out[:, :10], (L_map <= 0).astype(np.uint8))
        assert np.all(out[:, 10] == 1)
    # the gadget's role: without it decode_bp stops at the first codeword it meets, which is not the MAP decision
    H0, y0 = ldpc_ref.tree_code(seed=0, gadget=False)
    np.testing.assert_array_equal(y0[:, :10], y[:, :10])
    early = lo.decode_bp(H0, y0, 1.0, 8)
    differ = (early[:, :10] != (L_map <= 0)).any(axis=1)
    assert (early[:, :10] != (L_map <= 0)).sum() == 10
    assert not ((early[differ].astype(int) @ H0.T.astype(int)) % 2).any()      # each of them a codeword met early


def test_exact_bit_llrs_on_a_single_parity_check():
    """Three bits under one check: L_0 = Lc_0 + 2 atanh(tanh(Lc_1 / 2) tanh(Lc_2 / 2)), the textbook box-plus."""
    rs = np.random.RandomState(1)
    Lc = rs.randn(50, 3) * 2
    got = ldpc_ref.exact_bit_llrs(np.ones((1, 3), dtype=np.uint8), Lc)
    for v in range(3):
        a, b = [w for w in range(3) if w != v]
        want = Lc[:, v] + 2 * np.arctanh(np.tanh(Lc[:, a] / 2) * np.tanh(Lc[:, b] / 2))
        assert np.abs(got[:, v] - want).max() <= 1e-12


@pytest.mark.parametrize("m", [2, 4, 6, 8, 10])
def test_llr_oracle_is_the_brute_force_and_signs_are_hard_bits(m):
    rs = np.random.RandomState(m)
    const = eo.unit_qam(m)
    S, sigma2 = 400, 0.05
    z = const[rs.randint(0, 2 ** m, size=S)] + 0.2 * (rs.randn(S) + 1j * rs.randn(S))
    z[:4] = [3 + 3j, -3 + 0.1j, 0.1 - 3j, const[0]]
    got = lo.qam_llrs_maxlog(z, m, sigma2)
    want, dsum = ldpc_ref.llr_longdouble(z, m, sigma2)
    assert want.dtype == np.longdouble and want.shape == dsum.shape == (S, m)
    # the oracle squares a float64 modulus: a few roundings of each distance, then the subtraction
    excess = (np.abs(got - want) - 16 * EPS * dsum / sigma2).max()
    print(f"m={m}: max |oracle - brute force| = {float(np.abs(got - want).max()):.2e}")
    assert excess <= 0
    nz = want != 0
    assert nz.all()
    hard = eo.hard_bits(z.reshape(-1, 1), const, m).reshape(S, m)         # [N m, 1] -> [N, m]
    assert np.array_equal((got < 0)[nz], hard[nz] == 1)
    assert 0.3 < hard.mean() < 0.7
    # the floor of sigma^2
    np.testing.assert_array_equal(ldpc_ref.llr_longdouble(z, m, 0.0)[0], ldpc_ref.llr_longdouble(z, m, 1e-12)[0])
