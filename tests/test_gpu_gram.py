"""esn_gram_accumulate[_f32] and esn_gram_solve on the device against NumPy (tests/gram_ref.py), at the
shapes where the kernels take another path: the scalar loads (cols % 4 != 0), a column one past a tile, rows that are no
multiple of the chunk, wide and tall, and 33 tiles (cols 528, past the 512 of the Cholesky kernels) with float64 and
float32 E.  Five groups each; two shapes cut a transient.  Every device result is computed once per shape."""
import numpy as np
import pytest

import gram_ref

pytestmark = pytest.mark.gpu

G = 5
TOL_CHOL = 1e-7                 # the rule of tests/test_gpu_ridge.py for the Cholesky path
# name: rows, cols, n_out, transient, float32 E
SHAPES = {
    "scalar_1x5": (1, 5, 1, 0, False),
    "tall_33x5": (33, 5, 2, 3, False),
    "tile_plus_one_16x17": (16, 17, 4, 0, False),
    "tall_40x20": (40, 20, 4, 0, False),
    "wide_40x132": (40, 132, 8, 5, False),
    "wide_128x132": (128, 132, 8, 0, False),
    "wide_128x528": (128, 528, 8, 0, False),
    "wide_f32_128x528": (128, 528, 8, 0, True),
}
_CASES = {}


def case(name):
    """bank, E (device), D, the rows E64 [G, rows, cols] and scaled teacher Ds [G, rows, n_out], the fresh state."""
    if name not in _CASES:
        import torch
        from esn_ofdm_mimo_amd import batched
        rows, cols, n_out, tr, f32 = SHAPES[name]
        rs = np.random.RandomState(1000 + rows + cols)
        bank = batched.ReservoirBank(1, n_out, 2, np.zeros((2, 2)), np.zeros((2, 1)), np.zeros((2, n_out)))
        E = rs.randn(G, rows + tr, cols)
        D = rs.randn(G, rows + tr, n_out)
        t_scale, t_shift = rs.rand(G, n_out) + 0.5, 0.1 * rs.randn(G, n_out)
        bank.set_scaling(None, None, t_scale, t_shift)
        if f32:
            E = E.astype(np.float32)
        E_dev = torch.as_tensor(E, device="cuda")
        Ds = D[:, tr:] * t_scale[:, None, :] + t_shift[:, None, :]
        state = bank.gram_accumulate(E_dev, D, tr)
        _CASES[name] = dict(bank=bank, E=E_dev, D=D, E64=E.astype(np.float64)[:, tr:], Ds=Ds, state=state, tr=tr)
    return _CASES[name]


def acc_bound(c, rows, prior=0.0):
    return gram_ref.accumulate_bound(rows, np.abs(c["E64"]).max(), np.abs(c["Ds"]).max(), prior)


def worst(got, want, bound):
    return float(np.max(np.abs(got - want))) / bound


# ---- accumulate -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_accumulate_vs_numpy(name):
    rows, cols, n_out = SHAPES[name][:3]
    c = case(name)
    Gd, Cd = c["state"].G.cpu().numpy(), c["state"].C.cpu().numpy()
    assert Gd.shape == (G, cols, cols) and Cd.shape == (G, n_out, cols)
    ratio = 0.0
    for g in range(G):
        Gr, Cr = gram_ref.accumulate(c["E64"][g], c["Ds"][g])
        ratio = max(ratio, worst(Gd[g], Gr, acc_bound(c, rows)), worst(Cd[g], Cr, acc_bound(c, rows)))
    print(f"{name}: worst |device - numpy| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    assert np.array_equal(Gd, Gd.transpose(0, 2, 1)), "G is not bitwise symmetric"
    # (t_scale in 0.5 .. 1.5 and t_shift about 0.1 are part of Ds: C meets the bound only with both applied)


@pytest.mark.parametrize("name", ["scalar_1x5", "tile_plus_one_16x17", "wide_40x132", "wide_f32_128x528"])
def test_decay_zero_does_not_read_the_state(name):
    import torch
    from esn_ofdm_mimo_amd.batched import GramState
    c = case(name)
    st = c["state"]
    nan = GramState(torch.full_like(st.G, float("nan")), torch.full_like(st.C, float("nan")), st.t_scale, st.t_shift)
    c["bank"].gram_accumulate(c["E"], c["D"], c["tr"], nan, 0.0)
    assert torch.equal(nan.G, st.G) and torch.equal(nan.C, st.C)


@pytest.mark.parametrize("name", ["tall_33x5", "tile_plus_one_16x17", "wide_40x132", "wide_128x528"])
def test_decay_and_split_rows(name):
    """decay 0.5 on a prior state, and two calls on halves of the rows against one call on all of them."""
    import torch
    from esn_ofdm_mimo_amd.batched import GramState
    rows, cols, n_out, tr, _ = SHAPES[name]
    c = case(name)
    bank, st = c["bank"], c["state"]
    prior = GramState(st.G.clone(), st.C.clone(), st.t_scale, st.t_shift)
    bank.gram_accumulate(c["E"], c["D"], tr, prior, 0.5)
    Gd, Cd = prior.G.cpu().numpy(), prior.C.cpu().numpy()
    G0, C0 = st.G.cpu().numpy(), st.C.cpu().numpy()
    ratio = 0.0
    for g in range(G):
        Gr, Cr = gram_ref.accumulate(c["E64"][g], c["Ds"][g], (G0[g], C0[g]), 0.5)
        b = acc_bound(c, rows, prior=max(np.abs(G0[g]).max(), np.abs(C0[g]).max()))
        ratio = max(ratio, worst(Gd[g], Gr, b), worst(Cd[g], Cr, b))
    print(f"{name}: decay 0.5, worst / bound = {ratio:.3f}")
    assert ratio <= 1.0
    assert np.array_equal(Gd, Gd.transpose(0, 2, 1))
    if rows < 2:
        return
    h = tr + rows // 2                          # rows [tr, h) start the sum, rows [h, T) are added with decay 1
    two = bank.gram_accumulate(c["E"][:, :h].contiguous(), c["D"][:, :h], tr)
    bank.gram_accumulate(c["E"][:, h:].contiguous(), c["D"][:, h:], 0, two, 1.0)
    b = acc_bound(c, rows)                      # the same bound: the second call's one extra rounding is inside factor 4
    r2 = max(worst(two.G.cpu().numpy(), G0, b), worst(two.C.cpu().numpy(), C0, b))
    print(f"{name}: two halves against one call, worst / bound = {r2:.3f}")
    assert r2 <= 1.0


@pytest.mark.parametrize("name", ["tall_33x5", "wide_40x132", "wide_f32_128x528"])
def test_a_group_alone_is_bitwise_itself(name):
    import torch
    from esn_ofdm_mimo_amd import batched
    c = case(name)
    n_out, tr = SHAPES[name][2], c["tr"]
    g = 3
    alone = batched.ReservoirBank(1, n_out, 2, np.zeros((2, 2)), np.zeros((2, 1)), np.zeros((2, n_out)))
    alone.set_scaling(None, None, c["bank"].t_scale[g:g + 1], c["bank"].t_shift[g:g + 1])
    st = alone.gram_accumulate(c["E"][g:g + 1].contiguous(), c["D"][g:g + 1], tr)
    assert torch.equal(st.G[0], c["state"].G[g]) and torch.equal(st.C[0], c["state"].C[g])
    lam = np.array([[1e-2, 3.0]])
    W1, s1 = alone.gram_solve(st, lam)
    WG, sG = c["bank"].gram_solve(c["state"], np.repeat(lam, G, axis=0))
    assert torch.equal(W1[0], WG[g]) and torch.equal(s1[0], sG[g])


# ---- solve ------------------------------------------------------------------------------------------------------------
def lambdas(n_l):
    """[G, L]: a different lambda per group, the candidates a decade apart at most"""
    base = np.array([3e-3, 1e-2, 5e-2, 0.3, 2.0])[:, None]
    return base * (10.0 ** np.linspace(0.0, 2.0, n_l))[None, :] if n_l > 1 else base


@pytest.mark.parametrize("name", list(SHAPES))
def test_solve_vs_numpy_and_cholesky_path(name):
    import torch
    rows, cols, n_out, tr, f32 = SHAPES[name]
    c = case(name)
    bank, st = c["bank"], c["state"]
    G0, C0 = st.G.clone(), st.C.clone()
    Gh, Ch = st.G.cpu().numpy(), st.C.cpu().numpy()
    # G is symmetric bit for bit, so cond(G + lambda I) = (e_max + lambda) / (e_min + lambda) from one eigvalsh per
    # group serves every candidate (e_min of the rank-deficient shapes is round-off beside the smallest lambda, 3e-3)
    ev = [np.linalg.eigvalsh(Gh[g]) for g in range(G)]

    def cond_of(g, lam_gl):
        return (ev[g][-1] + lam_gl) / (ev[g][0] + lam_gl)

    ratio = 0.0
    for n_l in (1, 3, 16):
        lam = lambdas(n_l)
        W, status = bank.gram_solve(st, lam)
        assert W.shape == (G, n_l, n_out, cols) and status.shape == (G, n_l)
        assert int(status.ne(0).sum().item()) == 0, status
        W = W.cpu().numpy()
        for g in range(G):
            for l in range(n_l):
                ref = np.linalg.solve(Gh[g] + lam[g, l] * np.eye(cols), Ch[g].T).T
                bound = 10.0 * cond_of(g, lam[g, l]) * gram_ref.EPS * np.abs(ref).max()
                ratio = max(ratio, worst(W[g, l], ref, bound))
    print(f"{name}: solve against np.linalg.solve, worst / (10 cond eps max|W|) = {ratio:.4f}")
    assert ratio <= 1.0
    assert torch.equal(st.G, G0) and torch.equal(st.C, C0), "the solve wrote into the state"
    # the shipped path on the same rows: the Cholesky solve of the stacked system, at every shape
    lam1 = lambdas(1)[:, 0]
    W_g, _ = bank.gram_solve(st, lam1)
    W_c, st_c = bank.solve(c["E"], c["D"], tr, method="chol", ridge=lam1)
    assert int(st_c.ne(0).sum().item()) == 0
    W_g, W_c = W_g.cpu().numpy(), W_c.cpu().numpy()
    r2 = 0.0
    for g in range(G):
        bound = 2.0 * max(TOL_CHOL, 10.0 * cond_of(g, lam1[g]) * gram_ref.EPS) * np.abs(W_c[g]).max()
        r2 = max(r2, worst(W_g[g], W_c[g], bound))
    print(f"{name}: gram solve against method='chol', worst / summed bounds = {r2:.4f}")
    assert r2 <= 1.0


@pytest.mark.parametrize("name", ["tile_plus_one_16x17", "wide_40x132"])
def test_rank_deficient_candidate_is_flagged_alone(name):
    rows, cols, n_out = SHAPES[name][:3]
    c = case(name)
    lam = np.tile(np.array([1e-2, 0.0, 1.0]), (G, 1))
    W, status = c["bank"].gram_solve(c["state"], lam)
    assert status.cpu().numpy().tolist() == [[0, 1, 0]] * G
    W = W.cpu().numpy()
    assert not W[:, 1].any()
    Gh, Ch = c["state"].G.cpu().numpy(), c["state"].C.cpu().numpy()
    for g in range(G):
        for l in (0, 2):
            A = Gh[g] + lam[g, l] * np.eye(cols)
            ref = np.linalg.solve(A, Ch[g].T).T
            assert worst(W[g, l], ref, 10.0 * np.linalg.cond(A) * gram_ref.EPS * np.abs(ref).max()) <= 1.0


def test_invalid_lambda_and_limits():
    from esn_ofdm_mimo_amd import _lib
    c = case("tall_40x20")
    lam = np.tile(np.array([0.5, -1.0, np.nan]), (G, 1))
    W, status = c["bank"].gram_solve(c["state"], lam)
    assert status.cpu().numpy().tolist() == [[0, 2, 2]] * G
    assert not W[:, 1:].cpu().numpy().any()
    with pytest.raises(ValueError, match="1 to 16"):
        c["bank"].gram_solve(c["state"], np.ones((G, 17)))
    with pytest.raises(ValueError, match="decay"):
        c["bank"].gram_accumulate(c["E"], c["D"], 0, c["state"], 1.5)
    import torch
    with pytest.raises(_lib.EsnHipError, match="limit is 544"):
        c["bank"].gram_accumulate(torch.zeros((1, 2, 545), dtype=torch.float64, device="cuda"), np.zeros((1, 2, 4)), 0)
