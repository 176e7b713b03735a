"""Ridge-regression read-out (an extension; the reference fits with pinv only) through every layer:
the three solve kernels (LDS Cholesky, workspace Cholesky, QR) at lambda > 0, the lambda = 0 contract (bitwise today's
pinv solve), several lambda per pilot in one launch, the padding rows of a ragged last tile, rank deficiency, bad
lambda, the QR repair, ReservoirBank.fit / the drop-in ESN, and the BER gain at the headline shape.

Reference: ridge from a float64 SVD, W^T = V diag(s / (s^2 + lambda)) U^T D_s.  A singular value at round-off level
(s <= eps * max(rows, cols) * s_max, NumPy's matrix_rank cut) is the float image of an exact 0 of a rank-deficient E,
for which the factor is 0 at every lambda >= 0 -- without the cut the factor of that direction would be ~ 1 / s at a
lambda far below s^2 and the reference itself would be round-off noise.  The cut touches the rank-deficient cases only
(the regular inputs have s_min ~ 1e-3 s_max).

Tolerances are those of test_readout_solve_vs_pinv: 1e-7 ("chol") and 1e-9 ("qr") relative to max|W|."""
import numpy as np
import pytest

from oracle import esn_oracle as eo

pytestmark = pytest.mark.gpu

LAMBDAS = (1e-6, 1e-3, 1.0, 100.0)
TOL = {"chol": 1e-7, "qr": 1e-9}
G, TR = 3, 5

# name: rows, cols, method, n_out, float32 E, chol_dma knob
SHAPES = {
    # LDS Cholesky (Gram <= 128): ragged last tile, tall, float32 E with the LDS-DMA rings on and off
    "lds_wide_40x72": (40, 72, "chol", 4, False, None),
    "lds_tall_300x90": (300, 90, "chol", 4, False, None),
    "lds_wide_f32_dma1_128x528": (128, 528, "chol", 4, True, "1"),
    "lds_wide_f32_dma0_128x528": (128, 528, "chol", 4, True, "0"),
    # workspace Cholesky (Gram 129..512)
    "ws_wide_130x131": (130, 131, "chol", 4, False, None),
    "ws_tall_333x150": (333, 150, "chol", 4, False, None),
    "ws_wide_f32_130x150": (130, 150, "chol", 4, True, None),
    # QR: wide, tall, and n_out = 9, which the Cholesky path refuses
    "qr_wide_20x36": (20, 36, "qr", 4, False, None),
    "qr_tall_50x12": (50, 12, "qr", 4, False, None),
    "qr_wide_nout9_40x72": (40, 72, "qr", 9, False, None),
}


def rel_err(got, want):
    return float(np.max(np.abs(got - want)) / (np.max(np.abs(want)) + 1e-300))


def ridge_ref(E, Ds, lam):
    """[n_out, cols]: V diag(s / (s^2 + lambda)) U^T D_s in float64 (module docstring: the rank cut)."""
    U, s, Vt = np.linalg.svd(E, full_matrices=False)
    live = s > np.finfo(np.float64).eps * max(E.shape) * s[0]
    f = np.where(live, s / np.where(live, s * s + lam, 1.0), 0.0)
    return ((Vt.T * f) @ (U.T @ Ds)).T


@pytest.fixture(scope="module")
def batched():
    from esn_ofdm_mimo_amd import _lib, batched
    yield batched
    _lib.debug_set("chol_dma", "1")


def _bank(batched, cols, n_out):
    return batched.ReservoirBank(cols - 2, n_out, 2, np.zeros((2, 2)), np.zeros((2, cols - 2)), np.zeros((2, n_out)))


_CASES = {}


def case(batched, name):
    """Inputs of test_readout_solve_vs_pinv for one shape, drawn once: bank, E (device), D, float64 E, scaled teacher."""
    if name not in _CASES:
        import torch
        rows, cols, method, n_out, f32, _ = SHAPES[name]
        rs = np.random.RandomState(rows + cols)
        bank = _bank(batched, cols, n_out)
        E = rs.randn(G, rows + TR, cols)
        E[:, :, :3] *= 1e-3                      # uneven column scales
        D = rs.randn(G, rows + TR, n_out)
        t_scale = rs.rand(G, n_out) + 0.5
        bank.set_scaling(None, None, t_scale, None)
        if f32:
            E = E.astype(np.float32)
        E_dev = torch.as_tensor(E, device="cuda")
        E64 = E.astype(np.float64)
        Ds = D[:, TR:] * t_scale[:, None, :]
        _CASES[name] = (bank, E_dev, D, E64[:, TR:], Ds, {})
    return _CASES[name]


def want(batched, name, g, lam):
    _, _, _, E64, Ds, cache = case(batched, name)
    if (g, lam) not in cache:
        cache[(g, lam)] = ridge_ref(E64[g], Ds[g], lam)
    return cache[(g, lam)]


def solve(batched, name, ridge, **kw):
    from esn_ofdm_mimo_amd import _lib
    bank, E_dev, D, _, _, _ = case(batched, name)
    method, dma = SHAPES[name][2], SHAPES[name][5]
    _lib.debug_set("chol_dma", dma or "1")
    try:
        W, st = bank.solve(E_dev, D, TR, method=method, ridge=ridge, **kw)
        W, st = W.clone(), st.clone()
    finally:
        _lib.debug_set("chol_dma", "1")
    return W, st


# ---- 1 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_ridge_vs_svd_reference(batched, name):
    tol = TOL[SHAPES[name][2]]
    for lam in LAMBDAS:
        W, st = solve(batched, name, lam)
        assert W.shape == (G, SHAPES[name][3], SHAPES[name][1]) and st.shape == (G,)
        assert int(st.ne(0).sum().item()) == 0, (lam, st)
        W = W.cpu().numpy()
        for g in range(G):
            err = rel_err(W[g], want(batched, name, g, lam))
            print(f"{name} lambda={lam:g} g={g} rel_err={err:.3e}")
            assert err < tol, (lam, g, err)


# ---- 2 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_lambda_zero_is_todays_solve_bitwise(batched, name):
    import torch
    W0, st0 = solve(batched, name, None)                       # the existing entry point
    Wz, stz = solve(batched, name, np.zeros(G))
    assert torch.equal(stz, st0) and torch.equal(Wz, W0)
    Wz, stz = solve(batched, name, 0.0)
    assert torch.equal(stz, st0) and torch.equal(Wz, W0)
    mixed = np.array([[0.0, 1e-3, 0.0], [2.0, 0.0, 0.0], [0.0, 0.0, 7.0]])
    Wm, stm = solve(batched, name, mixed)
    assert Wm.shape == (G, 3) + tuple(W0.shape[1:]) and stm.shape == (G, 3)
    for g in range(G):
        for l in range(3):
            if mixed[g, l] == 0.0:
                assert int(stm[g, l]) == int(st0[g]) and torch.equal(Wm[g, l], W0[g]), (g, l)
            else:
                assert not torch.equal(Wm[g, l], W0[g]), (g, l)


# ---- 3 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_several_lambdas_in_one_launch(batched, name):
    import torch
    ridge = np.array([[1e-6, 1e-3, 0.0, 1.0, 100.0],
                      [3e-2, 0.0, 5.0, 1e-4, 2e-3],
                      [100.0, 1.0, 1e-3, 1e-6, 0.0]])
    Wm, stm = solve(batched, name, ridge)
    n_out, cols = SHAPES[name][3], SHAPES[name][1]
    assert Wm.shape == (G, 5, n_out, cols) and stm.shape == (G, 5)
    assert int(stm.ne(0).sum().item()) == 0
    tol = TOL[SHAPES[name][2]]
    for l in range(5):
        W1, st1 = solve(batched, name, torch.as_tensor(ridge[:, l].copy()))        # a [G] tensor: one lambda per group
        assert torch.equal(st1, stm[:, l])
        assert torch.equal(W1, Wm[:, l]), l
    for g in range(G):                                                           # ... and each is the ridge solution
        assert rel_err(Wm[g, 0].cpu().numpy(), want(batched, name, g, float(ridge[g, 0]))) < tol


# ---- 4 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lds_wide_40x72", "ws_wide_130x131"])
def test_lambda_stays_off_the_padding_rows(batched, name):
    """Gram dimensions 40 and 130 end in a ragged 16-row tile.  The padding rows carry zeros that the factorisation
    treats as dropped directions; a lambda = 100 added there would turn them into live pivots."""
    W, st = solve(batched, name, 100.0)
    assert int(st.ne(0).sum().item()) == 0
    for g in range(G):
        assert rel_err(W[g].cpu().numpy(), want(batched, name, g, 100.0)) < TOL["chol"]


# ---- 5 ------------------------------------------------------------------------------------------------------------
def _rank_deficient(batched):
    rs = np.random.RandomState(8)
    n_g, rows, cols, n_out = 3, 20, 50, 2
    bank = _bank(batched, cols, n_out)
    E = rs.randn(n_g, rows, cols)
    D = rs.randn(n_g, rows, n_out)
    E[1, 7] = E[1, 3]
    D[1, 7] = D[1, 3]                       # consistent duplicate (test_chol_flags_rank_deficiency_and_qr_repairs)
    return bank, E, D


def test_ridge_lifts_rank_deficiency(batched):
    bank, E, D = _rank_deficient(batched)
    W, st = bank.solve(E, D, 0, method="chol", ridge=0.0)
    assert list(st.cpu().numpy()) == [0, 1, 0]                                   # lambda = 0 flags as today
    lam = 1e-3 * np.array([np.mean(np.sum(E[g] * E[g], axis=1)) for g in range(3)])   # 1e-3 x mean Gram diagonal
    W, st = bank.solve(E, D, 0, method="chol", ridge=lam)
    assert list(st.cpu().numpy()) == [0, 0, 0]
    for g in range(3):
        assert rel_err(W[g].cpu().numpy(), ridge_ref(E[g], D[g], lam[g])) < TOL["chol"]
    # a zero column in a tall system: the Gram matrix E^T E has a zero row and column
    rs = np.random.RandomState(9)
    rows, cols, n_out = 50, 20, 2
    bank = _bank(batched, cols, n_out)
    E = rs.randn(3, rows, cols)
    D = rs.randn(3, rows, n_out)
    E[2, :, 11] = 0.0
    W, st = bank.solve(E, D, 0, method="chol", ridge=0.0)
    assert list(st.cpu().numpy()) == [0, 0, 1]
    lam = 1e-3 * np.array([np.mean(np.sum(E[g] * E[g], axis=0)) for g in range(3)])
    W, st = bank.solve(E, D, 0, method="chol", ridge=lam)
    assert list(st.cpu().numpy()) == [0, 0, 0]
    for g in range(3):
        assert rel_err(W[g].cpu().numpy(), ridge_ref(E[g], D[g], lam[g])) < TOL["chol"]
    assert float(W[2, :, 11].abs().max()) == 0.0


# ---- 6 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lds_wide_40x72", "lds_wide_f32_dma1_128x528", "ws_tall_333x150", "qr_wide_20x36",
                                  "qr_tall_50x12"])
def test_bad_lambda(batched, name):
    import torch
    ridge = np.array([[1e-3, -1.0, 1.0], [np.nan, 1e-3, 1.0], [1e-3, 1.0, np.inf]])
    W, st = solve(batched, name, ridge)
    bad = ~np.isfinite(ridge) | (ridge < 0)
    np.testing.assert_array_equal(st.cpu().numpy(), np.where(bad, 2, 0))
    for g in range(G):
        for l in range(3):
            if bad[g, l]:
                assert float(W[g, l].abs().max()) == 0.0
    good = np.where(bad, 0.5, ridge)                                             # the neighbours are unaffected
    Wg, _ = solve(batched, name, good)
    for g in range(G):
        for l in range(3):
            if not bad[g, l]:
                assert torch.equal(W[g, l], Wg[g, l]), (g, l)


# ---- 7 ------------------------------------------------------------------------------------------------------------
def test_repair_keeps_lambda(batched):
    """lambda = 1e-300 leaves the Gram matrix of the duplicated row singular in float64, so the Cholesky path flags the
    group; resolve_failed hands its lambda to the QR kernel, whose answer is the ridge solution at that lambda."""
    import torch
    bank, E, D = _rank_deficient(batched)
    lam = np.array([1e-3, 1e-300, 1e-3])
    W, st = bank.solve(E, D, 0, method="chol", ridge=lam)
    assert list(st.cpu().numpy()) == [0, 1, 0]
    before = W.clone()
    n = bank.resolve_failed(torch.as_tensor(E, device=W.device), D, 0, W, st, ridge=lam)
    assert n == 1
    assert torch.equal(W[0], before[0]) and torch.equal(W[2], before[2])
    got = E[1] @ W[1].cpu().numpy().T
    assert rel_err(got, E[1] @ ridge_ref(E[1], D[1], 1e-300).T) < 1e-6
    # a repaired group keeps a lambda that matters, too: flag by hand, repair, compare with the QR ridge solve
    lam = np.array([1e-3, 0.5, 1e-3])
    W, st = bank.solve(E, D, 0, method="chol", ridge=lam)
    W[1] = 0.0
    st[1] = 1
    assert bank.resolve_failed(torch.as_tensor(E, device=W.device), D, 0, W, st, ridge=lam) == 1
    assert int(st[1]) == 0
    assert rel_err(W[1].cpu().numpy(), ridge_ref(E[1], D[1], 0.5)) < TOL["qr"]


# ---- 8 ------------------------------------------------------------------------------------------------------------
def test_fit_and_dropin_ridge():
    import torch
    from esn_ofdm_mimo_amd import batched as bt, pyESN
    rs = np.random.RandomState(3)
    t, tr, lam = 200, 10, 1e-3
    u = rs.randn(t, 3)
    d = np.tanh(u @ rs.randn(3, 2)) + 0.3 * np.roll(u[:, :2], 1, axis=0)
    u2 = rs.randn(40, 3)
    esn = pyESN.ESN(3, 2, n_reservoir=80, noise=0, random_state=42, ridge=lam)
    assert esn.ridge == lam
    esn.fit(u, d, tr)
    assert esn.fit_status == 0
    o = eo.OracleESN(3, 2, n_reservoir=80, noise=0, random_state=42)
    o.fit(u, d, tr)
    ext = o._ext_states[tr:]
    o.W_out = ridge_ref(ext, o.scale_teacher(d)[tr:], lam)
    assert rel_err(ext @ esn.W_out.T, ext @ o.W_out.T) < 1e-8
    assert rel_err(esn.predict(u2, 0, continuation=True), o.predict(u2, 0, continuation=True)) < 1e-8
    # ridge = 0.0 is today's drop-in, bit for bit
    a = pyESN.ESN(3, 2, n_reservoir=80, noise=0, random_state=42, ridge=0.0)
    b = pyESN.ESN(3, 2, n_reservoir=80, noise=0, random_state=42)
    pa, pb = a.fit(u, d, tr), b.fit(u, d, tr)
    assert b.ridge == 0.0
    assert np.array_equal(a.W_out, b.W_out) and np.array_equal(pa, pb)
    assert not np.array_equal(a.W_out, esn.W_out)
    with pytest.raises(ValueError):
        pyESN.ESN(3, 2, n_reservoir=8, ridge=-1.0)
    # ReservoirBank.fit(ridge=): scalar and one lambda per group, against the solve of the same harvest
    bank = bt.ReservoirBank(3, 2, 80, b.W, b.W_in, b.W_feedb, noise=0.0)
    U, D = np.stack([u, u[::-1]]), np.stack([d, d[::-1]])
    lam_g = np.array([1e-3, 2e-2])
    E = bank.fit(U, D, transient=tr, precision="f64", noise_mode="none", ridge=lam_g).cpu().numpy()
    assert int(bank.fit_status.ne(0).sum().item()) == 0 and bank.W_out.shape == (2, 2, 83)
    for g in range(2):
        assert rel_err(E[g, tr:] @ bank.W_out[g].cpu().numpy().T, E[g, tr:] @ ridge_ref(E[g, tr:], D[g, tr:], lam_g[g]).T) < 1e-8
    w_g = bank.W_out.clone()
    bank.fit(U, D, transient=tr, precision="f64", noise_mode="none", ridge=1e-3)
    assert torch.equal(bank.W_out[0], w_g[0]) and not torch.equal(bank.W_out[1], w_g[1])
    with pytest.raises(ValueError):
        bank.fit(U, D, transient=tr, precision="f64", noise_mode="none", ridge=np.ones((2, 2)))


# ---- 9 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [dict(), dict(fit_precision="f16", precision="f16")], ids=["default", "f16"])
def test_the_gain_reaches_the_user(prec):
    """4x8 TDL-B, N = 128, 16-QAM, N_res = 512 at 21 dB, 16 blocks x 16 data frames, common frames (same seed): the
    float64 CPU oracle gives BER_ridge / BER_pinv = 0.76 at lambda = 1e-3 (0.88 for its worst block); the cap of 0.95
    is half-way insurance against the shared reservoir and the GPU generator's streams.  "f16" takes the float32-E
    Cholesky path."""
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep, LinkParams
    ridge = DetectorSweep(LinkParams(), n_reservoir=512, seed=0, ridge=1e-3, **prec)
    pinv = DetectorSweep(LinkParams(), n_reservoir=512, seed=0, ridge=None, **prec)
    ber_r, c_r = ridge.run([21.0], 16, frames_per_block=16)
    ber_p, c_p = pinv.run([21.0], 16, frames_per_block=16)
    print(f"BER ridge {ber_r[0]:.5f} pinv {ber_p[0]:.5f} ratio {ber_r[0] / ber_p[0]:.4f}")
    assert c_r[0, 1] == c_p[0, 1] == 16 * 16 * 128 * 4 * 4
    assert ridge.fits_repaired == 0
    assert ber_r[0] <= 0.95 * ber_p[0]
    # chunking leaves the counters alone with ridge on, and a callable lambda(Eb/No) is the same knob
    by_ebno = DetectorSweep(LinkParams(), n_reservoir=512, seed=0, ridge=lambda ebno_db: 1e-3 if ebno_db > 20 else 1.0,
                            **prec)
    _, c_5 = by_ebno.run([21.0], 16, frames_per_block=16, chunk_blocks=5)
    np.testing.assert_array_equal(c_5, c_r)
