"""Leave-one-out choice of the ridge parameter (esn_readout_ridge_loo_batch[_f32]) through every layer:
scores against the closed form of tests/loo_ref.py (itself pinned to a brute-force refit by test_loo_reference_cpu.py),
the choice, W_out at the chosen lambda, bad / failing / equal candidates, batch invariance, ReservoirBank.fit, the
drop-in ESN, DetectorSweep, and the BER the choice buys at the headline shape.

Tolerances.  Scores: 1e-6 relative -- the project grants a Cholesky solution 1e-7 (test_readout_solve_vs_pinv); the
score squares a quotient of two such quantities, to first order 2 x (1e-7 + 1e-7) = 4e-7, rounded up; two float64
formulations of the reference differ by <= 1e-10 on these inputs.  Choice: an index whose reference score is within
2e-6 of the reference minimum, after asserting that the reference's best and second best are >= 1e-2 apart (so exactly
one index qualifies; loo_ref.make_case draws the inputs with a margin of 2e-2 in the reference).  W_out: 1e-7 of
max|W| against the SVD ridge at the chosen lambda; it is not bitwise the Cholesky ridge solve's (this
kernel solves through the inverse factor in another summation order), so the 1e-7 stands."""
import os
import sys

import numpy as np
import pytest

from oracle import esn_oracle as eo

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loo_ref  # noqa: E402

pytestmark = pytest.mark.gpu

TR = 5
SCORE_TOL, CHOICE_TOL, MARGIN, W_TOL = 1e-6, 2e-6, 1e-2, 1e-7
MULT = np.array(loo_ref.GRID_MULT)
# name: rows, cols, n_out
SHAPES = {
    "wide_24x40": (24, 40, 2),
    "wide_ragged_100x140": (100, 140, 4),
    "wide_headline_128x528": (128, 528, 8),
    "square_128x128": (128, 128, 8),
    "tall_200x104": (200, 104, 4),
    "tall_60x17": (60, 17, 1),
}


def rel_err(got, want):
    return float(np.max(np.abs(got - want)) / (np.max(np.abs(want)) + 1e-300))


@pytest.fixture(scope="module")
def batched():
    from esn_ofdm_mimo_amd import batched
    return batched


def _bank(batched, cols, n_out):
    return batched.ReservoirBank(cols - 2, n_out, 2, np.zeros((2, 2)), np.zeros((2, cols - 2)), np.zeros((2, n_out)))


_CASES = {}


def case(batched, name, G, f32):
    """One shape, drawn once: bank, E on the device, D, t_scale, float64 fit rows, scaled teacher, grid [G, L],
    reference scores [G, L]."""
    key = (name, G, f32)
    if key not in _CASES:
        import torch
        rows, cols, n_out = SHAPES[name]
        E, D, t_scale = loo_ref.make_case(rows, cols, n_out, G, 1000 * rows + cols + G, transient=TR,
                                          min_margin=2 * MARGIN, f32=f32)
        if f32:
            E = E.astype(np.float32)
        bank = _bank(batched, cols, n_out)
        E_dev = torch.as_tensor(E, device="cuda")
        E64 = E.astype(np.float64)[:, TR:]
        Ds = D[:, TR:] * t_scale[:, None, :]
        grid = np.stack([loo_ref.gram_mean_diag(E64[g]) * MULT for g in range(G)])
        ref = np.stack([loo_ref.scores(E64[g], Ds[g], grid[g]) for g in range(G)])
        _CASES[key] = (bank, E_dev, D, t_scale, E64, Ds, grid, ref)
    return _CASES[key]


def run(bank, E_dev, D, t_scale, grid, tr=TR):
    """solve(ridge_grid=) -> W_out, status, scores, choice, per-entry status as NumPy copies."""
    bank.set_scaling(None, None, t_scale, None)
    W, st = bank.solve(E_dev, D, tr, ridge_grid=grid)
    return (W.cpu().numpy(), st.cpu().numpy(), bank.last_ridge_scores.cpu().numpy(),
            bank.last_ridge_choice.cpu().numpy(), bank.last_ridge_status.cpu().numpy())


# ---- 1: scores, choice, W_out -------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("G", [1, 5])
@pytest.mark.parametrize("name", list(SHAPES))
def test_scores_choice_and_w_out(batched, name, G, f32):
    bank, E_dev, D, t_scale, E64, Ds, grid, ref = case(batched, name, G, f32)
    W, st, score, choice, st_l = run(bank, E_dev, D, t_scale, grid)
    rows, cols, n_out = SHAPES[name]
    assert W.shape == (G, n_out, cols) and st.shape == (G,) and score.shape == (G, len(MULT)) and choice.shape == (G,)
    assert choice.dtype == np.int32 and not st.any() and not st_l.any()
    lam_dev = bank.last_ridge_lambda.cpu().numpy()
    for g in range(G):
        err = np.abs(score[g] - ref[g]) / ref[g]
        best = float(np.min(ref[g]))
        print(f"{name} G={G} {'f32' if f32 else 'f64'} g={g}: score rel err max {err.max():.3e}, "
              f"ref margin {loo_ref.margin(ref[g]):.3f}, choice {choice[g]} (ref {int(np.argmin(ref[g]))})")
        assert np.all(err <= SCORE_TOL), (g, err)
        assert loo_ref.margin(ref[g]) >= MARGIN
        assert 0 <= choice[g] < len(MULT)
        assert ref[g, choice[g]] - best <= CHOICE_TOL * best, (g, choice[g], ref[g])
        assert lam_dev[g] == grid[g, choice[g]]
        w_err = rel_err(W[g], loo_ref.ridge_svd(E64[g], Ds[g], grid[g, choice[g]]))
        print(f"    W_out rel err {w_err:.3e}")
        assert w_err <= W_TOL, (g, w_err)


# ---- 2: bad candidates ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,f32", [("wide_24x40", False), ("wide_headline_128x528", True), ("tall_200x104", False)])
def test_negative_nan_and_inf_candidates(batched, name, f32):
    bank, E_dev, D, t_scale, E64, Ds, grid, ref = case(batched, name, 5, f32)
    _, _, score0, choice0, _ = run(bank, E_dev, D, t_scale, grid)
    bad_grid = grid.copy()
    bad_grid[0, int(choice0[0])] = -1.0          # the winner itself goes: the runner-up must take over
    bad_grid[1, 0] = np.nan
    bad_grid[2, 6] = np.inf
    bad_grid[4, 2] = -np.inf
    bad = ~np.isfinite(bad_grid) | (bad_grid < 0)
    W, st, score, choice, st_l = run(bank, E_dev, D, t_scale, bad_grid)
    np.testing.assert_array_equal(st_l, np.where(bad, 2, 0))
    assert np.all(np.isposinf(score[bad]))
    np.testing.assert_array_equal(score[~bad], score0[~bad])                    # the neighbours, bit for bit
    assert not st.any()
    for g in range(5):
        assert not bad[g, choice[g]]
        assert choice[g] == int(np.argmin(np.where(bad[g], np.inf, ref[g])))


def _rank_deficient(batched):
    rs = np.random.RandomState(8)
    n_g, rows, cols, n_out = 3, 20, 50, 2
    bank = _bank(batched, cols, n_out)
    E = rs.randn(n_g, rows, cols)
    D = rs.randn(n_g, rows, n_out)
    E[1, 7] = E[1, 3]
    D[1, 7] = D[1, 3]                       # consistent duplicate, as in test_gpu_ridge.py
    return bank, E, D


def test_failed_pivot_flags_its_entry_only(batched):
    """A duplicated row leaves K singular in float64 at lambda = 1e-300: that entry gets status 1 and score +inf, the
    other candidates of the group and the other groups are scored as if it were not there."""
    import torch
    bank, E, D = _rank_deficient(batched)
    md = np.array([loo_ref.gram_mean_diag(E[g]) for g in range(3)])
    grid = np.stack([[1e-300, 1e-3 * md[g], 1e-1 * md[g]] for g in range(3)])
    W, st, score, choice, st_l = run(bank, torch.as_tensor(E, device="cuda"), D, None, grid, tr=0)
    np.testing.assert_array_equal(st_l, [[0, 0, 0], [1, 0, 0], [0, 0, 0]])
    assert np.isposinf(score[1, 0]) and np.isfinite(np.delete(score.ravel(), 3)).all()
    assert not st.any() and choice[1] in (1, 2)
    for l in (1, 2):
        want = loo_ref.closed_form(E[1], D[1], grid[1, l])
        assert abs(score[1, l] - want) <= SCORE_TOL * want
    assert rel_err(W[1], loo_ref.ridge_svd(E[1], D[1], grid[1, choice[1]])) <= W_TOL


def test_no_surviving_candidate_and_its_repair(batched):
    import torch
    bank, E, D = _rank_deficient(batched)
    md = loo_ref.gram_mean_diag(E[0])
    grid = np.array([[1e-3 * md, 1e-1 * md, 1e1 * md], [1e-300, np.nan, -1.0], [1e-3 * md, 1e-1 * md, 1e1 * md]])
    bank.set_scaling(None, None, None, None)
    E_dev = torch.as_tensor(E, device="cuda")
    W, st = bank.solve(E_dev, D, 0, ridge_grid=grid)
    assert bank.last_ridge_choice.cpu().numpy().tolist() == [bank.last_ridge_choice[0].item(), -1, bank.last_ridge_choice[2].item()]
    assert int(bank.last_ridge_choice[1]) == -1
    np.testing.assert_array_equal(bank.last_ridge_status.cpu().numpy()[1], [1, 2, 2])
    assert np.all(np.isposinf(bank.last_ridge_scores.cpu().numpy()[1]))
    assert list(st.cpu().numpy()) == [0, 1, 0]
    assert float(W[1].abs().max()) == 0.0
    assert np.isnan(float(bank.last_ridge_lambda[1]))
    before = W.clone()
    assert bank.resolve_failed(E_dev, D, 0, W, st, ridge_grid=grid) == 1
    # (the QR solve's own status: 1 here, it sees the duplicated row at lambda = 1e-300 as rank deficient and
    #  answers as pinv would -- test_repair_keeps_lambda's case)
    _, st_qr = bank.solve(E_dev[1:2].contiguous(), D[1:2], 0, method="qr", ridge=1e-300)
    assert list(st.cpu().numpy()) == [0, int(st_qr[0]), 0]
    assert torch.equal(W[0], before[0]) and torch.equal(W[2], before[2])
    assert float(bank.last_ridge_lambda[1]) == 1e-300                           # the largest finite candidate
    got = E[1] @ W[1].cpu().numpy().T
    assert rel_err(got, E[1] @ loo_ref.ridge_svd(E[1], D[1], 1e-300).T) < 1e-6  # (test_repair_keeps_lambda's bound)
    with pytest.raises(ValueError):
        bank.solve(E_dev, D, 0, ridge=1e-3, ridge_grid=grid)


@pytest.mark.parametrize("name", ["wide_ragged_100x140", "tall_60x17"])
def test_equal_candidates_lower_index_wins_and_single_candidate(batched, name):
    bank, E_dev, D, t_scale, E64, Ds, grid, ref = case(batched, name, 5, False)
    best = np.argmin(ref, axis=1)
    dup = np.stack([[grid[g, 0], grid[g, best[g]], grid[g, best[g]], grid[g, 6]] for g in range(5)])
    W, st, score, choice, _ = run(bank, E_dev, D, t_scale, dup)
    np.testing.assert_array_equal(score[:, 1], score[:, 2])
    expect = np.where(best == 0, 0, 1)
    np.testing.assert_array_equal(choice, expect)
    # L = 1: that lambda's solution, choice 0
    one = grid[:, 3:4].copy()
    W1, st1, score1, choice1, _ = run(bank, E_dev, D, t_scale, one)
    assert score1.shape == (5, 1) and not choice1.any() and not st1.any()
    for g in range(5):
        assert abs(score1[g, 0] - ref[g, 3]) <= SCORE_TOL * ref[g, 3]
        assert rel_err(W1[g], loo_ref.ridge_svd(E64[g], Ds[g], one[g, 0])) <= W_TOL
    # a plain sequence is one grid for every group
    W2, _, score2, _, _ = run(bank, E_dev, D, t_scale, list(grid[0]))
    W3, _, score3, _, _ = run(bank, E_dev, D, t_scale, np.tile(grid[0], (5, 1)))
    np.testing.assert_array_equal(score2, score3)
    np.testing.assert_array_equal(W2, W3)


def test_limits_are_named(batched):
    import torch
    bank = _bank(batched, 140, 2)
    E = torch.zeros((1, 130, 140), dtype=torch.float64, device="cuda")
    D = np.zeros((1, 130, 2))
    with pytest.raises(ValueError, match="128"):
        bank.solve(E, D, 0, ridge_grid=[1.0, 2.0])
    with pytest.raises(ValueError, match="16"):
        bank.solve(E[:, :100], D[:, :100], 0, ridge_grid=list(np.arange(1.0, 18.0)))
    with pytest.raises(ValueError):
        bank.solve(E[:, :100], D[:, :100], 0, ridge_grid=np.ones((2, 3)))


# ---- 3: batch invariance ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_group_alone_and_inside_a_batch_bitwise(batched, name, f32):
    bank, E_dev, D, t_scale, _, _, grid, _ = case(batched, name, 5, f32)
    W, _, score, choice, _ = run(bank, E_dev, D, t_scale, grid)
    W1, _, score1, choice1, _ = run(bank, E_dev[3:4].contiguous(), D[3:4], t_scale[3:4], grid[3:4])
    bank.set_scaling(None, None, t_scale, None)
    np.testing.assert_array_equal(score1[0], score[3])
    assert choice1[0] == choice[3]
    np.testing.assert_array_equal(W1[0], W[3])


# ---- 4: through the layers ----------------------------------------------------------------------------------------
DROPIN_GRID = (1e-8, 1e-6, 1e-4, 1e-2, 1.0)


def test_dropin_fit_and_predict_with_a_grid():
    from esn_ofdm_mimo_amd import pyESN
    rs = np.random.RandomState(3)
    t, tr = 200, 10
    u = rs.randn(t, 3)
    d = np.tanh(u @ rs.randn(3, 2)) + 0.3 * np.roll(u[:, :2], 1, axis=0) + 0.05 * rs.randn(t, 2)
    u2 = rs.randn(40, 3)
    esn = pyESN.ESN(3, 2, n_reservoir=80, noise=0, random_state=42, ridge_grid=DROPIN_GRID)
    esn.fit(u, d, tr)
    assert esn.fit_status == 0
    o = eo.OracleESN(3, 2, n_reservoir=80, noise=0, random_state=42)
    o.fit(u, d, tr)
    ext = o._ext_states[tr:]
    idx, ref = loo_ref.choose(ext, o.scale_teacher(d)[tr:], DROPIN_GRID)
    print(f"reference scores {ref}, margin {loo_ref.margin(ref):.3f}, pick {idx}; ESN picked {esn.ridge_choice_} "
          f"(lambda {esn.ridge_:g}), scores {esn.ridge_scores_}")
    assert loo_ref.margin(ref) >= MARGIN
    assert esn.ridge_choice_ == idx and esn.ridge_ == DROPIN_GRID[idx]
    assert np.all(np.abs(esn.ridge_scores_ - ref) <= SCORE_TOL * ref)
    o.W_out = loo_ref.ridge_svd(ext, o.scale_teacher(d)[tr:], DROPIN_GRID[idx])
    assert rel_err(ext @ esn.W_out.T, ext @ o.W_out.T) < 1e-8
    assert rel_err(esn.predict(u2, 0, continuation=True), o.predict(u2, 0, continuation=True)) < 1e-8
    with pytest.raises(ValueError):
        pyESN.ESN(3, 2, n_reservoir=8, ridge=1e-3, ridge_grid=DROPIN_GRID)
    # without a grid, ridge_ is the ridge that was given
    plain = pyESN.ESN(3, 2, n_reservoir=80, noise=0, random_state=42, ridge=1e-3)
    plain.fit(u, d, tr)
    assert plain.ridge_ == 1e-3


def test_bank_fit_with_one_candidate_is_fit_with_that_ridge():
    from esn_ofdm_mimo_amd import batched as bt, pyESN, helper_mimo_esn_generic as hg
    rs = np.random.RandomState(3)
    t, tr, lam = 200, 10, 1e-3
    u = rs.randn(t, 3)
    d = np.tanh(u @ rs.randn(3, 2)) + 0.3 * np.roll(u[:, :2], 1, axis=0)
    b = pyESN.ESN(3, 2, n_reservoir=80, noise=0, random_state=42)
    bank = bt.ReservoirBank(3, 2, 80, b.W, b.W_in, b.W_feedb, noise=0.0)
    U, D = np.stack([u, u[::-1]]), np.stack([d, d[::-1]])
    bank.fit(U, D, transient=tr, precision="f64", noise_mode="none", ridge=lam)
    w_ridge = bank.W_out.cpu().numpy().copy()
    bank.fit(U, D, transient=tr, precision="f64", noise_mode="none", ridge_grid=[lam])
    assert int(bank.fit_status.ne(0).sum().item()) == 0
    assert bank.fit_ridge.shape == (2,) and bank.fit_ridge.cpu().numpy().tolist() == [lam, lam]
    for g in range(2):
        assert rel_err(bank.W_out[g].cpu().numpy(), w_ridge[g]) <= 1e-7
    with pytest.raises(ValueError):
        bank.fit(U, D, transient=tr, precision="f64", noise_mode="none", ridge=lam, ridge_grid=[lam])
    # the batch trainer hands the grid on: [G, L], one group per candidate order
    yc = (u[:, :2] + 1j * u[:, 1:3])[None].repeat(2, axis=0)
    xc = (d[:, :1] + 1j * d[:, 1:2])[None].repeat(2, axis=0)
    bank2 = bt.ReservoirBank(4, 2, 80, b.W, rs.rand(80, 4) * 2 - 1, b.W_feedb, noise=0.0)
    hg.trainMIMOESN_batch(bank2, yc, xc, 1, 4, noise_mode="none", ridge_grid=np.array([[1e-4, 1e-2], [1e-2, 1e-4]]))
    ch = bank2.last_ridge_choice.cpu().numpy()
    assert ch[0] + ch[1] == 1                   # the same pilot twice: the same lambda, at swapped indices
    assert float(bank2.last_ridge_lambda[0]) == float(bank2.last_ridge_lambda[1])


def test_sweep_counts_every_block_once():
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep, LinkParams
    grid = (1e-4, 1e-2, 1.0)
    sweep = DetectorSweep(LinkParams(), n_reservoir=100, seed=0, ridge_grid=grid)
    _, c = sweep.run([6.0, 21.0], 7, frames_per_block=2, chunk_blocks=3)
    assert set(sweep.ridge_choice_counts) == {6.0, 21.0}
    for ebno in (6.0, 21.0):
        n = sweep.ridge_choice_counts[ebno]
        print(f"{ebno} dB: picks {n}")
        assert n.dtype == np.int64 and n.shape == (3,) and int(n.sum()) == 7
    _, c1 = sweep.run([6.0, 21.0], 7, frames_per_block=2)
    np.testing.assert_array_equal(c1, c)
    with pytest.raises(ValueError):
        DetectorSweep(LinkParams(), n_reservoir=100, seed=0, ridge=1e-3, ridge_grid=grid)


# ---- 5: the gain reaches the user -----------------------------------------------------------------------------------
GAIN_GRID = (1e-4, 3e-4, 1e-3, 3e-3, 1e-2, 3e-2, 0.1)


@pytest.mark.parametrize("prec", [dict(), dict(fit_precision="f16", precision="f16")], ids=["default", "f16"])
def test_the_choice_reaches_the_user(prec):
    """The shape of test_the_gain_reaches_the_user: 4x8 TDL-B, N = 128, 16-QAM, N_res = 512, 16 blocks x 16 data
    frames, the same seed for every leg.  At 21 dB the LOO choice beats pinv by the cap that test uses (0.95; the
    float64 CPU oracle gives 0.72), and at 21 and 6 dB it is within 1.05 of the best fixed lambda of the same grid
    (oracle: 1.000 and 1.016; 1.05 leaves room for the smaller sample)."""
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep, LinkParams
    ebno = [6.0, 21.0]
    loo = DetectorSweep(LinkParams(), n_reservoir=512, seed=0, ridge_grid=GAIN_GRID, **prec)
    ber_l, c_l = loo.run(ebno, 16, frames_per_block=16)
    assert c_l[0, 1] == c_l[1, 1] == 16 * 16 * 128 * 4 * 4
    assert loo.fits_repaired == 0
    for e in ebno:
        assert int(loo.ridge_choice_counts[e].sum()) == 16
    fixed = DetectorSweep(LinkParams(), n_reservoir=512, seed=0, ridge=None, **prec)     # one reservoir, every leg
    ber_p, _ = fixed.run(ebno, 16, frames_per_block=16)
    ber_f = []
    for lam in GAIN_GRID:
        fixed.ridge = lam
        ber_f.append(fixed.run(ebno, 16, frames_per_block=16)[0])
    ber_f = np.array(ber_f)                                                               # [L, 2]
    for i, e in enumerate(ebno):
        print(f"{e} dB: pinv {ber_p[i]:.5f} fixed {np.array2string(ber_f[:, i], precision=5)} LOO {ber_l[i]:.5f} "
              f"picks {loo.ridge_choice_counts[e]}  LOO/pinv {ber_l[i] / ber_p[i]:.4f} "
              f"LOO/best fixed {ber_l[i] / ber_f[:, i].min():.4f}")
    assert ber_l[1] <= 0.95 * ber_p[1]
    assert ber_l[1] <= 1.05 * ber_f[:, 1].min()
    assert ber_l[0] <= 1.05 * ber_f[:, 0].min()
