"""esn_readout_holdout_score[_f32] (csrc/esn_holdout.hip) on the device, through
ReservoirBank.holdout_choose and the typed entry points, against tests/multipilot_ref.py (pinned to an independent form
by test_holdout_reference_cpu.py).

Shapes: every value of cols in {5, 24, 132, 528} (5 is no multiple of 4: the scalar loads; 24 is less than one chunk of
32 columns; 132 is four chunks and a tail of 4; 528 is the headline), held-out rows in {1, 17, 128}, n_out in {1, 2, 8},
n_ridge in {1, 3, 16}, transient in {0, 10} and G in {1, 37}, in a covering set instead of the full product, float64 and
float32 E each; and two cases of more than 128 rows, where the kernel makes a second pass over W.

Tolerance (derived, not tuned): every residual is a dot product of `cols` terms, a scaling and a subtraction, so in any
summation order |r - r_exact| <= b[i][o] = (cols + 2) 2^-53 (sum_c |E W| + |D_s|), and then
|score - ref| <= 2 sqrt(ref) |b|_2 + |b|_2^2 (multipilot_ref.score_bound).  The choice is compared exactly, on inputs
whose two best reference scores are more than twice that bound apart (asserted on the reference side)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multipilot_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

# cols, held-out rows, n_out, n_ridge, transient, G, teacher shift given
CASES = [
    (5, 1, 1, 1, 0, 1, False), (5, 17, 2, 3, 10, 37, True), (5, 128, 8, 16, 0, 37, False),
    (24, 17, 8, 1, 0, 37, True), (24, 1, 2, 16, 10, 1, False), (24, 128, 1, 3, 10, 37, False),
    (132, 128, 2, 16, 0, 1, True), (132, 17, 1, 16, 10, 37, False), (132, 1, 8, 3, 0, 37, False),
    (528, 128, 8, 16, 10, 37, True), (528, 17, 2, 1, 10, 1, False), (528, 1, 1, 3, 0, 37, False),
    (40, 200, 3, 5, 3, 5, True), (528, 300, 8, 16, 0, 2, False),
]
IDS = ["c%d_r%d_o%d_l%d_t%d_g%d%s" % (*c[:6], "_shift" if c[6] else "") for c in CASES]


@pytest.fixture(scope="module")
def batched():
    from esn_ofdm_mimo_amd import batched
    return batched


def _bank(batched, cols, n_out):
    return batched.ReservoirBank(cols - 2, n_out, 2, np.zeros((2, 2)), np.zeros((2, cols - 2)), np.zeros((2, n_out)))


_DRAWN = {}


def draw(cols, rows, n_out, L, tr, G, shift, f32):
    """Held-out states with uneven column scales, a teacher that is a linear map of them plus noise, and candidates
    that miss that map by L different, well separated amounts (in a shuffled order, so the winner's index moves from
    group to group).  Drawn once per case; returns E [G, T, cols] (float32 if f32), D, W [G, L, n_out, cols], t_scale,
    t_shift or None, and the reference scores / bounds [G, L] on exactly what the device is given."""
    key = (cols, rows, n_out, L, tr, G, shift, f32)
    if key not in _DRAWN:
        rs = np.random.RandomState(1000 * cols + 10 * rows + n_out + L + G)
        T = rows + tr
        E = rs.randn(G, T, cols) * 10.0 ** rs.uniform(-2.0, 0.0, size=(G, 1, cols))
        if f32:
            E = E.astype(np.float32)
        E64 = E.astype(np.float64)
        truth = rs.randn(G, n_out, cols)
        t_scale = rs.rand(G, n_out) + 0.5
        t_shift = 0.1 * rs.randn(G, n_out) if shift else None
        clean = np.einsum("gtc,goc->gto", E64, truth)
        Ds = clean + 0.05 * np.std(clean) * rs.randn(G, T, n_out)
        D = (Ds - (t_shift[:, None, :] if shift else 0.0)) / t_scale[:, None, :]
        miss = np.stack([0.05 * (1 + rs.permutation(L)) for _ in range(G)])                 # [G, L], all different
        W = truth[:, None] + miss[:, :, None, None] * rs.randn(G, L, n_out, cols)
        Ds_dev = D * t_scale[:, None, :] + (t_shift[:, None, :] if shift else 0.0)           # as the kernel scales it
        want = np.stack([ref.holdout_scores(E64[g, tr:], Ds_dev[g, tr:], W[g]) for g in range(G)])
        bound = np.stack([ref.score_bound(E64[g, tr:], Ds_dev[g, tr:], W[g]) for g in range(G)])
        _DRAWN[key] = (E, D, W, t_scale, t_shift, want, bound)
    return _DRAWN[key]


def choose(batched, case, f32, status=None, W=None, groups=slice(None)):
    import torch
    cols, rows, n_out, L, tr, G, shift = case
    E, D, W0, t_scale, t_shift, _, _ = draw(*case, f32)
    bank = _bank(batched, cols, n_out)
    bank.set_scaling(None, None, t_scale[groups], None if t_shift is None else t_shift[groups])
    s, c = bank.holdout_choose(torch.as_tensor(E[groups], device="cuda"), D[groups], tr, (W0 if W is None else W)[groups],
                               None if status is None else status[groups])
    assert s.dtype == torch.float64 and c.dtype == torch.int32
    return s.cpu().numpy(), c.cpu().numpy()


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_scores_and_choice_against_the_restatement(batched, case, f32):
    cols, rows, n_out, L, tr, G, shift = case
    _, _, _, _, _, want, bound = draw(*case, f32)
    score, choice = choose(batched, case, f32)
    assert score.shape == (G, L) and choice.shape == (G,)
    ratio = np.abs(score - want) / bound
    two = np.sort(want, axis=1)[:, :2]
    gap = (two[:, 1] - two[:, 0]) / (2 * np.sort(bound, axis=1)[:, -1]) if L > 1 else np.full(G, np.inf)
    print(f"{IDS[CASES.index(case)]} {'f32' if f32 else 'f64'}: |score - ref| / bound max {ratio.max():.3e}, "
          f"rel err max {(np.abs(score - want) / want).max():.3e}, best-two gap / (2 bound) min {gap.min():.3e}")
    assert np.all(ratio <= 1.0), ratio.max()
    assert np.all(gap > 1.0)                                    # the winner is a fact of the data, not of the last bits
    np.testing.assert_array_equal(choice, np.argmin(want, axis=1))


MASK_CASE = CASES[9]            # the headline shape: 16 candidates x 8 outputs, 37 groups


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_masked_and_non_finite_candidates_never_win(batched, f32):
    cols, rows, n_out, L, tr, G, shift = MASK_CASE
    _, _, W, _, _, want, _ = draw(*MASK_CASE, f32)
    score0, choice0 = choose(batched, MASK_CASE, f32)
    status = np.zeros((G, L), dtype=np.int32)
    W2 = W.copy()
    for g in range(G):
        status[g, choice0[g]] = 1 + g % 2                      # the winner itself goes (a pivot failure, a bad lambda)
    status[3] = 1                                               # nobody left
    status[4] = 0
    W2[4, choice0[4], n_out - 1, cols - 1] = np.nan             # the winner's read-out is not finite
    W2[5, (choice0[5] + 1) % L, 0, 0] = np.inf
    score, choice = choose(batched, MASK_CASE, f32, status=status, W=W2)
    gone = status != 0
    gone[4, choice0[4]] = gone[5, (choice0[5] + 1) % L] = True
    assert np.all(np.isposinf(score[gone]))
    np.testing.assert_array_equal(score[~gone], score0[~gone])                  # the neighbours, bit for bit
    assert choice[3] == -1
    for g in range(G):
        if g != 3:
            assert choice[g] == int(np.argmin(np.where(gone[g], np.inf, want[g]))) and not gone[g, choice[g]]


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_every_output_is_written(batched, f32):
    """The typed entry point on tensors filled with a sentinel, status_in NULL and given."""
    import torch
    from esn_ofdm_mimo_amd import _lib
    lib = _lib.load()
    case = CASES[1]
    cols, rows, n_out, L, tr, G, shift = case
    E, D, W, t_scale, t_shift, want, bound = draw(*case, f32)
    dev = dict(device="cuda")
    Et, Dt, Wt = torch.as_tensor(E, **dev), torch.as_tensor(D, **dev), torch.as_tensor(W, **dev)
    ts, th = torch.as_tensor(t_scale, **dev), torch.as_tensor(t_shift, **dev)
    fn = lib.esn_readout_holdout_score_f32 if f32 else lib.esn_readout_holdout_score
    for masked in (False, True):
        score = torch.full((G, L), -7.0, dtype=torch.float64, **dev)
        choice = torch.full((G,), -77, dtype=torch.int32, **dev)
        st = torch.ones((G, L), dtype=torch.int32, **dev) if masked else None
        rc = fn(Et.data_ptr(), Dt.data_ptr(), Wt.data_ptr(), G, rows + tr, tr, cols, n_out, ts.data_ptr(), th.data_ptr(), L,
                None if st is None else st.data_ptr(), score.data_ptr(), choice.data_ptr(), _lib.stream_handle())
        assert rc == 0, lib.esn_last_error()
        s, c = score.cpu().numpy(), choice.cpu().numpy()
        if masked:
            assert np.all(np.isposinf(s)) and np.all(c == -1)
        else:
            assert np.all(np.abs(s - want) <= bound) and np.all((c >= 0) & (c < L))


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("case", [CASES[9], CASES[1], CASES[12]], ids=[IDS[9], IDS[1], IDS[12]])
def test_a_group_alone_is_bitwise_itself_inside_the_batch(batched, case, f32):
    G = case[5]
    score, choice = choose(batched, case, f32)
    for g in (0, G // 2, G - 1):
        s1, c1 = choose(batched, case, f32, groups=slice(g, g + 1))
        assert s1.tobytes() == score[g:g + 1].tobytes() and c1[0] == choice[g], g


def test_refusals_of_holdout_choose(batched):
    import torch
    bank = _bank(batched, 24, 2)
    E, D = torch.zeros((2, 9, 24), device="cuda", dtype=torch.float64), np.zeros((2, 9, 2))
    with pytest.raises(ValueError, match="candidates"):
        bank.holdout_choose(E, D, 0, np.zeros((2, 17, 2, 24)))
    with pytest.raises(ValueError, match="W_cand must be"):
        bank.holdout_choose(E, D, 0, np.zeros((2, 3, 2, 23)))
    with pytest.raises(ValueError, match="status must be"):
        bank.holdout_choose(E, D, 0, np.zeros((2, 3, 2, 24)), status=np.zeros((2, 4), dtype=np.int32))
    from esn_ofdm_mimo_amd import _lib
    with pytest.raises(_lib.EsnHipError, match="transient"):
        bank.holdout_choose(E, D, 9, np.zeros((2, 3, 2, 24)))
