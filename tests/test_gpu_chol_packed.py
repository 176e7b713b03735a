"""The LDS Cholesky read-out solve (Gram dimension <= 128, two workgroups per CU, packed Gram tiles, blocked
triangular solves) against numpy.linalg.pinv: group counts across odd tails and full residency, ragged Gram
dimensions, every n_out up to 8, the tall orientation, float32 states from a noisy harvest, and a rank-deficient
group among healthy ones."""
import numpy as np
import pytest

from oracle import esn_oracle as eo

pytestmark = pytest.mark.gpu


def rel_err(got, want):
    return float(np.max(np.abs(got - want)) / (np.max(np.abs(want)) + 1e-300))


@pytest.fixture(scope="module")
def batched():
    from esn_ofdm_mimo_amd import batched
    return batched


def _bank(batched, cols, n_out):
    return batched.ReservoirBank(cols - 2, n_out, 2, np.zeros((2, 2)), np.zeros((2, cols - 2)), np.zeros((2, n_out)))


def _pinv_w(E, D, t_scale=None):
    d = D if t_scale is None else D * t_scale
    return (np.linalg.pinv(E) @ d).T


def _check(batched, G, rows, cols, n_out, tr=3, e32=False, checked=None, seed=0):
    import torch
    rs = np.random.RandomState(seed + 7 * G + rows + cols + n_out)
    bank = _bank(batched, cols, n_out)
    E = rs.randn(G, rows + tr, cols)
    E[:, :, :3] *= 1e-2                      # uneven column scales
    D = rs.randn(G, rows + tr, n_out)
    t_scale = rs.rand(G, n_out) + 0.5
    bank.set_scaling(None, None, t_scale, None)
    if e32:
        E = E.astype(np.float32)
        W, status = bank.solve(torch.as_tensor(E, device="cuda"), D, tr, method="chol")
        E = E.astype(np.float64)
    else:
        W, status = bank.solve(E, D, tr, method="chol")
    assert int(status.ne(0).sum().item()) == 0
    W = W.cpu().numpy()
    for g in (range(G) if checked is None else checked):
        assert rel_err(W[g], _pinv_w(E[g, tr:], D[g, tr:], t_scale[g])) < 1e-7, g


@pytest.mark.parametrize("G", [1, 2, 3, 257, 2048])
def test_group_counts(batched, G):
    """Odd tails of the two-per-CU residency and a full device (2048 groups: the headline count)."""
    checked = None if G <= 3 else sorted({0, 1, G // 2, G - 2, G - 1})
    _check(batched, G, 128, 528, 8, e32=True, checked=checked)


@pytest.mark.parametrize("n", [16, 100, 127, 128])
@pytest.mark.parametrize("e32", [False, True])
def test_ragged_gram_dimension(batched, n, e32):
    _check(batched, 3, n, 528, 8, e32=e32)


@pytest.mark.parametrize("n_out", list(range(1, 9)))
def test_every_n_out(batched, n_out):
    _check(batched, 3, 128, 200, n_out, e32=True)
    _check(batched, 2, 77, 130, n_out)


@pytest.mark.parametrize("rows,cols,e32", [(300, 100, False), (300, 100, True), (512, 128, True), (140, 37, False)])
def test_tall_eight_outputs(batched, rows, cols, e32):
    """rows >= cols: A^T B partial sums over 8 x 128 (output, row) pairs on 512 threads."""
    _check(batched, 3, rows, cols, 8, e32=e32)


def test_float32_states_of_a_noisy_harvest(batched):
    """Float32 extended states of the batched harvest (state noise on: cond ~ 1e3), the bench's fit shape."""
    import torch
    rs = np.random.RandomState(31)
    n_in, n_out, n_res, t, tr, G = 16, 8, 512, 138, 10, 5
    w, w_in, w_fb = eo.draw_weights(rs, n_in, n_out, n_res, 0.9, 0.1)
    bank = batched.ReservoirBank(n_in, n_out, n_res, w, w_in, w_fb, noise=1e-3)
    t_scale = rs.rand(G, n_out) + 0.5
    bank.set_scaling(rs.rand(G, n_in) * 0.2 + 0.1, None, t_scale, None)
    u, d = rs.randn(G, t, n_in), rs.randn(G, t, n_out) * 0.3
    e32 = bank.harvest(u, d, precision="f16", noise_mode="counter", seed=4, e_dtype="f32")
    assert e32.dtype == torch.float32
    W, status = bank.solve(e32, d, tr, method="chol")
    assert int(status.ne(0).sum().item()) == 0
    E = e32.cpu().numpy().astype(np.float64)
    W = W.cpu().numpy()
    for g in range(G):
        assert np.linalg.cond(E[g, tr:]) > 10.0
        assert rel_err(W[g], _pinv_w(E[g, tr:], d[g, tr:], t_scale[g])) < 1e-7, g


@pytest.mark.parametrize("e32", [False, True])
def test_rank_deficient_group_among_healthy_ones(batched, e32):
    """Only the singular group is flagged; its neighbours' W_out equal a solve without it, bit for bit."""
    import torch
    rs = np.random.RandomState(12)
    G, rows, cols, n_out = 5, 128, 528, 8
    bank = _bank(batched, cols, n_out)
    E = rs.randn(G, rows, cols)
    D = rs.randn(G, rows, n_out)
    E[2, 90] = E[2, 41]
    D[2, 90] = D[2, 41]
    if e32:
        E = E.astype(np.float32)
    dev = lambda x: torch.as_tensor(x, device="cuda")
    W, status = bank.solve(dev(E), D, 0, method="chol")
    assert list(status.cpu().numpy()) == [0, 0, 1, 0, 0]
    keep = [0, 1, 3, 4]
    W_alone, st_alone = bank.solve(dev(E[keep]), D[keep], 0, method="chol")
    assert int(st_alone.ne(0).sum().item()) == 0
    assert np.array_equal(W.cpu().numpy()[keep], W_alone.cpu().numpy())
    E64 = E.astype(np.float64)
    for g in keep:
        assert rel_err(W[g].cpu().numpy(), _pinv_w(E64[g], D[g])) < 1e-7
    n = bank.resolve_failed(dev(E64), D, 0, W, status)
    assert n == 1
    assert rel_err(E64[2] @ W[2].cpu().numpy().T, D[2]) < 1e-6
