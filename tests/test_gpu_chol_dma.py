"""The LDS-DMA rings of the LDS Cholesky read-out solve (wide orientation, float32 E, Gram dimension <= 128): W_out
and status with chol_dma=1 must equal the register-staged passes (chol_dma=0) bit for bit, and pinv within the
tolerance of tests/test_gpu_chol_packed.py.  Covers group counts, ragged Gram dimensions, column counts that do
and do not fill whole 32-k chunks, a column count that is not a multiple of 4 (the fallback), every n_out and a
rank-deficient group."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def rel_err(got, want):
    return float(np.max(np.abs(got - want)) / (np.max(np.abs(want)) + 1e-300))


@pytest.fixture(scope="module")
def batched():
    from esn_ofdm_mimo_amd import _lib, batched
    yield batched
    _lib.debug_set("chol_dma", "1")


def _bank(batched, cols, n_out):
    return batched.ReservoirBank(cols - 2, n_out, 2, np.zeros((2, 2)), np.zeros((2, cols - 2)), np.zeros((2, n_out)))


def _solve_both(batched, bank, E, D, tr):
    import torch
    from esn_ofdm_mimo_amd import _lib
    E_dev = torch.as_tensor(E, device="cuda")
    out = {}
    for dma in ("0", "1"):
        _lib.debug_set("chol_dma", dma)
        W, status = bank.solve(E_dev, D, tr, method="chol")
        torch.cuda.synchronize()
        out[dma] = (W.clone(), status.clone())
    _lib.debug_set("chol_dma", "1")
    assert torch.equal(out["0"][1], out["1"][1])
    assert torch.equal(out["0"][0], out["1"][0])
    return out["1"]


def _check(batched, G, n, cols, n_out, tr=3, checked=None, seed=0):
    rs = np.random.RandomState(seed + 11 * G + n + cols + n_out)
    bank = _bank(batched, cols, n_out)
    E = rs.randn(G, n + tr, cols)
    E[:, :, :3] *= 1e-2
    D = rs.randn(G, n + tr, n_out)
    t_scale = rs.rand(G, n_out) + 0.5
    bank.set_scaling(None, None, t_scale, None)
    E = E.astype(np.float32)
    W, status = _solve_both(batched, bank, E, D, tr)
    assert int(status.ne(0).sum().item()) == 0
    W = W.cpu().numpy()
    E64 = E.astype(np.float64)
    for g in (range(G) if checked is None else checked):
        want = (np.linalg.pinv(E64[g, tr:]) @ (D[g, tr:] * t_scale[g])).T
        assert rel_err(W[g], want) < 1e-7, g


@pytest.mark.parametrize("G", [1, 7, 2048])
def test_group_counts(batched, G):
    checked = None if G <= 7 else sorted({0, 1, G // 2, G - 2, G - 1})
    _check(batched, G, 128, 528, 8, checked=checked)


@pytest.mark.parametrize("n", [97, 113, 128])
@pytest.mark.parametrize("cols", [528, 316, 300, 222])
def test_ragged_gram_and_columns(batched, n, cols):
    """316 and 300 end in a partial 32-k chunk (300 is not a multiple of 32); 222 is not a multiple of 4 and takes
    the register-staged fallback in both arms."""
    _check(batched, 3, n, cols, 8)


@pytest.mark.parametrize("n_out", list(range(1, 9)))
def test_every_n_out(batched, n_out):
    _check(batched, 2, 120, 528, n_out)


def test_rank_deficient_group(batched):
    import torch
    rs = np.random.RandomState(5)
    G, rows, cols, n_out = 5, 128, 528, 8
    bank = _bank(batched, cols, n_out)
    E = rs.randn(G, rows, cols)
    D = rs.randn(G, rows, n_out)
    E[3, 100] = E[3, 17]
    D[3, 100] = D[3, 17]
    E = E.astype(np.float32)
    W, status = _solve_both(batched, bank, E, D, 0)
    assert list(status.cpu().numpy()) == [0, 0, 0, 1, 0]
    E64 = E.astype(np.float64)
    for g in (0, 1, 2, 4):
        assert rel_err(W[g].cpu().numpy(), (np.linalg.pinv(E64[g]) @ D[g]).T) < 1e-7
    assert torch.isfinite(W[3]).all()
