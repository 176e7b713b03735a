"""The read-out fit (readout.ReadoutFit) and the scalings (bankbase.DeviceBank) are one piece of code on every bank that
inherits them: float64, no cluster path.

1. ReservoirBank.solve and ElmBank.solve give the same bytes on the same rows, teacher and teacher scalings -- QR and
   Cholesky, pinv and ridge [G, 2], and the leave-one-out choice among three candidates with its record read off each
   bank itself -- for a tall system (16 rows x 10 columns) and a wide one (16 x 24, the minimum-norm case).
2. ElmBank.resolve_failed repairs a group flagged by hand: its row is bitwise a QR solve of that group alone under its
   own teacher scalings; the other rows stay.
3. ElmBank and FnnBank keep the four scaling tensors they are given, once: no `_ro`, and a bank whose four attributes
   were assigned directly fits / trains and predicts what a bank after set_scaling does."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G, T, TRANSIENT, N_OUT = 3, 20, 4, 4
COLS = (10, 24)
GRID = [1e-6, 1e-3, 1e-1]
_cache = {}


def system(cols):
    """(ReservoirBank, ElmBank with n_hidden = cols - 1, E, D, t_scale, t_shift) of `cols` columns; made once."""
    if cols not in _cache:
        import torch
        from esn_ofdm_mimo_amd.batched import ReservoirBank
        from esn_ofdm_mimo_amd.elm import ElmBank
        rs = np.random.RandomState(100 + cols)
        E = torch.as_tensor(rs.randn(G, T, cols), device="cuda")
        D = torch.as_tensor(rs.randn(G, T, N_OUT), device="cuda")
        t_scale = torch.as_tensor(0.5 + rs.rand(G, N_OUT), device="cuda")
        t_shift = torch.as_tensor(0.1 * rs.randn(G, N_OUT), device="cuda")
        esn = ReservoirBank(cols - 2, N_OUT, 2, np.zeros((2, 2)), np.zeros((2, cols - 2)), np.zeros((2, N_OUT)))
        elm = ElmBank(2, N_OUT, cols - 1, 1, np.zeros((cols - 1, 2)), np.zeros(cols - 1))
        for bank in (esn, elm):
            bank.set_scaling(None, None, t_scale, t_shift)
        _cache[cols] = esn, elm, E, D, t_scale, t_shift
    return _cache[cols]


def ridge_gl():
    import torch
    return torch.as_tensor([[1e-3, 0.5], [0.0, 1e-2], [2.0, 1e-6]], dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("method", ["qr", "chol"])
@pytest.mark.parametrize("ridge", [False, True], ids=["pinv", "ridge"])
def test_both_banks_solve_the_same_bytes(cols, method, ridge):
    import torch
    esn, elm, E, D, _, _ = system(cols)
    kw = {"ridge": ridge_gl()} if ridge else {}
    W_a, st_a = esn.solve(E, D, TRANSIENT, method=method, **kw)
    W_b, st_b = elm.solve(E, D, TRANSIENT, method=method, **kw)
    assert tuple(W_a.shape) == ((G, 2, N_OUT, cols) if ridge else (G, N_OUT, cols))
    assert st_a.cpu().tolist() == ([[0, 0]] * G if ridge else [0] * G)
    assert torch.equal(W_a, W_b) and torch.equal(st_a, st_b)
    assert bool(W_a.abs().sum() > 0)


@pytest.mark.parametrize("cols", COLS)
def test_both_banks_choose_the_same_ridge_and_keep_the_record_themselves(cols):
    import torch
    esn, elm, E, D, _, _ = system(cols)
    W_a, st_a = esn.solve(E, D, TRANSIENT, ridge_grid=GRID)
    W_b, st_b = elm.solve(E, D, TRANSIENT, ridge_grid=GRID)
    assert st_a.cpu().tolist() == [0] * G
    assert torch.equal(W_a, W_b) and torch.equal(st_a, st_b)
    for name in ("last_ridge_choice", "last_ridge_lambda", "last_ridge_scores"):
        a, b = vars(esn)[name], vars(elm)[name]
        assert a is not b and torch.equal(a, b), name
    assert tuple(elm.last_ridge_scores.shape) == (G, len(GRID))
    assert all(0 <= c < len(GRID) for c in elm.last_ridge_choice.cpu().tolist())


@pytest.mark.parametrize("cols", COLS)
def test_the_elm_bank_repairs_a_flagged_group_under_its_own_scalings(cols):
    import torch
    from esn_ofdm_mimo_amd.batched import ReservoirBank
    _, elm, E, D, t_scale, t_shift = system(cols)
    W, st = elm.solve(E, D, TRANSIENT, method="chol")
    assert st.cpu().tolist() == [0, 0, 0]
    st[1] = 1                                       # flagged by hand
    before = W.clone()
    assert elm.resolve_failed(E, D, TRANSIENT, W, st) == 1
    alone = ReservoirBank(cols - 2, N_OUT, 2, np.zeros((2, 2)), np.zeros((2, cols - 2)), np.zeros((2, N_OUT)))
    alone.set_scaling(None, None, t_scale[1:2], t_shift[1:2])
    W_1, st_1 = alone.solve(E[1:2].contiguous(), D[1:2].contiguous(), TRANSIENT, method="qr")
    assert st_1.cpu().tolist() == [0] and st.cpu().tolist() == [0, 0, 0]
    assert torch.equal(W[1], W_1[0]) and not torch.equal(W[1], before[1])
    assert torch.equal(W[0], before[0]) and torch.equal(W[2], before[2])
    assert elm.t_scale is t_scale and elm.t_shift is t_shift


def _scalings(n_in):
    import torch
    rs = np.random.RandomState(7)
    return tuple(torch.as_tensor(a, device="cuda") for a in (0.5 + rs.rand(G, n_in), 0.1 * rs.randn(G, n_in),
                                                             0.5 + rs.rand(G, N_OUT), 0.1 * rs.randn(G, N_OUT)))


NAMES = ("in_scale", "in_shift", "t_scale", "t_shift")


def test_the_elm_bank_holds_its_scalings_once():
    import torch
    from esn_ofdm_mimo_amd.elm import ElmBank
    n_in, n_hidden, window = 2, 9, 3
    rs = np.random.RandomState(8)
    W_in, b = 0.3 * rs.randn(n_hidden, window * n_in), rs.rand(n_hidden) - 0.5
    U, D = rs.randn(G, T, n_in), rs.randn(G, T, N_OUT)
    given = _scalings(n_in)
    out = []
    for by_call in (True, False):
        bank = ElmBank(n_in, N_OUT, n_hidden, window, W_in, b, n_groups=G)
        assert all(getattr(bank, name) is None for name in NAMES)
        if by_call:
            bank.set_scaling(*given)
        else:
            bank.in_scale, bank.in_shift, bank.t_scale, bank.t_shift = given
        assert all(getattr(bank, name) is t for name, t in zip(NAMES, given)) and not hasattr(bank, "_ro")
        bank.fit(U, D, method="chol")
        assert bank.fit_status.cpu().tolist() == [0] * G
        out.append((bank.W_out, bank.predict(U, 1, transient=window - 1)))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    plain = ElmBank(n_in, N_OUT, n_hidden, window, W_in, b, n_groups=G)
    plain.fit(U, D, method="chol")
    assert not torch.equal(plain.W_out, out[0][0])                  # (the scalings are read at all)


def test_the_fnn_bank_holds_its_scalings_once():
    import torch
    from esn_ofdm_mimo_amd.fnn import FnnBank
    n_in, n_hidden, window = 2, 8, 3
    rs = np.random.RandomState(9)
    k = window * n_in
    init = (0.3 * rs.randn(n_hidden, k), 0.1 * rs.randn(n_hidden), 0.3 * rs.randn(N_OUT, n_hidden), 0.1 * rs.randn(N_OUT))
    U, D = rs.randn(G, T, n_in), rs.randn(G, T, N_OUT)
    given = _scalings(n_in)
    out = []
    for by_call in (True, False):
        bank = FnnBank(n_in, N_OUT, n_hidden, window, n_groups=G)
        assert all(getattr(bank, name) is None for name in NAMES)
        if by_call:
            bank.set_scaling(*given)
        else:
            bank.in_scale, bank.in_shift, bank.t_scale, bank.t_shift = given
        assert all(getattr(bank, name) is t for name, t in zip(NAMES, given)) and not hasattr(bank, "_ro")
        bank.train(U, D, init, epochs=5)
        out.append((bank.W1, bank.b2, bank.predict(U, 1, transient=window - 1)))
    assert all(torch.equal(a, b) for a, b in zip(*out))
    plain = FnnBank(n_in, N_OUT, n_hidden, window, n_groups=G).train(U, D, init, epochs=5)
    assert not torch.equal(plain.W1, out[0][0])                     # (the scalings are read at all)
