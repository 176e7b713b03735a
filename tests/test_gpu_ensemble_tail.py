"""esn_detect_count_ens[_f32] on the device: the combination of K slabs is the ordered, individually rounded weighted
sum NumPy float64 computes (tests/ensemble_ref.combine), and what follows is the tail of esn_detect_count with the same
butterflies on the same operands -- so every comparison here is bitwise: counters equal, X_hat equal as bytes."""
import numpy as np
import pytest

import ensemble_ref as er

pytestmark = pytest.mark.gpu

# (N, n_t, m, frames, frames per group): a ragged last group and no multiple of 8 frames at the fixed-shape tail's
# shape; a small one; one antenna, 64-QAM, a group per frame; antenna chunks (5 antennas of 2048 points do not fit LDS)
SHAPES = {"n128": (128, 4, 4, 19, 5), "n64": (64, 2, 2, 7, 3), "n16": (16, 1, 6, 5, 1), "chunks": (2048, 5, 2, 2, 1)}


@pytest.fixture(scope="module")
def dev():
    import torch
    from esn_ofdm_mimo_amd import _lib
    return torch, _lib.load(), _lib


def _case(shape, K, seed=0):
    N, n_t, m, B, F = SHAPES[shape]
    rs = np.random.RandomState(seed)
    G = (B + F - 1) // F
    p_i = rs.uniform(0.5, 2.0, G)
    # outputs around constellation points of power p_i, N-fold (the tail divides by N sqrt(p_i)): errors, not all
    Y = rs.randn(K, B, N, 2 * n_t) * 0.25 * np.sqrt(N)
    tx = rs.randint(0, 2, (B, N * m, n_t)).astype(np.uint8)
    return N, n_t, m, B, F, G, p_i, Y, tx


def _weights(G, K, seed=1):
    w = np.random.RandomState(seed).uniform(0.1, 1.0, (G, K))
    w[0, 0] = 0.0
    w[-1, K - 1] = -0.7
    return w


def _single(dev, Y, p_i, tx, F, N, n_t, m, want_xhat=True):
    """esn_detect_count / _f32 on Y [B, N, 2 n_t] (NumPy): (err, bits, X_hat) as NumPy."""
    torch, lib, _lib = dev
    f32 = Y.dtype == np.float32
    y = torch.as_tensor(np.ascontiguousarray(Y), device="cuda")
    B = y.shape[0]
    G = (B + F - 1) // F
    err = torch.zeros(G, dtype=torch.int64, device="cuda")
    nb = torch.zeros(G, dtype=torch.int64, device="cuda")
    xh = torch.empty((B, N, 2 * n_t), dtype=torch.float64, device="cuda")
    pt = torch.as_tensor(p_i, device="cuda")
    tt = torch.as_tensor(tx, device="cuda")
    fn = lib.esn_detect_count_f32 if f32 else lib.esn_detect_count
    _lib.check(fn(y.data_ptr(), B, F, N, n_t, m, pt.data_ptr(), tt.data_ptr(), err.data_ptr(), nb.data_ptr(),
                  xh.data_ptr(), _lib.stream_handle()), "esn_detect_count")
    return err.cpu().numpy(), nb.cpu().numpy(), xh.cpu().numpy()


def _ens(dev, Y, p_i, tx, F, N, n_t, m, weights=None, members=False, err0=None, bits0=None, y_dev=None):
    """esn_detect_count_ens / _f32 on Y [K, B, N, 2 n_t]: (err, bits, X_hat, member_err or None) as NumPy."""
    torch, lib, _lib = dev
    f32 = Y.dtype == np.float32
    y = torch.as_tensor(np.ascontiguousarray(Y), device="cuda") if y_dev is None else y_dev
    K, B = y.shape[:2]
    G = (B + F - 1) // F
    err = torch.zeros(G, dtype=torch.int64, device="cuda") if err0 is None else torch.as_tensor(err0, device="cuda")
    nb = torch.zeros(G, dtype=torch.int64, device="cuda") if bits0 is None else torch.as_tensor(bits0, device="cuda")
    me = torch.zeros((G, K), dtype=torch.int64, device="cuda") if members else None
    xh = torch.empty((B, N, 2 * n_t), dtype=torch.float64, device="cuda")
    pt = torch.as_tensor(p_i, device="cuda")
    tt = torch.as_tensor(tx, device="cuda")
    wt = None if weights is None else torch.as_tensor(np.ascontiguousarray(weights), device="cuda")
    fn = lib.esn_detect_count_ens_f32 if f32 else lib.esn_detect_count_ens
    _lib.check(fn(y.data_ptr(), K, B, F, N, n_t, m, pt.data_ptr(), None if wt is None else wt.data_ptr(), tt.data_ptr(),
                  err.data_ptr(), nb.data_ptr(), None if me is None else me.data_ptr(), xh.data_ptr(),
                  _lib.stream_handle()), "esn_detect_count_ens")
    return err.cpu().numpy(), nb.cpu().numpy(), xh.cpu().numpy(), None if me is None else me.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", ["n128", "n64", "n16"])
def test_one_member_is_the_single_tail_bitwise(dev, shape, dtype):
    N, n_t, m, B, F, G, p_i, Y, tx = _case(shape, 1)
    Y = Y.astype(dtype)
    e0, b0, x0 = _single(dev, Y[0], p_i, tx, F, N, n_t, m)
    e1, b1, x1, _ = _ens(dev, Y, p_i, tx, F, N, n_t, m)
    assert 0 < e0.sum() < b0.sum()
    assert np.array_equal(e0, e1) and np.array_equal(b0, b1)
    assert _same_bits(x0, x1)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("K", [3, 4, 16])
@pytest.mark.parametrize("shape", ["n128", "n64", "n16", "chunks"])
def test_members_are_summed_in_order_and_rounded_one_by_one(dev, shape, K, dtype, weighted):
    """Against esn_detect_count on the NumPy-summed Y.  Without weights 1/3 is inexact, which is the point; the weight
    table holds a zero and a negative entry."""
    N, n_t, m, B, F, G, p_i, Y, tx = _case(shape, K, seed=K)
    Y = Y.astype(dtype)
    w = _weights(G, K) if weighted else None
    e0, b0, x0 = _single(dev, er.combine(Y, w, F), p_i, tx, F, N, n_t, m)
    e1, b1, x1, _ = _ens(dev, Y, p_i, tx, F, N, n_t, m, weights=w)
    assert np.array_equal(e0, e1) and np.array_equal(b0, b1)
    assert _same_bits(x0, x1)
    assert np.array_equal(b1, np.minimum(F, B - F * np.arange(G)) * N * m * n_t)


def test_float_members_off_16_byte_alignment(dev):
    """A float Y that is 8-byte but not 16-byte aligned takes the element-wise loads: same bits."""
    torch = dev[0]
    N, n_t, m, B, F, G, p_i, Y, tx = _case("n64", 3, seed=9)
    Y = Y.astype(np.float32)
    buf = torch.empty(Y.size + 2, dtype=torch.float32, device="cuda")
    y_dev = buf[2:].view(Y.shape)
    y_dev.copy_(torch.as_tensor(Y))
    assert y_dev.data_ptr() % 16 == 8
    e0, b0, x0 = _single(dev, er.combine(Y, None, F), p_i, tx, F, N, n_t, m)
    e1, b1, x1, _ = _ens(dev, Y, p_i, tx, F, N, n_t, m, y_dev=y_dev)
    assert np.array_equal(e0, e1) and np.array_equal(b0, b1) and _same_bits(x0, x1)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape,K", [("n128", 4), ("n16", 3), ("chunks", 2)])
def test_member_counts_are_those_of_k_single_runs(dev, shape, K, dtype):
    N, n_t, m, B, F, G, p_i, Y, tx = _case(shape, K, seed=20 + K)
    Y = Y.astype(dtype)
    w = _weights(G, K, seed=3)
    e0, b0, x0, none = _ens(dev, Y, p_i, tx, F, N, n_t, m, weights=w)
    e1, b1, x1, me = _ens(dev, Y, p_i, tx, F, N, n_t, m, weights=w, members=True)
    assert none is None
    # the ensemble's own outputs do not move when the members are asked for
    assert np.array_equal(e0, e1) and np.array_equal(b0, b1) and _same_bits(x0, x1)
    for k in range(K):
        ek, _, _ = _single(dev, Y[k], p_i, tx, F, N, n_t, m)
        assert np.array_equal(me[:, k], ek), k
    assert len({tuple(me[:, k]) for k in range(K)}) > 1


def test_counters_accumulate(dev):
    N, n_t, m, B, F, G, p_i, Y, tx = _case("n64", 3, seed=5)
    e0, b0, _, m0 = _ens(dev, Y, p_i, tx, F, N, n_t, m, members=True)
    err0 = np.arange(G, dtype=np.int64) * 1000 + 7
    bits0 = np.arange(G, dtype=np.int64) * 5 + 11
    e1, b1, _, _ = _ens(dev, Y, p_i, tx, F, N, n_t, m, err0=err0, bits0=bits0)
    assert np.array_equal(e1, e0 + err0) and np.array_equal(b1, b0 + bits0)
    # member counters accumulate too: two launches into one table
    torch, lib, _lib = dev
    y = torch.as_tensor(Y, device="cuda")
    me = torch.as_tensor(m0.copy(), device="cuda")
    err = torch.zeros(G, dtype=torch.int64, device="cuda")
    nb = torch.zeros(G, dtype=torch.int64, device="cuda")
    pt, tt = torch.as_tensor(p_i, device="cuda"), torch.as_tensor(tx, device="cuda")
    _lib.check(lib.esn_detect_count_ens(y.data_ptr(), 3, B, F, N, n_t, m, pt.data_ptr(), None, tt.data_ptr(),
                                        err.data_ptr(), nb.data_ptr(), me.data_ptr(), None, _lib.stream_handle()), "ens")
    assert np.array_equal(me.cpu().numpy(), 2 * m0)
    assert np.array_equal(err.cpu().numpy(), e0) and np.array_equal(nb.cpu().numpy(), b0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_frame_alone_gives_the_bits_it_gives_in_the_batch(dev, dtype):
    N, n_t, m, B, F, G, p_i, Y, tx = _case("n128", 4, seed=31)
    Y = Y.astype(dtype)
    w = _weights(G, 4, seed=8)
    per_frame_pi, per_frame_w = np.repeat(p_i, F)[:B], np.repeat(w, F, axis=0)[:B]
    e, b, xh, me = _ens(dev, Y, per_frame_pi, tx, 1, N, n_t, m, weights=per_frame_w, members=True)
    for f in (0, 7, B - 1):
        e1, b1, x1, m1 = _ens(dev, Y[:, f:f + 1], per_frame_pi[f:f + 1], tx[f:f + 1], 1, N, n_t, m,
                              weights=per_frame_w[f:f + 1], members=True)
        assert e1[0] == e[f] and b1[0] == b[f] and _same_bits(x1[0], xh[f]) and np.array_equal(m1[0], me[f])
    # and in groups of F the same frames add up to the same counts
    eg, bg, xg, _ = _ens(dev, Y, p_i, tx, F, N, n_t, m, weights=w)
    assert np.array_equal(eg, np.add.reduceat(e, np.arange(0, B, F))) and _same_bits(xg, xh)
