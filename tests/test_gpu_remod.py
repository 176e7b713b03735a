"""esn_detect_remod (csrc/esn_remod.hip: detect, decide and re-modulate in one launch) on the device, against the NumPy
restatement tests/remod_ref.py and against esn_detect_count.

Inputs with unambiguous decisions: X = const[idx] + e for drawn indices, |Re e| and |Im e| at most a quarter of half the
grid spacing, Y = N ifft(X) sqrt(Pi) -- the restatement alone decides every element as drawn (asserted on the CPU side)
-- with errors planted in tx_bits.  Shapes: every axis the indexing depends on, in mixed company -- N in {16, 32, 128}
(even and odd stage counts, and the fixed-shape tail's N), n_t in {1, 2, 4, 5}, m in {2, 4, 6}, (cp, delay) in
{(0, 0), (7, 3), (7, 0)}, B in {1, 3, 67} in groups of 1 and 3 (ragged last group), Pi differing per group; and one
shape whose antennas do not fit LDS together (N = 1024, n_t = 9: workgroups of 8 and 1 antennas per frame).

  * D_hat, pre-filled with NaN, comes back finite everywhere and within 1e-12 of max |D_hat| of the restatement (the
    bound generated frames and the tail's X_hat are held to); decided bits exact;
  * counters and the bytes of X_hat are those of esn_detect_count on the same Y (at N = 128, n_t = 4, m = 4 that call
    runs the fixed-shape kernel); counters accumulate over two calls; tx_bits NULL counts nothing;
  * a frame alone equals itself inside a batch, bitwise;
  * fixed point: the body rows of D_hat fed back as Y decide the same bits -- zero errors against dec_bits;
  * rejected shapes return -1 with a message and leave the outputs untouched."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import remod_ref  # noqa: E402
from oracle.esn_oracle import unit_qam  # noqa: E402

pytestmark = pytest.mark.gpu

# N, n_t, m, cp, delay, B, frames per group
SHAPES = [
    (16, 1, 2, 0, 0, 1, 1), (16, 2, 4, 7, 3, 3, 3), (16, 5, 6, 7, 0, 67, 3), (16, 4, 4, 7, 3, 3, 1),
    (32, 1, 4, 7, 0, 67, 1), (32, 4, 6, 0, 0, 3, 3), (32, 2, 2, 7, 3, 1, 3), (32, 5, 4, 7, 3, 67, 3),
    (128, 4, 4, 7, 3, 67, 3), (128, 2, 2, 7, 0, 3, 1), (128, 5, 6, 0, 0, 1, 1), (128, 1, 2, 7, 3, 3, 3),
    (1024, 9, 2, 7, 3, 2, 1),      # LDS holds 8 antennas of N = 1024: two workgroups per frame, the second with one antenna
]
IDS = ["N%d-nt%d-m%d-cp%d-d%d-B%d-F%d" % s for s in SHAPES]


def make_case(shape, seed=0):
    """Y float64 [B, N, 2 n_t], p_i [G], idx [B, N, n_t] as drawn, tx_bits uint8 [B, N m, n_t] with planted errors and
    their count per group"""
    N, n_t, m, cp, delay, B, F = shape
    rs = np.random.RandomState(1000 * N + 100 * n_t + 10 * m + B + seed)
    G = (B + F - 1) // F
    p_i = 1e-5 * 10 ** rs.uniform(0.5, 3.0, size=G)                     # differs per group
    _, norm = remod_ref.slicer_constants(m)
    idx = rs.randint(0, 1 << m, size=(B, N, n_t))
    q = 0.25 / norm                                                     # a quarter of half the grid spacing 2 / norm
    X = unit_qam(m)[idx] + rs.uniform(-q, q, size=idx.shape) + 1j * rs.uniform(-q, q, size=idx.shape)
    y = N * np.fft.ifft(X, axis=1) * np.sqrt(p_i[np.arange(B) // F])[:, None, None]
    Y = np.zeros((B, N, 2 * n_t))
    Y[..., 0::2], Y[..., 1::2] = y.real, y.imag
    tx = remod_ref.index_bits(idx, m)
    flip = rs.rand(*tx.shape) < 0.05
    flip[0, 0, 0] = True                                                # (at least one error in group 0)
    planted = np.bincount(np.arange(B) // F, weights=flip.reshape(B, -1).sum(axis=1), minlength=G).astype(np.int64)
    return Y, p_i, idx, tx ^ flip.astype(np.uint8), planted


def dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda").to(dtype or torch.float64).contiguous()


def run(shape, Y, p_i, tx, err=None, nb=None, want_xhat=True, want_bits=True):
    """esn_detect_remod through the binding: (rc, D_hat, err, nb, X_hat, dec_bits) as device tensors; D_hat, X_hat and
    dec_bits are pre-filled (NaN, NaN, 255)"""
    import torch
    from esn_ofdm_mimo_amd import _lib
    lib = _lib.load()
    N, n_t, m, cp, delay, _, F = shape
    B = Y.shape[0]
    G = (B + F - 1) // F
    if tx is not None:
        err = torch.zeros(G, dtype=torch.int64, device="cuda") if err is None else err
        nb = torch.zeros(G, dtype=torch.int64, device="cuda") if nb is None else nb
    D = torch.full((B, max(delay + cp + N, 1), 2 * n_t), float("nan"), dtype=torch.float64, device="cuda")
    xh = torch.full((B, N, 2 * n_t), float("nan"), dtype=torch.float64, device="cuda") if want_xhat else None
    db = torch.full((B, N * m, n_t), 255, dtype=torch.uint8, device="cuda") if want_bits else None
    rc = lib.esn_detect_remod(_lib.ptr(Y), B, F, N, cp, delay, n_t, m, _lib.ptr(p_i), _lib.ptr(tx), _lib.ptr(err),
                              _lib.ptr(nb), _lib.ptr(xh), _lib.ptr(db), _lib.ptr(D), _lib.stream_handle())
    torch.cuda.synchronize()
    return rc, D, err, nb, xh, db


def count(shape, Y, p_i, tx):
    """esn_detect_count on the same Y: (err, bits, X_hat)"""
    import torch
    from esn_ofdm_mimo_amd import _lib
    lib = _lib.load()
    N, n_t, m, _, _, _, F = shape
    B = Y.shape[0]
    G = (B + F - 1) // F
    err = torch.zeros(G, dtype=torch.int64, device="cuda")
    nb = torch.zeros(G, dtype=torch.int64, device="cuda")
    xh = torch.empty((B, N, 2 * n_t), dtype=torch.float64, device="cuda")
    _lib.check(lib.esn_detect_count(_lib.ptr(Y), B, F, N, n_t, m, _lib.ptr(p_i), _lib.ptr(tx), _lib.ptr(err), _lib.ptr(nb),
                                    _lib.ptr(xh), _lib.stream_handle()), "esn_detect_count")
    return err, nb, xh


def same_bits(a, b):
    import torch
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    n_diff = int((a.contiguous().view(torch.int64) != b.contiguous().view(torch.int64)).sum())
    assert n_diff == 0, f"{n_diff} of {a.numel()} elements differ"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_against_the_restatement_and_the_counting_tail(shape):
    import torch
    N, n_t, m, cp, delay, B, F = shape
    Yh, ph, idx, txh, planted = make_case(shape)
    ref = remod_ref.detect_remod(Yh, F, N, cp, delay, n_t, m, ph, tx_bits=txh)
    assert np.array_equal(ref["idx"], idx)                              # the restatement alone decides as drawn
    assert np.array_equal(ref["err"], planted) and int(planted[0]) > 0
    Y, p_i, tx = dev(Yh), dev(ph), dev(txh, torch.uint8)
    rc, D, err, nb, xh, db = run(shape, Y, p_i, tx)
    assert rc == 0
    got = D.cpu().numpy()
    assert got.shape == ref["D_hat"].shape and np.isfinite(got).all()   # every element was written
    worst, top = np.abs(got - ref["D_hat"]).max(), np.abs(ref["D_hat"]).max()
    print(f"{shape}: max |D_hat - ref| = {worst:.3e} of {top:.3e} ({worst / top:.2e})")
    assert worst <= 1e-12 * top
    if delay:
        assert not got[:, :delay].any()
    assert np.array_equal(db.cpu().numpy(), ref["dec_bits"])
    assert err.cpu().numpy().tolist() == ref["err"].tolist() and nb.cpu().numpy().tolist() == ref["bits"].tolist()
    # bitwise the counting tail (fixed-shape kernel at N = 128, n_t = 4, m = 4)
    e0, n0, x0 = count(shape, Y, p_i, tx)
    assert torch.equal(err, e0) and torch.equal(nb, n0)
    same_bits(xh, x0)
    # counters accumulate over a second call; the other outputs are the same bytes
    rc, D2, err2, nb2, _, _ = run(shape, Y, p_i, tx, err=err.clone(), nb=nb.clone(), want_xhat=False, want_bits=False)
    assert rc == 0 and torch.equal(err2, 2 * e0) and torch.equal(nb2, 2 * n0)
    same_bits(D2, D)
    # tx_bits NULL: nothing is counted, the counters handed in are not touched
    keep_e, keep_n = torch.full_like(e0, 77), torch.full_like(n0, -5)
    rc, D3, _, _, xh3, db3 = run(shape, Y, p_i, None, err=keep_e, nb=keep_n)
    assert rc == 0 and bool((keep_e == 77).all()) and bool((keep_n == -5).all())
    same_bits(D3, D)
    same_bits(xh3, xh)
    assert torch.equal(db3, db)
    # a frame alone == itself inside the batch
    for f in sorted({0, B // 2, B - 1}):
        one = (N, n_t, m, cp, delay, 1, 1)
        rc, D1, e1, n1, xh1, db1 = run(one, Y[f:f + 1].contiguous(), p_i[f // F:f // F + 1].contiguous(),
                                       tx[f:f + 1].contiguous())
        assert rc == 0
        same_bits(D1[0], D[f])
        same_bits(xh1[0], xh[f])
        assert torch.equal(db1[0], db[f]) and int(n1[0]) == N * m * n_t
    # fixed point: the body of D_hat is a frame whose decisions are dec_bits
    body = D[:, delay + cp:].contiguous()
    assert body.shape == Y.shape
    rc, D4, e4, n4, _, db4 = run(shape, body, p_i, db)
    assert rc == 0 and int(e4.sum()) == 0 and torch.equal(n4, n0) and torch.equal(db4, db)
    assert float((D4 - D).abs().max()) <= 1e-12 * top


def test_rejected_shapes_leave_the_outputs_untouched():
    import torch
    from esn_ofdm_mimo_amd import _lib
    lib = _lib.load()
    good = (16, 2, 4, 7, 3, 3, 3)
    Yh, ph, _, txh, _ = make_case(good)
    Y, p_i, tx = dev(Yh), dev(ph), dev(txh, torch.uint8)
    # (N, n_t, m, cp, delay, B, F) the entry point must refuse, and a word of its message; buffers keep the good size
    for bad, word in (((24, 2, 4, 7, 3, 2, 3), b"power of two"), ((16, 17, 4, 7, 3, 1, 3), b"16"),
                      ((16, 2, 3, 7, 3, 3, 3), b"even"), ((16, 2, 4, 16, 3, 3, 3), b"[0, N)"),
                      ((16, 2, 4, -1, 3, 3, 3), b"[0, N)"), ((16, 2, 4, 7, -1, 3, 3), b"delay"),
                      ((16, 2, 4, 7, 3, 3, 0), b"invalid sizes")):
        N, n_t, m, cp, delay, B, F = bad
        err = torch.full((1,), 11, dtype=torch.int64, device="cuda")
        nb = torch.full((1,), 13, dtype=torch.int64, device="cuda")
        D = torch.full((3, 26, 4), float("nan"), dtype=torch.float64, device="cuda")
        xh = torch.full((3, 16, 4), float("nan"), dtype=torch.float64, device="cuda")
        db = torch.full((3, 64, 2), 255, dtype=torch.uint8, device="cuda")
        rc = lib.esn_detect_remod(_lib.ptr(Y), B, F, N, cp, delay, n_t, m, _lib.ptr(p_i), _lib.ptr(tx), _lib.ptr(err),
                                  _lib.ptr(nb), _lib.ptr(xh), _lib.ptr(db), _lib.ptr(D), _lib.stream_handle())
        msg = lib.esn_last_error()
        torch.cuda.synchronize()
        assert rc == -1 and b"esn_detect_remod" in msg and word in msg, (bad, rc, msg)
        assert int(err[0]) == 11 and int(nb[0]) == 13
        assert bool(torch.isnan(D).all()) and bool(torch.isnan(xh).all()) and bool((db == 255).all())


def test_through_the_bank():
    """ReservoirBank.detect_remod: the same outputs, optional ones on request, float32 Y refused"""
    import torch
    from esn_ofdm_mimo_amd.batched import ReservoirBank
    shape = (32, 2, 4, 7, 3, 5, 3)
    N, n_t, m, cp, delay, B, F = shape
    Yh, ph, idx, txh, planted = make_case(shape)
    ref = remod_ref.detect_remod(Yh, F, N, cp, delay, n_t, m, ph, tx_bits=txh)
    bank = ReservoirBank(2, 2 * n_t, 4, np.zeros((4, 4)), np.zeros((4, 2)), np.zeros((4, 2 * n_t)), noise=0.0)
    D, err, nb, xh, db = bank.detect_remod(Yh, txh, ph, F, N, cp, delay, n_t, m, want_xhat=True, want_bits=True)
    assert err.cpu().numpy().tolist() == planted.tolist() and nb.cpu().numpy().tolist() == ref["bits"].tolist()
    assert np.array_equal(db.cpu().numpy(), ref["dec_bits"])
    assert np.abs(D.cpu().numpy() - ref["D_hat"]).max() <= 1e-12 * np.abs(ref["D_hat"]).max()
    x = xh.cpu().numpy().reshape(B, N, n_t, 2)
    assert np.abs(x[..., 0] + 1j * x[..., 1] - ref["X_hat"]).max() <= 1e-12 * np.abs(ref["X_hat"]).max()
    D2, e2, n2 = bank.detect_remod(Yh, None, ph, F, N, cp, delay, n_t, m)
    assert e2 is None and n2 is None and torch.equal(D2, D)
    # counters handed in are added to
    D3, e3, n3 = bank.detect_remod(Yh, txh, ph, F, N, cp, delay, n_t, m, err=err, bits=nb)
    assert e3 is err and err.cpu().numpy().tolist() == (2 * planted).tolist()
    with pytest.raises(ValueError, match="float64"):
        bank.detect_remod(Yh.astype(np.float32), txh, ph, F, N, cp, delay, n_t, m)
