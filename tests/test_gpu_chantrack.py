"""esn_channel_track (csrc/esn_chantrack.hip: the decision-directed channel estimate) on the device, against the NumPy
restatement tests/chantrack_ref.py.

Inputs as tests/test_gpu_remod.py::make_case builds them: X_hat = const[idx] + e for drawn indices, |Re e| and |Im e| at
most a quarter of half the grid spacing, so the restatement alone decides every element as drawn (asserted); the received
frames are those decisions through drawn taps plus a little noise, N ifft sqrt(Pi) with a random cyclic-prefix part that
must not be read.  Pi and reg differ per group.  The generator asserts cond(G + reg) <= 1e4 for every estimate.

Bound per estimate: taps within max(1e-12, 16 n_t isi cond_e 2^-52) of max |taps_ref|; H within isi times that, each
entry being a sum of isi tap errors with unit weights.  Outputs pre-filled with NaN come back finite, status 0; the
X_hat path and the bits path give the same bytes; an estimate alone is bitwise itself inside the batch.  A hand-made
frame whose two antennas carry the same symbols, reg = 0, gives status 1 and NaN for that estimate only, its neighbours
bitwise unchanged; with reg > 0 it solves."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chantrack_ref as cr  # noqa: E402
import remod_ref  # noqa: E402
from oracle.esn_oracle import unit_qam  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
# N, n_t, n_r, isi, m, cp, W, n_est, estimates per group
SHAPES = [
    (16, 1, 1, 2, 2, 0, 1, 1, 1), (16, 2, 2, 4, 2, 3, 1, 3, 3), (32, 2, 3, 8, 4, 7, 2, 67, 3), (32, 4, 8, 4, 6, 7, 3, 3, 1),
    (64, 2, 2, 8, 2, 7, 1, 5, 2), (128, 4, 8, 8, 4, 7, 1, 3, 1), (128, 4, 8, 8, 4, 7, 2, 5, 3), (512, 2, 2, 8, 2, 7, 1, 2, 1),
]
IDS = ["N%d-nt%d-nr%d-L%d-m%d-cp%d-W%d-E%d-G%d" % s for s in SHAPES]
COND_MAX = 1e4


def make_case(shape, seed=0):
    """dict of host arrays: y_cp complex [n_est W, cp + N, n_r], X_hat complex, bits uint8, idx, p_i [G], reg [G, isi]"""
    N, n_t, n_r, L, m, cp, W, n_est, epg = shape
    rs = np.random.RandomState(1000 * N + 100 * n_t + 10 * L + n_est + seed)
    G = (n_est + epg - 1) // epg
    B = n_est * W
    p_i = 1e-5 * 10 ** rs.uniform(0.5, 3.0, size=G)                     # differs per group
    reg = 10 ** rs.uniform(-3.0, -1.0, size=(G, L))
    _, norm = remod_ref.slicer_constants(m)
    idx = rs.randint(0, 1 << m, size=(B, N, n_t))
    q = 0.25 / norm                                                     # a quarter of half the grid spacing 2 / norm
    X = unit_qam(m)[idx]
    X_hat = X + rs.uniform(-q, q, size=idx.shape) + 1j * rs.uniform(-q, q, size=idx.shape)
    taps = (rs.randn(n_est, n_r, n_t, L) + 1j * rs.randn(n_est, n_r, n_t, L)) * np.exp(-np.arange(L) / 3.0)
    Hf = np.transpose(np.fft.fft(taps, N, axis=3), (0, 3, 1, 2))        # [n_est, N, n_r, n_t]
    Yf = np.einsum("bkrt,bkt->bkr", np.repeat(Hf, W, axis=0), X)
    Yf = Yf + 0.03 * (rs.randn(*Yf.shape) + 1j * rs.randn(*Yf.shape))
    p_f = p_i[np.repeat(np.arange(n_est) // epg, W)]
    body = N * np.fft.ifft(Yf, axis=1) * np.sqrt(p_f)[:, None, None]
    prefix = (rs.randn(B, cp, n_r) + 1j * rs.randn(B, cp, n_r)) * np.abs(body).max()
    return dict(y_cp=np.concatenate([prefix, body], axis=1), X_hat=X_hat, bits=remod_ref.index_bits(idx, m), idx=idx,
                p_i=p_i, reg=reg)


def reference(shape, case):
    N, n_t, n_r, L, m, cp, W, n_est, epg = shape
    ref = cr.channel_track(case["y_cp"], W, epg, cp, n_t, L, m, case["p_i"], case["reg"], X_hat=case["X_hat"])
    assert np.array_equal(remod_ref.slice_indices(case["X_hat"], m), case["idx"])       # decided as drawn
    assert ref["status"].tolist() == [0] * n_est
    assert ref["cond"].max() <= COND_MAX, ref["cond"].max()
    return ref


def dev(a, dtype=None):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    return (t if dtype is None else t.to(dtype)).contiguous()


def run(shape, y, p_i, reg, X_hat=None, bits=None, n_est=None, want_taps=True):
    """esn_channel_track through the binding on device tensors: (rc, taps, H, status), outputs pre-filled (NaN, -1)"""
    import torch
    from esn_ofdm_mimo_amd import _lib
    lib = _lib.load()
    N, n_t, n_r, L, m, cp, W, n_all, epg = shape
    n_est = n_all if n_est is None else n_est
    nan = complex(float("nan"), float("nan"))
    taps = torch.full((n_est, n_r, n_t, L), nan, dtype=torch.complex128, device="cuda") if want_taps else None
    H = torch.full((n_est, N, n_r, n_t), nan, dtype=torch.complex128, device="cuda")
    status = torch.full((n_est,), -1, dtype=torch.int32, device="cuda")
    rc = lib.esn_channel_track(_lib.ptr(y), _lib.ptr(X_hat), _lib.ptr(bits), n_est, W, epg, N, cp, n_t, n_r, L, m,
                               _lib.ptr(p_i), _lib.ptr(reg), _lib.ptr(taps), _lib.ptr(H), _lib.ptr(status),
                               _lib.stream_handle())
    torch.cuda.synchronize()
    return rc, taps, H, status


def same_bits(a, b):
    import torch
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    va, vb = torch.view_as_real(a.contiguous()).view(torch.int64), torch.view_as_real(b.contiguous()).view(torch.int64)
    n_diff = int((va != vb).sum())
    assert n_diff == 0, f"{n_diff} of {va.numel()} doubles differ"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_against_the_restatement(shape):
    import torch
    N, n_t, n_r, L, m, cp, W, n_est, epg = shape
    case = make_case(shape)
    ref = reference(shape, case)
    y, xh, bits = dev(case["y_cp"]), dev(case["X_hat"]), dev(case["bits"], torch.uint8)
    p_i, reg = dev(case["p_i"]), dev(case["reg"])
    rc, taps, H, status = run(shape, y, p_i, reg, X_hat=xh)
    assert rc == 0
    assert status.cpu().tolist() == [0] * n_est
    got_t, got_h = taps.cpu().numpy(), H.cpu().numpy()
    assert np.isfinite(got_t.view(np.float64)).all() and np.isfinite(got_h.view(np.float64)).all()   # all written
    for e in range(n_est):
        bound = max(1e-12, 16 * n_t * L * ref["cond"][e] * EPS)
        top = np.abs(ref["taps"][e]).max()
        dt, dh = np.abs(got_t[e] - ref["taps"][e]).max() / top, np.abs(got_h[e] - ref["H"][e]).max() / top
        if e in (0, n_est - 1):
            print(f"{shape} estimate {e}: cond {ref['cond'][e]:.3g}, |taps - ref| / max {dt:.2e}, |H - ref| / max "
                  f"{dh:.2e}, bound {bound:.2e} (H: x {L})")
        assert dt <= bound, (e, dt, bound)
        assert dh <= L * bound, (e, dh, L * bound)
    # the bits path: the same decisions, the same bytes; taps are optional
    rc, taps_b, H_b, status_b = run(shape, y, p_i, reg, bits=bits)
    assert rc == 0 and torch.equal(status_b, status)
    same_bits(taps_b, taps)
    same_bits(H_b, H)
    rc, none, H_n, _ = run(shape, y, p_i, reg, X_hat=xh, want_taps=False)
    assert rc == 0 and none is None
    same_bits(H_n, H)
    # an estimate alone == itself inside the batch
    for e in sorted({0, n_est // 2, n_est - 1}):
        g = e // epg
        rc, t1, H1, s1 = run(shape, y[e * W:(e + 1) * W].contiguous(), p_i[g:g + 1].contiguous(), reg[g:g + 1].contiguous(),
                             X_hat=xh[e * W:(e + 1) * W].contiguous(), n_est=1)
        assert rc == 0 and int(s1[0]) == 0
        same_bits(t1[0], taps[e])
        same_bits(H1[0], H[e])


def test_a_singular_estimate_is_flagged_alone():
    import torch
    shape = (32, 2, 3, 8, 4, 7, 2, 5, 2)
    N, n_t, n_r, L, m, cp, W, n_est, epg = shape
    case = make_case(shape, seed=1)
    bad = 2
    idx = case["idx"].copy()
    idx[bad * W:(bad + 1) * W, :, 1] = idx[bad * W:(bad + 1) * W, :, 0]          # both antennas: the same symbols
    bits_h = remod_ref.index_bits(idx, m)
    y, bits, p_i = dev(case["y_cp"]), dev(bits_h, torch.uint8), dev(case["p_i"])
    zero = dev(np.zeros_like(case["reg"]))
    ref = cr.channel_track(case["y_cp"], W, epg, cp, n_t, L, m, case["p_i"], np.zeros_like(case["reg"]), bits=bits_h)
    assert ref["status"].tolist() == [0, 0, 1, 0, 0]
    rc, taps, H, status = run(shape, y, p_i, zero, bits=bits)
    assert rc == 0 and status.cpu().tolist() == [0, 0, 1, 0, 0]
    assert bool(torch.isnan(torch.view_as_real(taps[bad])).all()) and bool(torch.isnan(torch.view_as_real(H[bad])).all())
    rc, taps0, H0, status0 = run(shape, y, p_i, zero, bits=dev(case["bits"], torch.uint8))   # the frames as drawn
    assert rc == 0 and status0.cpu().tolist() == [0] * n_est
    for e in (0, 1, 3, 4):
        same_bits(taps[e], taps0[e])
        same_bits(H[e], H0[e])
        assert bool(torch.isfinite(torch.view_as_real(H[e])).all())
    # a prior makes it solvable
    rc, taps1, H1, status1 = run(shape, y, p_i, dev(case["reg"]), bits=bits)
    assert rc == 0 and status1.cpu().tolist() == [0] * n_est
    ref1 = cr.channel_track(case["y_cp"], W, epg, cp, n_t, L, m, case["p_i"], case["reg"], bits=bits_h)
    top = np.abs(ref1["taps"][bad]).max()
    bound = max(1e-12, 16 * n_t * L * ref1["cond"][bad] * EPS)
    assert np.abs(taps1[bad].cpu().numpy() - ref1["taps"][bad]).max() <= bound * top, (ref1["cond"][bad], bound)


def test_through_the_frame_source():
    """FrameSource.track_channel: reg is the MAP weight of the pilot estimator's prior, the outputs those of the entry
    point; argument errors are ValueErrors"""
    import dataclasses
    import torch
    from esn_ofdm_mimo_amd.montecarlo import FrameSource, LinkParams
    p = dataclasses.replace(LinkParams.block_fading(2, 2, n_sub=32), m=2)
    src = FrameSource(p, seed=3)
    shape = (p.n_sub, p.n_t, p.n_r, p.isi, p.m, p.cp, 2, 4, 1)
    case = make_case(shape)
    ebno = 18.0
    regs = cr.map_reg(p.n_sub, p.cp, p.isi, p.no, p.p_i(ebno))
    np.testing.assert_allclose(src.track_prior(ebno), regs, rtol=1e-14)
    ref = cr.channel_track(case["y_cp"], 2, 1, p.cp, p.n_t, p.isi, p.m, np.full(4, p.p_i(ebno)), np.tile(regs, (4, 1)),
                           X_hat=case["X_hat"])
    y, xh, bits = dev(case["y_cp"]), dev(case["X_hat"]), dev(case["bits"], torch.uint8)
    H, status, taps = src.track_channel(y, ebno, X_hat=xh, window=2, want_taps=True)
    assert status.cpu().tolist() == [0] * 4 and status.dtype == torch.int32
    top = np.abs(ref["taps"]).max()
    bound = max(1e-12, 16 * p.n_t * p.isi * ref["cond"].max() * EPS)
    assert np.abs(taps.cpu().numpy() - ref["taps"]).max() <= bound * top
    assert np.abs(H.cpu().numpy() - ref["H"]).max() <= p.isi * bound * top
    H2, status2 = src.track_channel(y, ebno, bits=bits, window=2)
    same_bits(H2, H)
    for kw in (dict(), dict(X_hat=xh, bits=bits), dict(X_hat=xh, window=0), dict(X_hat=xh, window=9), dict(X_hat=xh, window=3)):
        with pytest.raises(ValueError):
            src.track_channel(y, ebno, **kw)
