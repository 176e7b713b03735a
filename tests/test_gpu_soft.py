"""The SINR-weighted soft outputs on the device: esn_mmse_sinr and esn_qam_llr_weighted against their NumPy restatement
(tests/soft_ref.py), the fused soft tail esn_detect_llr[_f32] bit for bit against esn_detect_count[_f32] followed by
esn_qam_llr_weighted, and montecarlo.coded_equalized_point against coded_ber_point (its MMSE leg) and against the NumPy
chain behind the equaliser (its ESN leg).  Seven frames in groups of three, so the last group is ragged, and a Pi of its
own for every group."""
import numpy as np
import pytest

import equalize_ref as qr
import soft_ref as sr
from oracle import esn_oracle as eo

pytestmark = pytest.mark.gpu

NO = 1e-5
B, FPG = 7, 3
P_I = np.array([3e-4, 6e-4, 1.5e-4])
SHAPES = [(16, 1, 1, 2), (32, 2, 2, 4), (64, 3, 5, 6), (128, 4, 8, 4)]      # (N, n_t, n_r, m)
_cases = {}


def _tail():
    from esn_ofdm_mimo_amd.bankbase import DetectorTail, DeviceBank

    class Tail(DeviceBank, DetectorTail):
        pass
    return Tail()


def _frames(rs, n_frames, N, n_t, m, p_i_of_frame, gain=1.0, sigma=0.25):
    """Y [n_frames, N, 2 n_t] whose spectrum over N sqrt(Pi) is `gain` (the equaliser's bias, [n_frames, N, n_t]) times a
    constellation point plus noise -- what an MMSE equaliser hands on: in a deep fade it shrinks symbol and noise alike
    -- and the bits of the points in the TxBits layout [n_frames, N m, n_t], one in twenty flipped so that every shape
    has errors to count."""
    idx = rs.randint(0, 2 ** m, size=(n_frames, N, n_t))
    X = gain * (eo.unit_qam(m)[idx] + sigma * (rs.randn(n_frames, N, n_t) + 1j * rs.randn(n_frames, N, n_t)) / np.sqrt(2.0))
    y = N * np.fft.ifft(X, axis=1) * np.sqrt(p_i_of_frame)[:, None, None]
    Y = np.empty((n_frames, N, 2 * n_t))
    Y[:, :, 0::2], Y[:, :, 1::2] = y.real, y.imag
    bits = eo.bit_labels_lsb_first(m)[idx] ^ (rs.rand(n_frames, N, n_t, m) < 0.05)   # [n_frames, N, n_t, m]
    return Y, np.ascontiguousarray(bits.transpose(0, 1, 3, 2).reshape(n_frames, N * m, n_t)).astype(np.uint8)


def _case(shape):
    """One shape's channel, weights, frames and the unfused outputs, made once: H with a deep fade in the last group,
    w / mu from esn_mmse_sinr, X_hat and counters from esn_detect_count, the restatement's weights and LLRs."""
    if shape in _cases:
        return _cases[shape]
    import torch
    from esn_ofdm_mimo_amd import _lib
    N, n_t, n_r, m = shape
    tail = _tail()
    dev = lambda a, dt=None: torch.as_tensor(np.ascontiguousarray(a), device=tail.device, dtype=dt)
    rs = np.random.RandomState(N + n_r)
    G = (B + FPG - 1) // FPG
    H = (rs.randn(G, N, n_r, n_t) + 1j * rs.randn(G, N, n_r, n_t)) / np.sqrt(2.0)
    H[G - 1, 1] *= 1e-9
    ref = sr.sinr_weights(H, P_I, NO)
    Y, bits = _frames(rs, B, N, n_t, m, P_I[np.arange(B) // FPG], gain=ref[1][np.arange(B) // FPG])
    c = dict(tail=tail, dev=dev, H=H, Y=dev(Y), bits=dev(bits), p_i=dev(P_I), G=G)
    w, mu = (torch.full((G, N, n_t), float("nan"), dtype=torch.float64, device=tail.device) for _ in range(2))
    mean = torch.full((G,), float("nan"), dtype=torch.float64, device=tail.device)
    _lib.check(tail.lib.esn_mmse_sinr(G, N, n_t, n_r, _lib.ptr(c["p_i"]), NO, _lib.ptr(dev(H)), _lib.ptr(w), _lib.ptr(mu),
                                      _lib.ptr(mean), _lib.stream_handle()), "esn_mmse_sinr")
    c.update(w=w, mu=mu, mean=mean, ref=ref)
    c["err"], c["nb"], c["xh"] = tail.detect_count(c["Y"], c["bits"], c["p_i"], FPG, N, n_t, m, want_xhat=True)
    _cases[shape] = c
    return c


def _weighted(c, shape, xh, w, mu, fpg, n_frames=None):
    """esn_qam_llr_weighted on caller-owned outputs pre-filled with NaN."""
    import torch
    from esn_ofdm_mimo_amd import _lib
    N, n_t, n_r, m = shape
    b = xh.shape[0] if n_frames is None else n_frames
    llr = torch.full((b, n_t, N * m), float("nan"), dtype=torch.float64, device=xh.device)
    s2 = torch.full((b,), float("nan"), dtype=torch.float64, device=xh.device)
    _lib.check(c["tail"].lib.esn_qam_llr_weighted(b, fpg, N, n_t, m, _lib.ptr(xh), _lib.ptr(w), _lib.ptr(mu), _lib.ptr(llr),
                                                  _lib.ptr(s2), _lib.stream_handle()), "esn_qam_llr_weighted")
    return llr, s2


@pytest.mark.parametrize("shape", SHAPES)
def test_mmse_sinr_against_the_restatement(shape):
    """Relative 1e-9 per entry, the bound esn_mmse_detect_count's solve is held to; the deep fade sits at the clamp on
    both sides."""
    c = _case(shape)
    w_ref, mu_ref, mean_ref = c["ref"]
    w, mu, mean = (c[k].cpu().numpy() for k in ("w", "mu", "mean"))
    errs = [float(np.max(np.abs(a - b) / np.abs(b))) for a, b in ((w, w_ref), (mu, mu_ref), (mean, mean_ref))]
    print(shape, "relative error of w, mu, gamma_mean", errs)
    assert np.isfinite(w).all() and np.isfinite(mu).all() and np.isfinite(mean).all()
    assert max(errs) < 1e-9
    assert np.all(mu[c["G"] - 1, 1] == 1.0 - sr.T_MAX)
    # gamma_mean is optional, and a block alone is the block inside the batch
    import torch
    from esn_ofdm_mimo_amd import _lib
    N, n_t, n_r, m = shape
    g = c["G"] - 1
    w1, mu1 = (torch.full((1, N, n_t), float("nan"), dtype=torch.float64, device=c["w"].device) for _ in range(2))
    _lib.check(c["tail"].lib.esn_mmse_sinr(1, N, n_t, n_r, _lib.ptr(c["p_i"][g:].contiguous()), NO,
                                           _lib.ptr(c["dev"](c["H"][g:])), _lib.ptr(w1), _lib.ptr(mu1), None,
                                           _lib.stream_handle()), "esn_mmse_sinr")
    assert torch.equal(w1[0], c["w"][g]) and torch.equal(mu1[0], c["mu"][g])


@pytest.mark.parametrize("shape", SHAPES)
def test_weighted_llrs_are_qam_llr_without_weights_and_the_restatement_with_them(shape):
    import torch
    from esn_ofdm_mimo_amd import _lib
    N, n_t, n_r, m = shape
    c = _case(shape)
    flat = torch.full((B, n_t, N * m), float("nan"), dtype=torch.float64, device=c["xh"].device)
    flat_s2 = torch.full((B,), float("nan"), dtype=torch.float64, device=c["xh"].device)
    _lib.check(c["tail"].lib.esn_qam_llr(B, N, n_t, m, _lib.ptr(c["xh"]), _lib.ptr(flat), _lib.ptr(flat_s2),
                                         _lib.stream_handle()), "esn_qam_llr")
    llr0, s20 = _weighted(c, shape, c["xh"], None, None, FPG)
    assert torch.equal(llr0, flat) and torch.equal(s20, flat_s2)
    llr, s2 = _weighted(c, shape, c["xh"], c["w"], c["mu"], FPG)
    assert torch.isfinite(llr).all() and torch.equal(s2, flat_s2)
    X = c["xh"].cpu().numpy().reshape(B, N, n_t, 2)
    want, want_s2 = sr.llr_weighted(X[..., 0] + 1j * X[..., 1], c["w"].cpu().numpy(), c["mu"].cpu().numpy(), m, FPG)
    err = float(np.max(np.abs(llr.cpu().numpy() - want)))
    print(shape, "max |llr - ref|", err, "max |ref|", np.abs(want).max(), "sigma2", np.max(np.abs(s2.cpu().numpy() / want_s2 - 1)))
    assert err <= 1e-9 * max(1.0, np.abs(want).max())
    assert np.max(np.abs(s2.cpu().numpy() / want_s2 - 1.0)) < 1e-12


def _fused(c, shape, Y, bits, p_i, w, mu, fpg, want_xhat=True):
    """detect_llr; the bank method allocates llr and sigma2 itself, so the NaN pre-fill goes through the C ABI."""
    import torch
    from esn_ofdm_mimo_amd import _lib
    N, n_t, n_r, m = shape
    b = Y.shape[0]
    g = (b + fpg - 1) // fpg
    dev = Y.device
    llr = torch.full((b, n_t, N * m), float("nan"), dtype=torch.float64, device=dev)
    s2 = torch.full((b,), float("nan"), dtype=torch.float64, device=dev)
    xh = torch.full((b, N, 2 * n_t), float("nan"), dtype=torch.float64, device=dev) if want_xhat else None
    err, nb = (torch.zeros(g, dtype=torch.int64, device=dev) if bits is not None else None for _ in range(2))
    name = "esn_detect_llr_f32" if Y.dtype == torch.float32 else "esn_detect_llr"
    _lib.check(getattr(c["tail"].lib, name)(_lib.ptr(Y), b, fpg, N, n_t, m, _lib.ptr(p_i), _lib.ptr(bits), _lib.ptr(err),
                                            _lib.ptr(nb), _lib.ptr(w), _lib.ptr(mu), _lib.ptr(llr), _lib.ptr(s2),
                                            _lib.ptr(xh), _lib.stream_handle()), name)
    return err, nb, llr, s2, xh


@pytest.mark.parametrize("io", ["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES)
def test_fused_tail_is_detect_count_then_weighted_llrs_bit_for_bit(shape, io):
    """err, bits and X_hat are esn_detect_count[_f32]'s; llr and sigma2 are esn_qam_llr_weighted's on that X_hat, bitwise:
    the fused kernel sums the sigma^2 terms in that kernel's order with as many threads."""
    import torch
    N, n_t, n_r, m = shape
    c = _case(shape)
    Y = c["Y"].to(torch.float32) if io == "f32" else c["Y"]
    e0, n0, x0 = (c["err"], c["nb"], c["xh"]) if io == "f64" else \
        c["tail"].detect_count(Y, c["bits"], c["p_i"], FPG, N, n_t, m, want_xhat=True)
    assert int(e0.sum()) > 0
    for w, mu in ((c["w"], c["mu"]), (None, None), (c["w"], None)):
        err, nb, llr, s2, xh = _fused(c, shape, Y, c["bits"], c["p_i"], w, mu, FPG)
        assert torch.equal(err, e0) and torch.equal(nb, n0) and torch.equal(xh, x0)
        want, want_s2 = _weighted(c, shape, x0, w, mu, FPG)
        assert torch.isfinite(llr).all() and torch.isfinite(s2).all()
        assert torch.equal(s2, want_s2) and torch.equal(llr, want)
    # the bank method: the same outputs, X_hat only where asked for, nothing counted without tx_bits
    out = c["tail"].detect_llr(Y, c["bits"], c["p_i"], FPG, N, n_t, m, weights=c["w"], bias=c["mu"], want_xhat=True)
    want, want_s2 = _weighted(c, shape, x0, c["w"], c["mu"], FPG)
    assert len(out) == 5 and torch.equal(out[0], e0) and torch.equal(out[1], n0) and torch.equal(out[4], x0)
    assert torch.equal(out[2], want) and torch.equal(out[3], want_s2)
    out = c["tail"].detect_llr(Y, None, c["p_i"], FPG, N, n_t, m, weights=c["w"], bias=c["mu"])
    assert len(out) == 4 and out[0] is None and out[1] is None and torch.equal(out[2], want)
    err, nb, llr, s2, xh = _fused(c, shape, Y, c["bits"], c["p_i"], c["w"], c["mu"], FPG, want_xhat=False)
    assert xh is None and torch.equal(llr, want) and torch.equal(err, e0)
    # weights and bias are float64 as given, as in LdpcCode.llrs: nothing is cast on the way
    for kw in (dict(weights=c["w"].to(torch.float32)), dict(bias=c["mu"].cpu().numpy().astype(np.float32)),
               dict(weights=c["w"][:, :-1]), dict(bias=c["mu"][:1])):
        with pytest.raises(ValueError, match="float64"):
            c["tail"].detect_llr(Y, c["bits"], c["p_i"], FPG, N, n_t, m, **kw)


@pytest.mark.parametrize("shape", SHAPES)
def test_a_frame_alone_gives_the_llrs_it_gives_inside_the_batch_under_any_group_cut(shape):
    import torch
    N, n_t, n_r, m = shape
    c = _case(shape)
    _, _, llr, s2, _ = _fused(c, shape, c["Y"], c["bits"], c["p_i"], c["w"], c["mu"], FPG)
    j = B - 1                                                 # the last frame, alone with its group's Pi and weights
    g = j // FPG
    one = _fused(c, shape, c["Y"][j:j + 1].contiguous(), c["bits"][j:j + 1].contiguous(), c["p_i"][g:g + 1].contiguous(),
                 c["w"][g:g + 1].contiguous(), c["mu"][g:g + 1].contiguous(), 1)
    assert torch.equal(one[2][0], llr[j]) and torch.equal(one[3][0], s2[j])
    assert int(one[0][0]) <= int(c["err"][g]) and int(one[1][0]) == N * m * n_t
    grp = torch.arange(B, device=llr.device) // FPG           # one frame per group, every frame with copies of its group's
    cut = _fused(c, shape, c["Y"], c["bits"], c["p_i"][grp].contiguous(), c["w"][grp].contiguous(),
                 c["mu"][grp].contiguous(), 1)
    assert torch.equal(cut[2], llr) and torch.equal(cut[3], s2)
    assert int(cut[0].sum()) == int(c["err"].sum())
    wl, ws2 = _weighted(c, shape, c["xh"][j:j + 1].contiguous(), c["w"][g:g + 1].contiguous(),
                        c["mu"][g:g + 1].contiguous(), 1)
    assert torch.equal(wl[0], llr[j]) and torch.equal(ws2[0], s2[j])


@pytest.mark.parametrize("io", ["f64", "f32"])
def test_one_frame_at_the_lds_limit(io):
    """N = 2048, n_t = 4: 147 520 of the 153 600 bytes of LDS a workgroup may ask for."""
    import torch
    shape = (2048, 4, 4, 4)
    N, n_t, n_r, m = shape
    c = dict(tail=_tail())
    assert c["tail"].lib.esn_detect_llr_lds_bytes(N, n_t) == 147520
    rs = np.random.RandomState(5)
    p_i = np.array([3e-4])
    Y, bits = _frames(rs, 1, N, n_t, m, p_i)
    dev = c["tail"].device
    Y = torch.as_tensor(Y, device=dev, dtype=torch.float32 if io == "f32" else torch.float64)
    bits, p_i = torch.as_tensor(bits, device=dev), torch.as_tensor(p_i, device=dev)
    w = torch.as_tensor(0.5 + rs.rand(1, N, n_t), device=dev)
    mu = torch.as_tensor(0.5 + 0.5 * rs.rand(1, N, n_t), device=dev)
    e0, n0, x0 = c["tail"].detect_count(Y, bits, p_i, 1, N, n_t, m, want_xhat=True)
    err, nb, llr, s2, xh = _fused(c, shape, Y, bits, p_i, w, mu, 1)
    want, want_s2 = _weighted(c, shape, x0, w, mu, 1)
    assert torch.equal(err, e0) and torch.equal(nb, n0) and torch.equal(xh, x0)
    assert torch.isfinite(llr).all() and torch.equal(llr, want) and torch.equal(s2, want_s2)


# ---------------------------------------------------------------------------------------------- coded_equalized_point
@pytest.fixture(scope="module")
def mc():
    from esn_ofdm_mimo_amd import montecarlo
    return montecarlo


SMALL = dict(n_t=2, n_r=2, n_sub=32, m=2)
_points = {}


def _small_point(mc, llr):
    """coded_equalized_point on the 2x2 / N = 32 / QPSK link, 4 blocks x 3 frames, code (64, .), once per llr."""
    if llr not in _points:
        from esn_ofdm_mimo_amd.coded import LdpcCode
        p = mc.LinkParams(**SMALL)
        code = _points.setdefault("code", LdpcCode(p.n_sub * p.m, 4, 8, seed=5))
        _points[llr] = mc.coded_equalized_point(mc.FrameSource(p, seed=6), code, 9.0, 2, 4, llr=llr, frames_per_block=3,
                                                seed=3)
    return _points[llr]


def test_flat_point_has_the_mmse_leg_of_coded_ber_point_bit_for_bit(mc):
    r = _small_point(mc, "flat")
    sweep = mc.DetectorSweep(mc.LinkParams(**SMALL), n_reservoir=16, seed=6, precision="f64")
    ref = mc.coded_ber_point(sweep, _points["code"], 9.0, 2, 4, frames_per_block=3, seed=3)
    print("flat", {k: r[k] for k in ("ESN_uncoded", "MMSE_uncoded", "ESN_coded", "MMSE_coded")}, "a", r["a_mmse"], r["a_esn"])
    assert set(r) == set(ref)
    assert r["MMSE_uncoded"] == ref["MMSE_uncoded"] and r["MMSE_coded"] == ref["MMSE_coded"]
    assert np.array_equal(r["a_mmse"], ref["a_mmse"]) and np.array_equal(r["b_mmse"], ref["b_mmse"])
    assert 0.0 < r["MMSE_uncoded"] < 0.5 and 0.0 <= r["ESN_uncoded"] < 0.5


def test_sinr_point_runs_with_finite_slopes_and_the_flat_points_uncoded_columns(mc):
    flat, sinr = _small_point(mc, "flat"), _small_point(mc, "sinr")
    print("sinr", {k: sinr[k] for k in ("ESN_uncoded", "MMSE_uncoded", "ESN_coded", "MMSE_coded")}, "a", sinr["a_mmse"],
          sinr["a_esn"])
    assert sinr["ESN_uncoded"] == flat["ESN_uncoded"] and sinr["MMSE_uncoded"] == flat["MMSE_uncoded"]
    for k in ("a_esn", "b_esn", "a_mmse", "b_mmse"):
        assert sinr[k].shape == (2,) and np.isfinite(sinr[k]).all()
    assert 0.0 <= sinr["ESN_coded"] <= 1.0 and 0.0 <= sinr["MMSE_coded"] <= 1.0
    assert not np.array_equal(sinr["a_mmse"], flat["a_mmse"])


def test_esn_leg_against_the_numpy_chain_on_the_same_coded_bits(mc):
    """2 blocks x 2 frames, no state noise: the coded frames are made again (points._coded_block_data, the point's own
    key), the NumPy chain behind the equaliser runs on them with the point's reservoir, and X_hat agrees within 1e-8 of
    its largest magnitude; the error count agrees exactly where the chain's smallest distance from a slicer threshold
    exceeds 1e-5 -- the margin rule of test_point_against_the_numpy_chain in tests/test_gpu_equalized_esn.py, the test
    of equalized_esn_point this one is the coded counterpart of."""
    from esn_ofdm_mimo_amd import points
    from esn_ofdm_mimo_amd.coded import LdpcCode
    ebno, G, F, n_res, ridge, seed, snr_idx = 15.0, 2, 2, 8, 1e-5, 9, 1
    p = mc.LinkParams(**SMALL)
    code = _points.setdefault("code", LdpcCode(p.n_sub * p.m, 4, 8, seed=5))
    src = mc.FrameSource(p, seed=seed)
    r = mc.coded_equalized_point(src, code, ebno, snr_idx, G, llr="flat", n_reservoir=n_res, ridge=ridge, noise=0.0,
                                 frames_per_block=F, seed=4, want_xhat=True)
    u, tx_bits, _, (pbits, px, py), py_ls, dy = points._coded_block_data(src, code, ebno, snr_idx, G, F, 4, 12345)
    H = src.estimate_channel(pbits, py_ls, ebno).cpu().numpy()
    p_i = np.full(G, p.p_i(ebno))
    _, pilot_rows = qr.equalize(py.cpu().numpy(), H, p_i, p.no, p.cp, 0, 1)
    _, data_rows = qr.equalize(dy.cpu().numpy(), H, p_i, p.no, p.cp, 0, F)
    pilot_x, bits = px.cpu().numpy(), tx_bits.cpu().numpy()
    weights = mc.draw_reservoir(2 * p.n_t, 2 * p.n_t, n_res, 0.9, 0.1, seed * 7919 + 17)
    want_x, want_err = [], 0
    for b in range(G):
        esn = qr.make_esn(p.n_t, n_res, p.input_scaling(ebno), p.teacher_scale, ridge, noise=0.0, weights=weights)
        X, hard = qr.chain_block(esn, pilot_rows[b], pilot_x[b], data_rows[b * F:(b + 1) * F], p.n_sub, p.cp, 0, p_i[b], p.m)
        want_x.append(X)
        want_err += sum(int(np.sum(hard[f] != bits[b * F + f])) for f in range(F))
    want_x = np.concatenate(want_x)
    margin = qr.slicer_margin(want_x, p.m)
    e = float(np.max(np.abs(r["x_esn"].cpu().numpy() - want_x)) / np.max(np.abs(want_x)))
    print("X_hat", e, "slicer margin", margin, "ESN_uncoded", r["ESN_uncoded"], "chain errors", want_err)
    assert e < 1e-8
    assert margin > 1e-5
    assert r["ESN_uncoded"] == want_err / float(G * F * p.n_sub * p.m * p.n_t)
