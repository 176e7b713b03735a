"""The coded leg (esn_ldpc_encode, esn_qam_llr, esn_ldpc_decode_count; coded.py) at the shapes in use and at its edges.

tests/test_gpu_coded.py runs each kernel at one shape and accepts the decoder when 95 % of the words agree.  Here:

  * LLRs and sigma^2 for every constellation size the API takes, for the per-stream call of block_fading_point
    (n_t = 1, 64 or 128 elements in a 256-thread block), odd sizes, one element, points on the constellation, on decision
    boundaries, outside it, -0.0, and a noise-free frame whose sigma^2 sits at the 1e-12 floor -- against a brute force
    in long double (tests/ldpc_ref.py) under a bound derived from the kernel's roundings, and against the uncoded
    detector's hard decisions;
  * the encoder for four code sizes and inputs whose upper bits are set;
  * the decoder EXACTLY: every word equals oracle.ldpc_oracle.decode_bp after 1, 2, 3, ... iterations, wherever the
    oracle's own trace shows that no decision and no check product is within 1e-6 of a tie (then a one-ulp difference in
    tanh / log cannot flip a bit); on a cycle-free graph against bitwise MAP by enumeration, i.e. against mathematics and
    not a restatement; with saturated messages (X = +-1, the two special branches); the group counters; the largest
    graph that fits the LDS, and the first that does not."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ldpc_ref  # noqa: E402
from oracle import esn_oracle as eo  # noqa: E402
from oracle import ldpc_oracle as lo  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
MARGIN = 1e-6            # no |L_post| and no 1 - |X| below this over the compared iterations


@functools.lru_cache(maxsize=None)
def _code(n=512, d_v=4, d_c=8):
    from esn_ofdm_mimo_amd.coded import LdpcCode
    return LdpcCode(n, d_v, d_c, seed=5)


def _dev(code, a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=code.device)


# ---------------------------------------------------------------------------------------------------------------- LLRs
LLR_SHAPES = [(2, 64, 1, 4),        # SISO per-stream call
              (4, 128, 1, 4),       # per-stream call
              (6, 48, 3, 2),        # 144 elements, not a multiple of 64
              (8, 37, 2, 2),        # odd subcarrier count
              (10, 16, 1, 2),       # less than one wave
              (4, 1, 1, 3),         # single element
              (2, 300, 3, 2)]       # 900 elements, not a multiple of 256


def _plants(m):
    """(value, Re in level units, Im in level units); None = off the lattice of levels and boundaries."""
    side, norm = 1 << (m // 2), np.sqrt(2.0 * ((1 << m) - 1) / 3.0)
    lv = side - 1
    return [(complex(0.0, 0.0), 0, 0),                                   # on both boundaries through the origin
            (complex(2 / norm, -2 / norm), 2, -2),                       # boundaries between the levels 1 and 3 (m >= 4)
            (complex(3.0, -3.0), None, None),                            # outside on both axes
            (complex(-3.0, 1 / norm), None, 1),                          # outside on one axis
            (complex(-0.0, -0.0), 0, 0),
            (eo.unit_qam(m)[side - 1], -lv, lv),                         # exactly a point (a corner)
            (complex(-2 / norm, 1 / norm), -2, 1),                       # a boundary on one axis only
            (complex(-3.0, 3.0), None, None)]


def _ties(units, m):
    """Bits of one axis left undecided at `units` (an even number of half level spacings from the origin): those in
    which the two equidistant levels differ."""
    side = 1 << (m // 2)
    if units is None or units % 2 or abs(units) + 1 > side - 1:
        return 0
    a0 = (units - 1 + side - 1) // 2
    return bin(a0 ^ (a0 + 1)).count("1")


@functools.lru_cache(maxsize=None)
def _llr_case(shape):
    """Frames for one shape, the kernel's answer and the long-double reference, computed once.  Frames 0 .. B-2 are
    constellation points plus 0.15 complex Gaussian noise with the plants written over some elements; the last frame
    is entirely noise-free (plants would lift its sigma^2 off the floor, so it has none)."""
    m, n_sub, n_t, B = shape
    code = _code()
    rs = np.random.RandomState(1000 * m + n_sub)
    const = eo.unit_qam(m)
    x = const[rs.randint(0, 2 ** m, size=(B, n_sub, n_t))]
    x[:B - 1] += 0.15 * (rs.randn(B - 1, n_sub, n_t) + 1j * rs.randn(B - 1, n_sub, n_t))
    plants = _plants(m)
    n_el = n_sub * n_t
    n_pl = min(len(plants), n_el - 1)                   # at least one element of a frame stays an ordinary noisy point
    boundary = np.zeros((B, n_el), dtype=bool)
    ties = exact = 0
    for b in range(B - 1):
        pos = rs.permutation(n_el)[:n_pl]
        flat = x[b].reshape(-1)                         # a view: x is contiguous
        for (val, re_u, im_u), p in zip(plants, pos):
            flat[p] = val
            t = _ties(re_u, m) + _ties(im_u, m)
            ties += t
            exact += (_ties(re_u, m) if re_u == 0 else 0) + (_ties(im_u, m) if im_u == 0 else 0)
            boundary[b, p] = t > 0
    llr, s2 = code.llrs(_dev(code, x), m)
    assert llr.shape == (B, n_t, n_sub * m) and s2.shape == (B,)
    want_s2 = np.array([np.mean([lo.sigma2_from_decisions(x[b, :, tx], m) for tx in range(n_t)]) for b in range(B)])
    want = np.empty((B, n_t, n_sub, m), dtype=np.longdouble)
    dsum = np.empty_like(want)
    for b in range(B):
        for tx in range(n_t):
            want[b, tx], dsum[b, tx] = ldpc_ref.llr_longdouble(x[b, :, tx], m, want_s2[b])
    # the kernel rounds each squared distance a few times and then subtracts; the second term is the relative error
    # of the sigma^2 sum
    tol = 16 * EPS * dsum / np.maximum(want_s2, 1e-12)[:, None, None, None] + 1e-13 * np.abs(want)
    return dict(x=x, llr=llr.cpu().numpy().reshape(B, n_t, n_sub, m), s2=s2.cpu().numpy(), want_s2=want_s2, want=want,
                tol=tol, ties=ties, exact=exact, boundary=boundary.reshape(B, n_sub, n_t), llr_dev=llr, s2_dev=s2)


@pytest.mark.parametrize("shape", LLR_SHAPES, ids=lambda s: "m%d-N%d-nt%d-B%d" % s)
def test_llrs_and_sigma2_against_long_double(shape):
    m, n_sub, n_t, B = shape
    c = _llr_case(shape)
    rel = np.abs(c["s2"] - c["want_s2"]) / c["want_s2"]
    ratio = float((np.abs(c["llr"] - c["want"]) / c["tol"]).max())
    print(f"{shape}: sigma2 {c['want_s2']}, rel err {rel.max():.1e}; max |llr - want| / bound = {ratio:.3f}; "
          f"max |llr| {np.abs(c['llr']).max():.3e}")
    assert np.all(rel <= 1e-12)
    assert c["want_s2"][B - 1] == 1e-12 and np.all(c["want_s2"][:B - 1] > 1e-3)     # the floor, and well off it
    assert np.all(np.isfinite(c["llr"]))
    assert np.all(np.abs(c["llr"] - c["want"]) <= c["tol"])
    assert np.abs(c["llr"][B - 1]).max() > 1e10                                     # LLRs near 1e12 d at the floor


@pytest.mark.parametrize("shape", LLR_SHAPES, ids=lambda s: "m%d-N%d-nt%d-B%d" % s)
def test_llr_signs_are_the_uncoded_detectors_hard_bits(shape):
    """[B, n_t, N, m] against hard_bits' [N m, n_t].  A sign is compared wherever the reference LLR exceeds the bound of
    the test above, i.e. wherever that test determines it.  What is left out are the planted boundary points and
    nothing else: the bits in which the two equidistant levels differ, exactly 0 in the reference for the boundaries
    through the origin; +-2 / norm is not a float64 midpoint of its neighbours, its LLR a few ulp of either sign."""
    m, n_sub, n_t, B = shape
    c = _llr_case(shape)
    const = eo.unit_qam(m)
    decided = np.abs(c["want"]) > c["tol"]                                          # [B, n_t, N, m]
    assert (~decided).sum() == c["ties"] and c["exact"] <= (c["want"] == 0).sum() <= c["ties"], \
        ((~decided).sum(), c["ties"], (c["want"] == 0).sum(), c["exact"])
    assert not (~decided).any(axis=3).transpose(0, 2, 1)[~c["boundary"]].any()
    n_pl = min(n_sub * n_t - 1, 8)                      # the origin is planted as 0.0 (first) and as -0.0 (fifth)
    assert c["exact"] == m * (B - 1) * ((n_pl >= 1) + (n_pl >= 5))
    n_cmp = 0
    for b in range(B):
        hard = eo.hard_bits(c["x"][b], const, m)                                    # [N m, n_t]
        neg = (c["llr"][b] < 0).transpose(1, 2, 0).reshape(n_sub * m, n_t)
        ok = decided[b].transpose(1, 2, 0).reshape(n_sub * m, n_t)
        assert np.array_equal(neg[ok], hard[ok] == 1)
        n_cmp += ok.sum()
    assert n_cmp == B * n_sub * n_t * m - c["ties"]


@pytest.mark.parametrize("shape", LLR_SHAPES, ids=lambda s: "m%d-N%d-nt%d-B%d" % s)
def test_per_stream_call_of_block_fading_point(shape):
    """x.permute(0, 2, 1).reshape(-1, N, 1): one sigma^2 per (frame, stream), the LLRs scaled by it."""
    m, n_sub, n_t, B = shape
    c, code = _llr_case(shape), _code()
    per_stream = _dev(code, c["x"]).permute(0, 2, 1).reshape(-1, n_sub, 1).contiguous()
    llr, s2 = code.llrs(per_stream, m)
    assert llr.shape == (B * n_t, 1, n_sub * m)
    llr, s2 = llr.cpu().numpy().reshape(B, n_t, n_sub, m), s2.cpu().numpy().reshape(B, n_t)
    for b in range(B):
        for tx in range(n_t):
            w2 = lo.sigma2_from_decisions(c["x"][b, :, tx], m)
            assert abs(s2[b, tx] - w2) <= 1e-12 * w2
            want, dsum = ldpc_ref.llr_longdouble(c["x"][b, :, tx], m, w2)
            assert np.all(np.abs(llr[b, tx] - want) <= 16 * EPS * dsum / max(w2, 1e-12) + 1e-13 * np.abs(want))
    if n_t > 1:                                         # streams of one frame do differ in sigma^2
        assert np.ptp(s2[0]) > 1e-3 * s2[0].max()


@pytest.mark.parametrize("shape", LLR_SHAPES, ids=lambda s: "m%d-N%d-nt%d-B%d" % s)
def test_llr_frames_are_independent_and_sigma2_is_optional(shape):
    import torch
    from esn_ofdm_mimo_amd import _lib
    from esn_ofdm_mimo_amd._lib import check, ptr
    m, n_sub, n_t, B = shape
    c, code = _llr_case(shape), _code()
    for b in range(B):
        llr1, s21 = code.llrs(_dev(code, c["x"][b:b + 1]), m)
        assert torch.equal(llr1[0], c["llr_dev"][b]) and torch.equal(s21[0], c["s2_dev"][b])
    xd = _dev(code, c["x"])
    out = torch.full_like(c["llr_dev"], float("nan"))
    check(_lib.load().esn_qam_llr(B, n_sub, n_t, m, ptr(xd), ptr(out), None, _lib.stream_handle()), "esn_qam_llr")
    assert torch.equal(out, c["llr_dev"])


@pytest.mark.parametrize("m,B,n_t,N", [(2, 2, 1, 64), (6, 2, 3, 16)])
def test_calibration_at_other_constellation_sizes(m, B, n_t, N):
    code = _code()
    rs = np.random.RandomState(20 + m)
    bits = (rs.rand(B, N * m, n_t) > 0.5).astype(np.uint8)
    llr = rs.randn(B, n_t, N * m) * 3 - (2.0 * np.transpose(bits, (0, 2, 1)) - 1.0) * 1.5
    a, b = code.fit_calibration(_dev(code, llr), _dev(code, bits), m)
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert a.shape == b.shape == (m,)
    for bit in range(m):
        xs = llr.reshape(B, n_t, N, m)[..., bit].reshape(-1)
        ys = np.transpose(bits, (0, 2, 1)).reshape(B, n_t, N, m)[..., bit].reshape(-1).astype(float)
        wa, wb = lo.fit_logreg_1d(xs, ys, maxiter=400, lr=0.1, l2=1e-3)
        assert abs(a[bit] - wa) < 1e-9 and abs(b[bit] - wb) < 1e-9
        assert wa < 0


# ------------------------------------------------------------------------------------------------------------- encoder
@pytest.mark.parametrize("n,d_v,d_c,n_t,B", [(16, 2, 4, 1, 3), (96, 3, 6, 2, 7), (512, 4, 8, 1, 5), (512, 4, 8, 3, 2),
                                             (2104, 4, 8, 2, 1)])
def test_encoder_reads_bit_0_only(n, d_v, d_c, n_t, B):
    code = _code(n, d_v, d_c)
    assert code.H.shape == (n * d_v // d_c, n) and np.all(code.H.sum(0) == d_v) and np.all(code.H.sum(1) == d_c)
    rs = np.random.RandomState(n + n_t)
    u = np.array([0, 1, 2, 3, 254, 255], dtype=np.uint8)[rs.randint(0, 6, size=(B, n_t, code.k))]
    bits = code.encode(_dev(code, u), n_t).cpu().numpy()
    assert bits.shape == (B, n, n_t) and bits.dtype == np.uint8
    cw = np.transpose(bits, (0, 2, 1))                                              # [B, n_t, n]
    np.testing.assert_array_equal(cw, lo.encode(code.P, u & 1))
    assert not ((cw.reshape(-1, n).astype(int) @ code.H.T.astype(int)) % 2).any()
    np.testing.assert_array_equal(cw[..., :code.k], u & 1)
    assert (u > 1).mean() > 0.5 and 0.3 < (u & 1).mean() < 0.7


# ------------------------------------------------------------------------------------------------------------- decoder
def _decode_direct(code, H, y, k, maxiter, u_true=None, cw_per_group=None):
    """esn_ldpc_decode_count for an arbitrary parity-check matrix.  Returns (rc, message, x_out, err, nbits); x_out is
    pre-filled with 7, which no launch leaves behind."""
    import torch
    from esn_ofdm_mimo_amd import _lib
    from esn_ofdm_mimo_amd._lib import ptr
    lib = _lib.load()
    H = np.asarray(H)
    n_cw, n = y.shape
    assert H.shape[1] == n and 0 < k <= n
    graph = [_dev(code, a) for a in ldpc_ref.graph_arrays(H)]
    yd = _dev(code, np.asarray(y, dtype=np.float64))
    cpg = n_cw if cw_per_group is None else cw_per_group
    g = (n_cw + cpg - 1) // cpg
    xo = torch.full((n_cw, n), 7, dtype=torch.uint8, device=code.device)
    err = torch.zeros(g, dtype=torch.int64, device=code.device)
    nb = torch.zeros(g, dtype=torch.int64, device=code.device)
    ud = None
    if u_true is not None:
        assert u_true.shape == (n_cw, k)
        ud = _dev(code, u_true.astype(np.uint8))
    rc = lib.esn_ldpc_decode_count(n_cw, n, k, H.shape[0], int(H.sum()), ptr(graph[0]), ptr(graph[1]), ptr(graph[2]),
                                   ptr(graph[3]), ptr(yd), 1.0, int(maxiter), ptr(ud), cpg, ptr(xo), ptr(err), ptr(nb),
                                   _lib.stream_handle())
    msg = lib.esn_last_error().decode(errors="replace") if rc else ""
    return rc, msg, xo.cpu().numpy(), err.cpu().numpy(), nb.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _awgn_words(n, d_v, d_c, n_cw, sigma, seed, trace_iters):
    """Codewords of _code(n, d_v, d_c) behind BPSK and noise sigma, as calibrated LLRs (a = -1, b = 0 leaves them as
    they are) and as the decoder's observations; and the oracle's trace of them."""
    code = _code(n, d_v, d_c)
    rs = np.random.RandomState(seed)
    u = (rs.rand(n_cw, code.k) > 0.5).astype(np.uint8)
    c = lo.encode(code.P, u)
    llr = 2.0 * ((1.0 - 2.0 * c) + sigma * rs.randn(*c.shape)) / sigma ** 2
    yobs = 0.5 * np.clip(llr, -20, 20)
    L_post, margin = ldpc_ref.bp_trace(code.H, yobs, 1.0, trace_iters)
    return u, llr, yobs, L_post, margin


def _decode(code, llr, u, n_t, cw_per_group, maxiter, **kw):
    import torch
    a = torch.full((4,), -1.0, dtype=torch.float64, device=code.device)               # -(a x + b) = x
    b = torch.zeros(4, dtype=torch.float64, device=code.device)
    x_llr = _dev(code, llr.reshape(-1, n_t, llr.shape[-1]))
    return code.decode_count(x_llr, a, b, None if u is None else _dev(code, u), cw_per_group=cw_per_group, bits_per_sym=4,
                             maxiter=maxiter, **kw)


def _assert_no_near_tie(L_post, margin, iters, what):
    lp, mg = np.abs(L_post[:iters]).min(), margin[:iters].min()
    print(f"{what}: over {iters} iterations min |L_post| = {lp:.2e}, min (1 - |X|) = {mg:.2e}")
    assert lp >= MARGIN and mg >= MARGIN, "these inputs come too close to a tie: change the seed, not the bound"


PREFIX = [(0.9, it) for it in (1, 2, 3, 4, 6)] + [(1.1, it) for it in (1, 2, 3, 4, 6)] + [(0.7, it) for it in (1, 2, 3)]


@pytest.mark.parametrize("sigma,maxiter", PREFIX)
def test_decoder_iteration_prefix_is_the_oracles(sigma, maxiter):
    code = _code()
    u, llr, yobs, L_post, margin = _awgn_words(512, 4, 8, 16, sigma, 6, 3 if sigma == 0.7 else 6)
    _assert_no_near_tie(L_post, margin, maxiter, f"sigma {sigma}")
    err, nb, xo = _decode(code, llr, u, 4, 4, maxiter, want_bits=True)
    want = lo.decode_bp(code.H, yobs, 1.0, maxiter)
    np.testing.assert_array_equal(xo.cpu().numpy(), want)                           # every word, every bit
    np.testing.assert_array_equal(want, ldpc_ref.trace_decision(code.H, L_post[:maxiter])[0])
    want_err = (want[:, :code.k] != u).reshape(4, -1).sum(axis=1)
    np.testing.assert_array_equal(err.cpu().numpy(), want_err)
    np.testing.assert_array_equal(nb.cpu().numpy(), [4 * code.k] * 4)
    if maxiter <= 2:
        assert want_err.min() > 0                                                   # nothing is decoded yet: a real prefix


def test_decoder_is_exact_map_on_a_tree():
    code = _code()
    H, y = ldpc_ref.tree_code(seed=0)
    L_map = ldpc_ref.exact_bit_llrs(H, 2.0 * y / 10.0 ** (-0.1))[:, :10]
    assert np.abs(L_map).min() >= 1e-6
    map_bits = (L_map <= 0).astype(np.uint8)
    rc, msg, xo, err, nb = _decode_direct(code, H, y, 10, 8, u_true=map_bits, cw_per_group=64)
    assert rc == 0, msg
    np.testing.assert_array_equal(xo[:, :10], map_bits)
    assert np.all(xo[:, 10] == 1)                                                   # the gadget never lets a word stop
    assert err.tolist() == [0] * 4 and nb.tolist() == [640] * 4
    assert 0.2 < map_bits.mean() < 0.8 and (map_bits != (y[:, :10] <= 0)).sum() > 100   # MAP is not the channel's sign


def test_decoder_saturated_messages_take_the_special_branches():
    """y = +-50: Lc is about 126 and tanh(Lc / 2) is exactly 1, so every check product is +1 (den == 0) or -1
    (num == 0).  Each message is then +-1 against |Lc| = 126, and the decision stays the channel's sign."""
    code = _code()
    rs = np.random.RandomState(8)
    u = (rs.rand(6, code.k) > 0.5).astype(np.uint8)
    c = lo.encode(code.P, u)
    flip = rs.rand(*c.shape) < 0.02
    flip[0] = False
    y = 50.0 * (1.0 - 2.0 * c) * np.where(flip, -1.0, 1.0)
    assert np.tanh(0.5 * 2.0 * 50.0 / 10.0 ** (-0.1)) == 1.0
    rc, msg, xo, err, nb = _decode_direct(code, code.H, y, code.k, 5, u_true=u, cw_per_group=1)
    assert rc == 0, msg
    np.testing.assert_array_equal(xo, (y <= 0).astype(np.uint8))
    np.testing.assert_array_equal(xo[0], c[0])
    np.testing.assert_array_equal(err, flip[:, :code.k].sum(axis=1))
    assert nb.tolist() == [code.k] * 6 and err[1:].min() > 0
    np.testing.assert_array_equal(lo.decode_bp(code.H, y, 1.0, 5), xo)


def test_decoder_group_accounting():
    import torch
    code = _code()
    k, its = code.k, 3
    u, llr, yobs, L_post, margin = _awgn_words(512, 4, 8, 16, 0.9, 6, 6)
    u, llr, yobs = u[:10], llr[:10], yobs[:10]
    _assert_no_near_tie(L_post[:, :10], margin[:, :10], its, "groups")
    want = lo.decode_bp(code.H, yobs, 1.0, its)
    wrong = (want[:, :k] != u).sum(axis=1)
    want_err = [wrong[:4].sum(), wrong[4:8].sum(), wrong[8:].sum()]
    assert min(want_err) > 0 and len(set(want_err)) == 3
    err, nb, xo = _decode(code, llr, u, 2, 4, its, want_bits=True)                  # 5 frames of 2 streams, groups of 4
    np.testing.assert_array_equal(xo.cpu().numpy(), want)
    assert err.cpu().tolist() == want_err and nb.cpu().tolist() == [4 * k, 4 * k, 2 * k]
    # counters supplied by the caller are added to
    err2 = torch.tensor([1000, 2000, 3000], dtype=torch.int64, device=code.device)
    nb2 = torch.tensor([7, 70, 700], dtype=torch.int64, device=code.device)
    e, b = _decode(code, llr, u, 2, 4, its, err=err2, nbits=nb2)
    assert e is err2 and b is nb2
    assert err2.cpu().tolist() == [1000 + want_err[0], 2000 + want_err[1], 3000 + want_err[2]]
    assert nb2.cpu().tolist() == [7 + 4 * k, 70 + 4 * k, 700 + 2 * k]
    # no transmitted bits: decisions only
    e, b, xo = _decode(code, llr, None, 2, 4, its, want_bits=True)
    np.testing.assert_array_equal(xo.cpu().numpy(), want)
    assert e.cpu().tolist() == [0, 0, 0] and b.cpu().tolist() == [0, 0, 0]


def test_decoder_words_are_independent_of_their_batch():
    code = _code()
    u, llr, yobs, _, _ = _awgn_words(512, 4, 8, 16, 1.1, 6, 6)
    u, llr = u[:6], llr[:6]
    _, _, batch = _decode(code, llr, u, 1, 6, 6, want_bits=True)
    _, _, rev = _decode(code, llr[::-1], u[::-1], 1, 6, 6, want_bits=True)
    batch, rev = batch.cpu().numpy(), rev.cpu().numpy()
    np.testing.assert_array_equal(rev[::-1], batch)
    for w in (0, 5):
        _, _, alone = _decode(code, llr[w:w + 1], u[w:w + 1], 1, 1, 6, want_bits=True)
        np.testing.assert_array_equal(alone.cpu().numpy()[0], batch[w])
    assert len({row.tobytes() for row in batch}) == 6


@pytest.mark.parametrize("n,d_v,d_c,n_cw,seed", [(16, 2, 4, 16, 1), (96, 3, 6, 16, 1), (2104, 4, 8, 2, 1)])
def test_decoder_small_and_large_graphs(n, d_v, d_c, n_cw, seed):
    """n = 2104 needs 16 E + 9 n = 153,592 bytes of dynamic LDS, the largest (4, 8) length launch_ldpc_decode serves."""
    code = _code(n, d_v, d_c)
    assert 16 * code.n_edges + 9 * n <= 150 * 1024
    u, llr, yobs, L_post, margin = _awgn_words(n, d_v, d_c, n_cw, 0.9, seed, 3)
    _assert_no_near_tie(L_post, margin, 3, f"n = {n}")
    err, nb, xo = _decode(code, llr, u, 1, n_cw, 3, want_bits=True)
    want = lo.decode_bp(code.H, yobs, 1.0, 3)
    np.testing.assert_array_equal(xo.cpu().numpy(), want)
    assert err.cpu().tolist() == [(want[:, :code.k] != u).sum()] and nb.cpu().tolist() == [n_cw * code.k]
    assert (want != (yobs <= 0)).any()                                              # the iterations did change bits


def test_decoder_refuses_a_graph_beyond_the_lds():
    """n = 2112: 154,176 bytes > 150 KB.  The error names the limit and nothing is launched."""
    code = _code()
    H = lo.gallager_parity_check(2112, 4, 8, np.random.RandomState(3))
    assert 16 * int(H.sum()) + 9 * 2112 == 154176 > 150 * 1024
    y = np.ones((2, 2112))
    rc, msg, xo, err, nb = _decode_direct(code, H, y, 1059, 3, u_true=np.zeros((2, 1059), dtype=np.uint8))
    assert rc == -2 and "does not fit LDS" in msg, (rc, msg)
    assert np.all(xo == 7) and err.tolist() == [0] and nb.tolist() == [0]
