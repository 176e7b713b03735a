"""DetectorSweep(track="decisions" | "genie"): the read-out re-fitted after every data symbol of a block.

Against tests/tracking_ref.py (the tracked loop on the CPU oracle, one block at a time), fed the device's own frames
(generated over its taps_sym) and reservoir: 2x2, "exp", fading="jakes", N = 16, isi = 8, QPSK, N_res = 16 -- 20 read-out
columns against 16 rows at window 1 and 32 rows at window 2, so both solve forms (rows < cols, rows > cols) -- float64
predict and fit, no state noise, 3 blocks x 6 data symbols.  Per-symbol error counts exactly equal; each symbol's X_hat
within BOUND of max.

BOUND.  tests/test_gpu_driver_loop.py holds the device to ESN_BOUND = 1e-10 of max, derived in
tests/test_oracle_driver_loop.py from cond(E) of the reference's own fits: 10 cond(E) 2^-52 for a QR solve and
10 cond(E)^2 2^-52 = 8.5e-11 for the normal equations at the fixtures' cond(E) = 196.  The sweep solves by Cholesky on the
Gram matrix ("auto"), and the stacked fits of this small configuration (16 or 32 rows of a 16-unit reservoir) are worse
conditioned than those fixtures, so the same rule is applied to the reference's own stacked E on the CPU:
BOUND = max(ESN_BOUND, 10 max_k cond(E_k)^2 2^-52), computed in the test from tracking_ref's cond, printed, and required
to stay a decade below the smallest distance of the reference's X_hat to a decision boundary, which itself must be
at least 1e-6 (the seed is chosen for that): the counts can then be compared exactly.

Invariance (state noise 0.001): counters and symbol_error_counts are bit-identical for chunk_blocks in {1, 3, all} and
for the sum of ranks 0 and 1 of a world of 2; per-symbol counts sum to the totals.  track=None is the sweep built without
the argument.  "decisions" and "genie" agree on data symbol 0.  And tracking does something: at fd_tsym = 0.02 the
whole-block BER orders genie < decisions < static."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tracking_ref  # noqa: E402
from oracle import driver_loop as dl  # noqa: E402
from oracle import esn_oracle as eo  # noqa: E402

pytestmark = pytest.mark.gpu

ESN_BOUND = dl.ESN_BOUND
G, F, N_RES, EBNO, SEED = 3, 6, 16, 21.0, 5
FD_TSYM = 0.01


def _params(n_sub=16, fd_tsym=FD_TSYM, frames=F, fading="jakes", m=2):
    from esn_ofdm_mimo_amd.montecarlo import LinkParams
    p = dataclasses.replace(LinkParams.block_fading(2, 2, n_sub=n_sub), m=m)
    return dataclasses.replace(p, coherence_fixed=frames, f_d=fd_tsym * p.fs / (p.n_sub + p.cp), fading=fading)


def _sweep(params=None, n_res=N_RES, noise=0.0, precision="f64", **kw):
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep
    return DetectorSweep(params or _params(), n_reservoir=n_res, precision=precision, fit_precision="f64", seed=SEED,
                         noise=noise, **kw)


@pytest.fixture(scope="module")
def device_frames():
    """what chunk (Eb/No index 0, blocks 0 .. G - 1) of the sweeps below generates, on the host, and the shared reservoir"""
    sw = _sweep()
    d = sw.src.blocks_fast(EBNO, 0, 0, G, F, want_data_x=True)
    assert tuple(d["taps_sym"].shape)[:2] == (G, 1 + F)
    p = sw.p
    host = {k: d[k].cpu().numpy() for k in ("pilot_y", "pilot_x", "data_y", "data_x", "data_bits")}
    for k in ("data_y", "data_x", "data_bits"):
        host[k] = host[k].reshape(G, F, *host[k].shape[1:])
    host["weights"] = tuple(w[0].cpu().numpy() for w in sw.bank.weights)
    host["p"] = p
    return host


def _reference(host, track, window):
    p = host["p"]
    out = []
    for b in range(G):
        esn = eo.OracleESN(2 * p.n_r, 2 * p.n_t, N_RES, noise=0.0, input_scaling=p.input_scaling(EBNO) * np.ones(2 * p.n_r),
                           teacher_scaling=p.teacher_scale * np.ones(2 * p.n_t), random_state=1, weights=host["weights"])
        out.append(tracking_ref.track_block(esn, host["pilot_y"][b], host["pilot_x"][b], host["data_y"][b],
                                            host["data_bits"][b], host["data_x"][b], p.n_sub, p.cp, p.n_t, p.n_r, p.delay,
                                            p.p_i(EBNO), p.m, track, window))
    return out


@pytest.mark.parametrize("window", [1, 2])
@pytest.mark.parametrize("track", ["decisions", "genie"])
def test_against_the_cpu_loop(device_frames, track, window):
    ref = _reference(device_frames, track, window)
    p = device_frames["p"]
    sw = _sweep(track=track, track_window=window, symbol_counts=True)
    sw.keep_track_xhat = True
    _, counters = sw.run([EBNO], G, chunk_blocks=G)
    got_sym = sw.symbol_error_counts[EBNO]
    want_err = np.sum([r["errors"] for r in ref], axis=0)
    cond = max(float(r["cond"].max()) for r in ref)
    margin = min(r["margin"] for r in ref)
    bound = max(ESN_BOUND, 10 * cond ** 2 * 2.0 ** -52)
    xh = sw.track_xhat.cpu().numpy().reshape(F, G, p.n_sub, p.n_t, 2)
    xh = xh[..., 0] + 1j * xh[..., 1]
    want_x = np.stack([r["x_hat"] for r in ref], axis=1)                # [F, G, N, n_t]
    top = np.abs(want_x).max()
    dev = np.abs(xh - want_x).reshape(F, -1).max(axis=1)
    print(f"{track} window {window}: errors per symbol device {got_sym[:, 0].tolist()} reference {want_err.tolist()}; "
          f"worst cond(E) {cond:.4g}, bound {bound:.2e} of max, margin {margin:.3e}, max |X_hat| {top:.3f}; "
          f"|X_hat - ref| / max per symbol {(dev / top).tolist()}")
    assert margin >= 1e-6, margin
    assert margin >= 10 * bound * top, (margin, bound, top)
    assert dev.max() <= bound * top, (dev / top).tolist()
    assert got_sym[:, 0].tolist() == want_err.tolist()
    assert got_sym[:, 1].tolist() == [G * p.n_sub * p.m * p.n_t] * F
    assert counters[0].tolist() == got_sym.sum(axis=0).tolist()


def test_counters_do_not_depend_on_chunking_or_world_size():
    blocks = 6
    kw = dict(noise=0.001, track="decisions", track_window=2, symbol_counts=True)
    sw = _sweep(**kw)
    _, want = sw.run([EBNO, 12.0], blocks, chunk_blocks=blocks)
    want_sym = {e: sw.symbol_error_counts[e].copy() for e in (EBNO, 12.0)}
    for e, row in zip((EBNO, 12.0), want):
        assert want_sym[e].sum(axis=0).tolist() == row.tolist()         # per-symbol counts sum to the totals
        assert np.all(want_sym[e][:, 1] == blocks * 16 * 2 * 2)
    assert int(want[:, 0].sum()) > 0
    for chunk in (1, 3):
        s2 = _sweep(**kw)
        _, c = s2.run([EBNO, 12.0], blocks, chunk_blocks=chunk)
        assert np.array_equal(c, want), chunk
        for e in want_sym:
            assert np.array_equal(s2.symbol_error_counts[e], want_sym[e]), (chunk, e)
    parts = [_sweep(rank=r, world_size=2, **kw) for r in range(2)]
    cs = [s.run([EBNO, 12.0], blocks, chunk_blocks=2, dist=None)[1] for s in parts]
    assert np.array_equal(cs[0] + cs[1], want)
    for e in want_sym:
        assert np.array_equal(parts[0].symbol_error_counts[e] + parts[1].symbol_error_counts[e], want_sym[e])
    # the totals do not depend on symbol_counts either
    _, c = _sweep(**dict(kw, symbol_counts=False)).run([EBNO, 12.0], blocks, chunk_blocks=4)
    assert np.array_equal(c, want)


@pytest.mark.parametrize("fading", ["block", "jakes"])
def test_track_none_is_the_sweep_without_the_argument(fading):
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep
    p = _params(fading=fading)
    a = DetectorSweep(p, n_reservoir=N_RES, precision="f64", fit_precision="f64", seed=SEED, symbol_counts=True)
    b = _sweep(p, noise=0.001, track=None, symbol_counts=True)
    _, ca = a.run([EBNO], 4, chunk_blocks=3)
    _, cb = b.run([EBNO], 4, chunk_blocks=3)
    assert np.array_equal(ca, cb) and np.array_equal(a.symbol_error_counts[EBNO], b.symbol_error_counts[EBNO])
    assert b.track is None


def test_decisions_and_genie_share_symbol_zero():
    runs = {}
    for track in ("decisions", "genie"):
        sw = _sweep(noise=0.001, track=track, symbol_counts=True)
        sw.run([EBNO], 6, chunk_blocks=4)
        runs[track] = sw.symbol_error_counts[EBNO]
    print({k: v[:, 0].tolist() for k, v in runs.items()})
    assert runs["decisions"][0].tolist() == runs["genie"][0].tolist()
    assert not np.array_equal(runs["decisions"], runs["genie"])


def test_tracking_does_something():
    """2x2, "exp", N = 64, QPSK, N_res = 32, 21 dB, fd_tsym = 0.02 (f_d = 576.9 Hz), 24 data symbols, 64 blocks, float32
    predict, window 2, no state noise.  The NumPy loop put whole-block BER at about 0.05 (genie) / 0.2 (decisions) / 0.33
    (static) over 6 to 16 blocks, so the plain ordering has an absolute margin near 0.1 at 393 216 bits."""
    p = _params(n_sub=64, fd_tsym=0.02, frames=24)
    assert abs(p.f_d - 576.9) < 0.05 and abs(p.fd_tsym - 0.02) < 1e-12
    ber = {}
    for track in (None, "decisions", "genie"):
        sw = _sweep(p, n_res=32, precision="f32", track=track, track_window=2, symbol_counts=True)
        b, c = sw.run([21.0], 64)
        assert int(c[0, 1]) == 64 * 24 * 64 * 2 * 2 == 393216
        ber[track] = float(b[0])
        sc = sw.symbol_error_counts[21.0]
        print(track, "BER per symbol:", np.round(sc[:, 0] / sc[:, 1], 3).tolist())
    print(f"whole-block BER: static {ber[None]:.4f}, decisions {ber['decisions']:.4f}, genie {ber['genie']:.4f}")
    assert ber["genie"] < ber["decisions"] < ber[None]


def test_argument_errors():
    for kw, word in ((dict(track="directed"), "track must be"), (dict(track="genie", track_window=0), "track_window"),
                     (dict(track="decisions", ridge_grid=[1e-3, 1e-2]), "ridge_grid"),
                     (dict(track="decisions", train_ebno=12.0), "train_ebno"),
                     (dict(track="genie", io="f32", precision="f32"), "io='f32'")):
        with pytest.raises(ValueError, match=word):
            _sweep(**kw)
    with pytest.raises(ValueError, match="continuation"):
        _sweep(dataclasses.replace(_params(), continuation=True), track="decisions")
