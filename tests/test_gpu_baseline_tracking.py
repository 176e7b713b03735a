"""baseline_tracking_point (points.py): the LS-MMSE baseline with its channel estimate re-made after every data symbol.

Against the same loop in NumPy, one block at a time, on the device's own frames: oracle.baselines.estimate_channel on the
sparse pilot, oracle.baselines.mmse_detect per data symbol, tests/chantrack_ref.py over the most recent `window` data
symbols (decisions: the reference's own X_hat, sliced; genie: the transmitted bits), the previous H kept where the
estimate is flagged.  2x2, "exp", fading="jakes", QPSK, N = 32, isi = 8, 21 dB, fd_tsym = 0.01, 3 blocks x 6 data
symbols, windows 1 and 2.  Per-symbol error counts exactly equal.

BOUND (the rule of tests/test_gpu_tracking.py).  The device's H differs from the reference's by at most
d_H = max(1e-10, isi max(1e-12, 16 n_t isi cond(G) 2^-52)) of max: 1e-10 is what tests/test_gpu_baseline.py holds the
pilot estimate to, the other term what tests/test_gpu_chantrack.py holds a tracked estimate to.  The detector solves
(H_k^H H_k + No/Pi I) x = H_k^H y per subcarrier, so a relative change d_H of H moves x by about cond_k d_H, cond_k the
condition number of that matrix; with the factor 10 of the tracking test, and 1e-9 of max for the detector itself
(tests/test_gpu_baseline.py): BOUND = max(1e-9, 10 max_k cond_k d_H), computed from the reference's own matrices and
printed.  The reference's smallest distance of X_hat to a decision boundary must be at least 1e-6 and a decade above
BOUND max |X_hat| (the seed is chosen for that); every symbol's X_hat is then within BOUND of max and the counts equal.

Invariance: counters are bit-identical for chunk_blocks in {1, 3, all} and for first_block splits summed.  track=None
equals mmse_detect_count on the pilot estimate, per symbol.  Decisions and genie agree on data symbol 0.  And tracking
does something: at 2x2, N = 64, QPSK, 21 dB, fd_tsym = 0.02, 16 blocks x 24 symbols, window 1, the block-mean BER orders
genie < decisions < static (a NumPy chain over 12 such blocks gave 0.0145 / 0.071 / 0.347)."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chantrack_ref as cr  # noqa: E402
import remod_ref  # noqa: E402
from tracking_ref import boundary_margin  # noqa: E402
from oracle import baselines  # noqa: E402
from oracle import esn_oracle as eo  # noqa: E402
from oracle.ofdm_frames import LinkConfig  # noqa: E402

pytestmark = pytest.mark.gpu

G, F, EBNO, SEED = 3, 6, 21.0, 5
FD_TSYM = 0.01
EPS = 2.0 ** -52


def _params(n_sub=32, fd_tsym=FD_TSYM, frames=F):
    from esn_ofdm_mimo_amd.montecarlo import LinkParams
    p = dataclasses.replace(LinkParams.block_fading(2, 2, n_sub=n_sub), m=2)
    return dataclasses.replace(p, coherence_fixed=frames, f_d=fd_tsym * p.fs / (p.n_sub + p.cp), fading="jakes")


def _source(params=None, seed=SEED):
    from esn_ofdm_mimo_amd.montecarlo import FrameSource
    return FrameSource(params or _params(), seed=seed)


@pytest.fixture(scope="module")
def device_frames():
    """what baseline_tracking_point generates for blocks 0 .. G - 1 at Eb/No index 0, on the host"""
    src = _source()
    d = src.blocks_fast(EBNO, 0, 0, G, F, with_ls_pilot=True)
    p = src.p
    host = {k: d[k].cpu().numpy() for k in ("pilot_bits", "pilot_y_ls", "data_y", "data_bits")}
    for k in ("data_y", "data_bits"):
        host[k] = host[k].reshape(G, F, *host[k].shape[1:])
    host["p"] = p
    return host


def _track_block(p, pilot_bits, pilot_y_ls, data_y, data_bits, track, window):
    """one block of the loop in NumPy: dict(errors [F], x_hat [F, N, n_t], cond_g: worst cond(G) of the tracked
    estimates, cond_k: worst cond of a detector matrix, failed)"""
    cfg = LinkConfig(n_t=p.n_t, n_r=p.n_r, n_sub=p.n_sub, m=p.m, isi=p.isi, fs=p.fs, no=p.no, clip_db=p.clip_db)
    const = eo.unit_qam(p.m)
    idx = cr.bits_to_indices(pilot_bits[None], p.m)[0]
    x_ls = np.zeros((p.n_sub, p.n_t), dtype=np.complex128)
    for tx in range(p.n_t):
        x_ls[tx::p.n_t, tx] = const[idx[tx::p.n_t, tx]]
    H = baselines.estimate_channel(cfg, EBNO, x_ls, pilot_y_ls)
    p_i = p.p_i(EBNO)
    reg = cr.map_reg(p.n_sub, p.cp, p.isi, p.no, p_i)
    lam = p.no / p_i
    errors, x_hats, cond_g, cond_k, failed = [], [], 1.0, 1.0, 0
    for k in range(F):
        x_hat = baselines.mmse_detect(cfg, EBNO, H, data_y[k])
        cond_k = max(cond_k, max(np.linalg.cond(h.conj().T @ h + lam * np.eye(p.n_t)) for h in H))
        got = remod_ref.index_bits(remod_ref.slice_indices(x_hat, p.m)[None], p.m)[0]
        errors.append(int((got != data_bits[k]).sum()))
        x_hats.append(x_hat)
        if k == F - 1:
            break
        ws = min(window, k + 1)
        kw = dict(X_hat=np.stack(x_hats[-ws:])) if track == "decisions" else dict(bits=data_bits[k + 1 - ws:k + 1])
        est = cr.channel_track(data_y[k + 1 - ws:k + 1], ws, 1, p.cp, p.n_t, p.isi, p.m, [p_i], reg[None], **kw)
        if est["status"][0] == 0:
            H = est["H"][0]
            cond_g = max(cond_g, float(est["cond"][0]))
        else:
            failed += 1
    return dict(errors=np.array(errors), x_hat=np.stack(x_hats), cond_g=cond_g, cond_k=cond_k, failed=failed)


@pytest.mark.parametrize("window", [1, 2])
@pytest.mark.parametrize("track", ["decisions", "genie"])
def test_against_the_numpy_loop(device_frames, track, window):
    from esn_ofdm_mimo_amd.montecarlo import baseline_tracking_point
    h, p = device_frames, device_frames["p"]
    ref = [_track_block(p, h["pilot_bits"][b], h["pilot_y_ls"][b], h["data_y"][b], h["data_bits"][b], track, window)
           for b in range(G)]
    out = baseline_tracking_point(_source(), EBNO, 0, G, F, track=track, window=window, want_xhat=True)
    want_err = np.sum([r["errors"] for r in ref], axis=0)
    want_x = np.stack([r["x_hat"] for r in ref], axis=1)                # [F, G, N, n_t]
    cond_g, cond_k = max(r["cond_g"] for r in ref), max(r["cond_k"] for r in ref)
    d_h = max(1e-10, p.isi * max(1e-12, 16 * p.n_t * p.isi * cond_g * EPS))
    bound = max(1e-9, 10 * cond_k * d_h)
    margin, top = boundary_margin(want_x, p.m), np.abs(want_x).max()
    dev = np.abs(out["x_hat"].cpu().numpy() - want_x).reshape(F, -1).max(axis=1)
    print(f"{track} window {window}: errors per symbol device {out['errors'].tolist()} reference {want_err.tolist()}; "
          f"worst cond(G) {cond_g:.4g}, worst detector cond {cond_k:.4g}, bound {bound:.2e} of max, margin {margin:.3e}, "
          f"max |X_hat| {top:.3f}; |X_hat - ref| / max per symbol {(dev / top).tolist()}; flagged {out['failed']}")
    assert margin >= 1e-6, margin
    assert margin >= 10 * bound * top, (margin, bound, top)
    assert dev.max() <= bound * top, (dev / top).tolist()
    assert out["errors"].tolist() == want_err.tolist()
    assert out["bits"].tolist() == [G * p.n_sub * p.m * p.n_t] * F
    assert out["failed"] == sum(r["failed"] for r in ref)
    assert out["ber"] == want_err.sum() / out["bits"].sum()


def test_counters_do_not_depend_on_chunking_or_on_the_split():
    from esn_ofdm_mimo_amd.montecarlo import baseline_tracking_point
    blocks = 6
    kw = dict(track="decisions", window=2)
    want = baseline_tracking_point(_source(), EBNO, 0, blocks, F, **kw)
    assert int(want["errors"].sum()) > 0 and want["bits"].tolist() == [blocks * 32 * 2 * 2] * F
    for chunk in (1, 3):
        got = baseline_tracking_point(_source(), EBNO, 0, blocks, F, chunk_blocks=chunk, **kw)
        assert np.array_equal(got["errors"], want["errors"]) and np.array_equal(got["bits"], want["bits"]), chunk
        assert got["failed"] == want["failed"]
    parts = [baseline_tracking_point(_source(), EBNO, 0, n, F, first_block=b0, chunk_blocks=2, **kw)
             for b0, n in ((0, 2), (2, 4))]
    assert np.array_equal(parts[0]["errors"] + parts[1]["errors"], want["errors"])
    assert np.array_equal(parts[0]["bits"] + parts[1]["bits"], want["bits"])


def test_track_none_counts_against_the_pilot_estimate():
    from esn_ofdm_mimo_amd.montecarlo import baseline_tracking_point
    src = _source()
    blocks = 4
    out = baseline_tracking_point(src, EBNO, 0, blocks, F, chunk_blocks=3)
    d = src.blocks_fast(EBNO, 0, 0, blocks, F, with_ls_pilot=True)
    H = src.estimate_channel(d["pilot_bits"], d["pilot_y_ls"], EBNO)
    e, nb = src.mmse_detect_count(H, d["data_y"], d["data_bits"], F, EBNO)         # one H per block of F frames
    assert int(out["errors"].sum()) == int(e.sum()) and int(out["bits"].sum()) == int(nb.sum())
    e1, nb1 = src.mmse_detect_count(H.repeat_interleave(F, dim=0), d["data_y"], d["data_bits"], 1, EBNO)
    assert out["errors"].tolist() == e1.view(blocks, F).sum(dim=0).cpu().tolist()
    assert out["bits"].tolist() == nb1.view(blocks, F).sum(dim=0).cpu().tolist()
    assert out["failed"] == 0 and "x_hat" not in out


def test_decisions_and_genie_share_symbol_zero():
    from esn_ofdm_mimo_amd.montecarlo import baseline_tracking_point
    runs = {t: baseline_tracking_point(_source(), EBNO, 0, 6, F, track=t, chunk_blocks=4) for t in (None, "decisions", "genie")}
    print({k: v["errors"].tolist() for k, v in runs.items()})
    assert runs["decisions"]["errors"][0] == runs["genie"]["errors"][0] == runs[None]["errors"][0]
    assert not np.array_equal(runs["decisions"]["errors"], runs[None]["errors"])


def test_tracking_does_something():
    from esn_ofdm_mimo_amd.montecarlo import baseline_tracking_point
    p = _params(n_sub=64, fd_tsym=0.02, frames=24)
    assert abs(p.fd_tsym - 0.02) < 1e-12
    ber = {}
    for track in (None, "decisions", "genie"):
        out = baseline_tracking_point(_source(p), 21.0, 0, 16, 24, track=track, window=1)
        assert int(out["bits"].sum()) == 16 * 24 * 64 * 2 * 2
        ber[track] = out["ber"]
        print(track, "BER per symbol:", np.round(out["errors"] / out["bits"], 3).tolist(), "flagged", out["failed"])
    print(f"block-mean BER: static {ber[None]:.4f}, decisions {ber['decisions']:.4f}, genie {ber['genie']:.4f}")
    assert ber["genie"] < ber["decisions"] < ber[None]
