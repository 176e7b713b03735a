"""The two coded comparison points of the Monte-Carlo harness, one Eb/No point each, batched on the device: the 4x8
driver's coded + uncoded ESN against LS/MMSE (coded_ber_point) and the block-fading drivers' five detectors
(block_fading_point).  Both send LDPC-coded payloads through the frames of a DetectorSweep's FrameSource and train
through the sweep's bank as it stands; frames and ESN legs stay float64 / complex128 whatever the sweep's io says.
Beside them baseline_tracking_point: the LS-MMSE baseline of one Eb/No point, uncoded, detected symbol by symbol with its
channel estimate re-made after every data symbol (what DetectorSweep(track=...) is to the ESN); it needs a FrameSource
only.  And elm_point / fnn_point / cnn_point / lstm_point: the windowed ELM (elm.py), FNN (fnn.py) and CNN (cnn.py) and
the LSTM (lstm.py), the reference's pinv-trained and Adam-trained comparators, on the same frames; ensemble_point, K
small ESNs averaged before the FFT; and equalized_esn_point, a small ESN behind the LS-MMSE equaliser.  The uncoded points
share _check_block_args, _check_esn_point_args, _chunks and _retry_with_qr here, frames.pilot_rows / group_scalings
and, with DetectorSweep, sweep.reservoir_seed / host_reservoirs / host_reservoir_bank / fit_e_dtype."""
from __future__ import annotations

import numpy as np

from . import reservoirs as _reservoirs
from .batched import ReservoirBank
from .frames import _view_real, group_scalings, pilot_rows, summarize_channel_metrics
from .readout import _lambdas
from .sweep import (DetectorSweep, check_io, fit_e_dtype, host_reservoir_bank, host_reservoirs, reservoir_seed,
                    stream_seed)


def _check_block_args(n_blocks, first_block, chunk_blocks, frames_per_block):
    """What every uncoded point refuses of its block range."""
    if int(n_blocks) < 1 or int(first_block) < 0:
        raise ValueError(f"n_blocks = {n_blocks} must be positive and first_block = {first_block} non-negative")
    if chunk_blocks is not None and int(chunk_blocks) < 1:
        raise ValueError(f"chunk_blocks = {chunk_blocks} must be positive")
    if frames_per_block is not None and int(frames_per_block) < 1:
        raise ValueError(f"frames_per_block = {frames_per_block} must be positive")


def _check_esn_point_args(method, io, precision, ridge, ridge_grid=None):
    """What the points that fit a reservoir's read-out refuse alike."""
    if method not in ("auto", "qr", "chol"):
        raise ValueError(f"method must be 'auto', 'qr' or 'chol', not {method!r}")
    check_io(io, precision)
    if ridge is not None and ridge_grid is not None:
        raise ValueError("give ridge or ridge_grid, not both")
    if ridge is not None and not float(ridge) >= 0:
        raise ValueError(f"ridge = {ridge} must be None or non-negative")


def _chunks(first_block, n_blocks, chunk):
    """The chunks of blocks first_block .. first_block + n_blocks - 1, at most `chunk` blocks each: yields (b0, g, lo) --
    the chunk's first global block, its length, and where its counters start in a point's [n_blocks] vectors."""
    first_block, end = int(first_block), int(first_block) + int(n_blocks)
    for b0 in range(first_block, end, chunk):
        yield b0, min(chunk, end - b0), b0 - first_block


def _retry_with_qr(body, method):
    """The result of body(method), a point's chunk loop, which returns (result, flagged fits); a point with a flagged fit
    is redone as a whole, once, with method "qr".  int(flagged) is the point's one host read."""
    result, flagged = body(method)
    if method != "qr" and int(flagged) != 0:
        result, flagged = body("qr")
    return result


def _coded_block_data(src, code, ebno_db, snr_idx, G, F, seed, salt):
    """The coded data of G blocks with F data frames each out of the FrameSource src: info bits u [G F, n_t, k] from a
    generator keyed by (seed, snr_idx, salt), their code words tx_bits [G F, N m, n_t], the blocks' taps, the pilot
    (bits, x, y), the LS-pattern pilot and the data frames that carry tx_bits."""
    torch, p = src.torch, src.p
    gen = torch.Generator(device=src.device)
    gen.manual_seed((seed * 1000003 + snr_idx * 7919 + salt) % (2 ** 63 - 1))
    u = torch.randint(0, 2, (G * F, p.n_t, code.k), generator=gen, device=src.device, dtype=torch.uint8)
    tx_bits = code.encode(u, p.n_t)
    taps = src.taps(G, snr_idx, 0)
    pilot = src.frames(taps, 1, ebno_db, snr_idx, 0, 0, want_x=True)
    _, _, py_ls = src.frames(taps, 1, ebno_db, snr_idx, 0, 0, ls_pattern=True)
    _, _, dy = src.frames(taps, F, ebno_db, snr_idx, 0, 1, bits_in=tx_bits)
    return u, tx_bits, taps, pilot, py_ls, dy


def _esn_leg(sweep, ebno_db, pilot_y, pilot_x, data_y, tx_bits, F, snr_idx, seed, scale_ebno=None):
    """The ESN of `sweep` on one point's blocks: train on the pilots (input scaling of scale_ebno, if given), repair,
    predict and detect the data frames.  Returns (errors [G], bits [G]) and X_hat complex [G F, N, n_t]."""
    torch, p, G = sweep.torch, sweep.p, pilot_y.shape[0]
    sweep.set_snr(ebno_db, G, scale_ebno=scale_ebno)
    E = sweep.train(pilot_y, pilot_x, seed=sweep.stream_seed(snr_idx, 0) + seed)
    sweep.repair_fit(E)
    y = sweep.bank.predict(_view_real(data_y), F, T=p.t_frame + p.delay, transient=p.forget,
                           precision=sweep.precision, noise_mode="counter", seed=sweep.stream_seed(snr_idx, 1) + seed)
    e, nb, xh = sweep.bank.detect_count(y, tx_bits, sweep.p_i, F, p.n_sub, p.n_t, p.m, want_xhat=True)
    return (e, nb), torch.view_as_complex(xh.view(G * F, p.n_sub, p.n_t, 2).contiguous())


def baseline_tracking_point(src, ebno_db, snr_idx, n_blocks, frames_per_block=None, track=None, window=1, first_block=0,
                            chunk_blocks=None, zf=False, want_xhat=False):
    """One Eb/No point of the LS-MMSE baseline with its channel estimate tracked through the block, on the frames a
    DetectorSweep over the same FrameSource seed detects (blocks_fast with the sweep's keys): per chunk the pilot
    estimate H (esn_channel_estimate on the sparse LS pilot), then data symbol k of all blocks at once through
    mmse_detect_count with one H per frame and, unless k is the last, a new H from FrameSource.track_channel over the
    most recent `window` data symbols -- track="decisions": the detector's own X_hat, sliced; "genie": the transmitted
    bits, the bound.  The pilot is not part of the window.  An estimate the kernel flags keeps the block's previous H.
    track=None: every symbol against the pilot estimate, what tools/doppler_sweep.py counts.  zf=True: the zero-forcing
    detector in place of MMSE.  Returns dict(errors int64 [F], bits int64 [F] per data symbol, ber, failed = flagged
    estimates); counters stay on the device until the end.  want_xhat is test support, not part of a sweep: on a tracked
    run it adds `x_hat` complex [F, n_blocks, N, n_t], the detector's output on every data symbol, and keeps all of those
    tensors alive until the end -- tests/test_gpu_baseline_tracking.py holds it against the NumPy loop; leave it False
    at any size that matters."""
    if track not in (None, "decisions", "genie"):
        raise ValueError(f"track must be None, 'decisions' or 'genie', not {track!r}")
    if not isinstance(window, int) or not 1 <= window <= 8:
        raise ValueError(f"window must be an integer in 1..8, not {window!r}")
    _check_block_args(n_blocks, first_block, chunk_blocks, frames_per_block)
    torch, p = src.torch, src.p
    F, chunk = int(frames_per_block or p.coherence_symbols), int(chunk_blocks or n_blocks)
    errors, nbits = (torch.zeros(F, dtype=torch.int64, device=src.device) for _ in range(2))
    failed = torch.zeros((), dtype=torch.int64, device=src.device)
    kept = []
    for b0, g, _ in _chunks(first_block, n_blocks, chunk):
        d = src.blocks_fast(ebno_db, snr_idx, b0, g, F, with_ls_pilot=True)
        H = src.estimate_channel(d["pilot_bits"], d["pilot_y_ls"], ebno_db)
        if track is None:
            e, nb = src.mmse_detect_count(H.repeat_interleave(F, dim=0), d["data_y"], d["data_bits"], 1, ebno_db, zf=zf)
            errors += e.view(g, F).sum(dim=0)
            nbits += nb.view(g, F).sum(dim=0)
            continue
        dy = d["data_y"].view(g, F, p.t_frame, p.n_r)
        db = d["data_bits"].view(g, F, p.n_sub * p.m, p.n_t)
        decided = []                                                  # X_hat of the most recent `window` symbols
        kept.append([])
        for k in range(F):
            e, nb, xh = src.mmse_detect_count(H, dy[:, k].contiguous(), db[:, k].contiguous(), 1, ebno_db,
                                              want_xhat=True, zf=zf)
            errors[k] += e.sum()
            nbits[k] += nb.sum()
            if want_xhat:
                kept[-1].append(xh)
            if k == F - 1:
                break
            decided = (decided + [xh])[-window:]
            ws = min(window, k + 1)
            y_win = dy[:, k + 1 - ws:k + 1].reshape(g * ws, p.t_frame, p.n_r)
            if track == "decisions":
                Hn, st = src.track_channel(y_win, ebno_db, X_hat=torch.stack(decided, dim=1).reshape(g * ws, p.n_sub, p.n_t),
                                           window=ws)
            else:
                Hn, st = src.track_channel(y_win, ebno_db, bits=db[:, k + 1 - ws:k + 1].reshape(g * ws, -1, p.n_t),
                                           window=ws)
            bad = st != 0
            failed += bad.sum()
            H = torch.where(bad[:, None, None, None], H, Hn)
    errors, nbits = errors.cpu().numpy(), nbits.cpu().numpy()
    out = dict(errors=errors, bits=nbits, ber=float(errors.sum()) / float(nbits.sum()), failed=int(failed))
    if want_xhat and kept:
        out["x_hat"] = torch.cat([torch.stack(c) for c in kept], dim=1)
    return out


def coded_ber_point(sweep, code, ebno_db, snr_idx, n_blocks, frames_per_block=None, cal_frac=0.3, seed=0):
    """One Eb/No point of the reference's coded + uncoded comparison, batched on the device
    (Demo_MIMO_4x8_Sionna_CDL_ESN_v2.py:283-530): LDPC-coded payloads on every data symbol, ESN and
    LS/MMSE detection, max-log LLRs, logistic LLR calibration fitted on the first `cal_frac` of the
    blocks (the reference: the first 30 % of the symbols, :266,:476-482,:513-523) and sum-product
    decoding of the rest.  Returns dict(ESN_uncoded, MMSE_uncoded, ESN_coded, MMSE_coded, a_esn, ...).
    Frames and the ESN leg stay float64 / complex128 whatever sweep.io says: the MMSE leg reads complex128."""
    sweep._require_block_independent_bank("coded_ber_point")
    sweep._require_block_fading("coded_ber_point")
    p, src = sweep.p, sweep.src
    F, G = frames_per_block or p.coherence_symbols, n_blocks
    u, tx_bits, _, (pbits, px, py), py_ls, dy = _coded_block_data(src, code, ebno_db, snr_idx, G, F, seed, 12345)
    (e_esn, n_esn), x_esn = _esn_leg(sweep, ebno_db, py, px, dy, tx_bits, F, snr_idx, seed)
    # LS/MMSE baseline
    H = src.estimate_channel(pbits, py_ls, ebno_db)
    e_mm, n_mm, x_mm = src.mmse_detect_count(H, dy, tx_bits, F, ebno_db, want_xhat=True)
    out = dict(ESN_uncoded=float(e_esn.sum()) / float(n_esn.sum()), MMSE_uncoded=float(e_mm.sum()) / float(n_mm.sum()))
    n_cal = max(1, int(round(cal_frac * G))) * F                             # frames used for calibration
    for name, xhat in (("ESN", x_esn), ("MMSE", x_mm)):
        _calibrated_leg(out, name, code, code.llrs(xhat, p.m)[0], tx_bits, u, n_cal, p.n_t * F, p.m)
    return out


def _calibrated_leg(out, name, code, llr, tx_bits, u, n_cal, cw_per_group, m):
    """The coded BER of one detector into out[name + "_coded"], with its calibration out["a_" / "b_" + name.lower()]:
    fit_calibration on the first n_cal frames of llr [B, n_t, N m], decode_count on the rest."""
    a, b = code.fit_calibration(llr[:n_cal], tx_bits[:n_cal], m)
    err, nb = code.decode_count(llr[n_cal:].contiguous(), a, b, u[n_cal:], cw_per_group, m)
    out[name + "_coded"] = float(err.sum()) / max(float(nb.sum()), 1.0)
    out["a_" + name.lower()] = a.cpu().numpy()
    out["b_" + name.lower()] = b.cpu().numpy()


def block_fading_point(sweep, code, ebno_db, snr_idx, n_blocks, fixed_sweep=None, decode_every=4, llr_scale=1.5,
                       seed=0, channel_metrics=False):
    """One Eb/No point of the block-fading drivers' comparison (OFDM_{SISO,SIMO_1-2,MIMO_2-2}_NBF_LDPC.py /
    Demo_MIMO_4x8_ChannelRank_..._fast.py :266-521), batched on the device: per coherence block one pilot and
    L - 1 LDPC-coded data symbols (the pilot symbol carries no data here, :387); detectors ESN (SNR-matched),
    ESN trained at a fixed Eb/No (`fixed_sweep`: a DetectorSweep built with train_ebno=12), LS-ZF,
    MMSE and Perfect-ZF (:450-460); uncoded BER over every data symbol, coded BER on every `decode_every`-th
    symbol of the run (kk % 4 == 1, :202,389) with the drivers' uncalibrated LLRs: per-stream decision-directed
    sigma^2, x LLR_SCALE 1.5, clip +-20 (:478-485).  Returns the reference's holder names (BER_* / BERC_*).
    channel_metrics=True adds the drivers' channel record of this Eb/No point (:369-385,515-521) as plain floats:
    capacity_bits_per_sc, frac_rank_ge_full, cond_p50, cond_p90 (FrameSource.channel_metrics on H_true).
    Frames and the ESN legs stay float64 / complex128 whatever the sweeps' io says: the LS / MMSE / ZF legs read
    complex128."""
    sweep._require_block_independent_bank("block_fading_point")
    sweep._require_block_fading("block_fading_point")
    if fixed_sweep is not None:
        fixed_sweep._require_block_independent_bank("block_fading_point")
    torch, p, src = sweep.torch, sweep.p, sweep.src
    L = p.coherence_symbols
    F, G = L - 1, n_blocks
    u, tx_bits, taps, (pbits, px, py), py_ls, dy = _coded_block_data(src, code, ebno_db, snr_idx, G, F, seed, 4242)
    xhat = {}
    err = {}
    err["ESN_matched"], xhat["ESN_matched"] = _esn_leg(sweep, ebno_db, py, px, dy, tx_bits, F, snr_idx, seed)
    if fixed_sweep is not None:
        t_eb = fixed_sweep.train_ebno
        _, px_f, py_f = src.frames(taps, 1, t_eb, snr_idx, 0, 0, want_x=True)     # same pilot bits at the fixed power
        err["ESN_trainFixed"], xhat["ESN_trainFixed"] = _esn_leg(fixed_sweep, ebno_db, py_f, px_f, dy, tx_bits, F,
                                                                 snr_idx, seed, scale_ebno=t_eb)
    H_ls = src.estimate_channel(pbits, py_ls, ebno_db, ls_only=True)
    H_mmse = src.estimate_channel(pbits, py_ls, ebno_db)
    H_true = src.true_channel(taps)
    for name, H, zf in (("LS_ZF", H_ls, True), ("MMSE", H_mmse, False), ("PerfectZF", H_true, True)):
        e, nb, xh = src.mmse_detect_count(H, dy, tx_bits, F, ebno_db, want_xhat=True, zf=zf)
        xhat[name], err[name] = xh, (e, nb)
    out = {"BER_" + k: float(v[0].sum()) / float(v[1].sum()) for k, v in err.items()}
    # coded leg: symbol kk (1-based over the run; block b holds kk = L b + 1 (pilot) .. L b + L) decodes iff kk % every == 1
    kk = (torch.arange(G, device=sweep.device)[:, None] * L + 2 + torch.arange(F, device=sweep.device)[None, :]).reshape(-1)
    sel = torch.nonzero((kk % decode_every) == 1).flatten()
    a = torch.full((p.m,), -float(llr_scale), dtype=torch.float64, device=sweep.device)   # -(a llr + b) = scale * llr
    b = torch.zeros(p.m, dtype=torch.float64, device=sweep.device)
    for name, xh in xhat.items():
        xs = xh[sel]                                                           # [S, N, n_t]
        per_stream = xs.permute(0, 2, 1).reshape(-1, p.n_sub, 1).contiguous()  # sigma^2 per (frame, tx) column (:479)
        llr, _ = code.llrs(per_stream, p.m)                                    # [S n_t, 1, N m]
        e, nb = code.decode_count(llr.view(xs.shape[0], p.n_t, -1), a, b, u[sel], max(1, xs.shape[0] * p.n_t), p.m)
        out["BERC_" + name] = float(e.sum()) / max(float(nb.sum()), 1.0)
    out["decoded_symbols"] = int(sel.numel())
    if channel_metrics:
        out.update(summarize_channel_metrics(*src.channel_metrics(H_true, ebno_db), p.n_t, p.n_r))
    return out


def _check_windowed_point_args(slice, weights, precision, window, n_blocks, first_block, chunk_blocks, frames_per_block):
    """What the comparator points refuse alike, from the arguments alone."""
    if slice not in ("aligned", "reference"):
        raise ValueError(f"slice must be 'aligned' or 'reference', not {slice!r}")
    if weights not in ("shared", "per_block"):
        raise ValueError(f"weights must be 'shared' or 'per_block', not {weights!r}")
    if precision not in ("f64", "f16"):
        raise ValueError(f"precision must be 'f64' or 'f16', not {precision!r}")
    if not isinstance(window, int) or not 1 <= window <= 16:
        raise ValueError(f"window must be an integer in 1..16, not {window!r}")
    _check_block_args(n_blocks, first_block, chunk_blocks, frames_per_block)


def _windowed_point(src, ebno_db, snr_idx, n_blocks, first_block, frames_per_block, chunk_blocks, precision, slice, train):
    """The chunk loop of the comparator points over blocks first_block .. first_block + n_blocks - 1: per chunk of g
    blocks from b0 on, blocks_fast, the pilots as U [g, T, 2 n_r] and D [g, T, 2 n_t] (T = t_frame + delay, the teacher
    delayed), train(U, D, scaling, b0, g) -- which returns a windowed.WindowedBank trained on them under
    set_scaling(*scaling), inputs and teacher scaled by 1 / sqrt(var_x) -- then one predict over the chunk's data
    frames, cut as `slice` says, and the detector tail into that chunk's part of the counters.  Returns (errors, bits):
    int64 [n_blocks] on the device; nothing is read back."""
    torch, p = src.torch, src.p
    n_in, n_out, T = 2 * p.n_r, 2 * p.n_t, p.t_frame + p.delay
    F, n_blocks = int(frames_per_block or p.coherence_symbols), int(n_blocks)
    chunk = int(chunk_blocks or min(n_blocks, 4096))
    errors, nbits = (torch.zeros(n_blocks, dtype=torch.int64, device=src.device) for _ in range(2))
    scale = 1.0 / np.sqrt(p.var_x(ebno_db))
    for b0, g, lo in _chunks(first_block, n_blocks, chunk):
        data = src.blocks_fast(ebno_db, snr_idx, b0, g, F)
        U, D = pilot_rows(data["pilot_y"], data["pilot_x"], p.delay)
        bank = train(U, D, group_scalings(g, n_in, scale, n_out, scale, src.device), b0, g)
        dy = _view_real(data["data_y"])
        if slice == "aligned":
            Y = bank.predict(dy, F, T=T, transient=p.forget, precision=precision)
        else:
            Y = bank.predict(dy, F, T=T, transient=0, precision=precision)[:, :p.n_sub].contiguous()
        bank.detect_count(Y, data["data_bits"], src.p_i(ebno_db, g), F, p.n_sub, p.n_t, p.m,
                          err=errors[lo:lo + g], bits=nbits[lo:lo + g])
    return errors, nbits


def _stack_sets(sets):
    """Per-block parameter sets, each a tuple of arrays -> one tuple of arrays [len(sets), ...]."""
    return tuple(np.stack(a) for a in zip(*sets))


def _trained_point(src, ebno_db, snr_idx, n_blocks, shape_error, make_bank, draw, transient, *, epochs, lr, precision,
                   slice, weights, first_block, frames_per_block, chunk_blocks):
    """_windowed_point for an Adam-trained comparator (a trained.TrainedBank), after the checks fnn_point, cnn_point and
    lstm_point share: shape_error(T) says why the training kernel does not serve the link's shape (or None),
    make_bank(n_groups) builds the bank, draw(None) is the shared initial set and draw(block) the one of a global block
    (stacked per array over a chunk's blocks); every chunk is trained from them over rows [transient, T) by `epochs` Adam
    steps of size lr and predicted at `precision`."""
    if not isinstance(epochs, int) or epochs < 1:
        raise ValueError(f"epochs must be a positive integer, not {epochs!r}")
    if not lr >= 0:
        raise ValueError(f"lr = {lr} must be non-negative")
    why = shape_error(src.p.t_frame + src.p.delay)
    if why:
        raise ValueError("the training kernel does not serve this shape: " + why)
    shared = draw(None) if weights == "shared" else None
    bank = make_bank(min(int(chunk_blocks or 4096), int(n_blocks)))

    def train(U, D, scaling, b0, g):
        init = shared if shared is not None else _stack_sets([draw(b0 + i) for i in range(g)])
        bank.set_scaling(*scaling)
        return bank.train(U, D, init, transient=transient, epochs=epochs, lr=lr)

    return _windowed_point(src, ebno_db, snr_idx, n_blocks, first_block, frames_per_block, chunk_blocks, precision, slice,
                           train)


def elm_weights(n_hidden, k, gain, seed, block=None):
    """W_in = gain U(-1, 1) [n_hidden, k], then b = U(-1, 1) [n_hidden], from RandomState(seed) -- or, for the set of
    one global block, RandomState([seed, block])."""
    rs = np.random.RandomState(seed if block is None else [seed, block])
    return gain * rs.uniform(-1, 1, (n_hidden, k)), rs.uniform(-1, 1, n_hidden)


def elm_point(src, ebno_db, snr_idx, n_blocks, *, n_hidden=512, window=8, gain=0.05, ridge=None, method="auto",
              precision="f64", slice="aligned", weights="shared", first_block=0, seed=0, frames_per_block=None,
              chunk_blocks=None):
    """One Eb/No point of the windowed ELM (elm.ElmBank), the reference's pinv-trained comparator, on the frames a
    DetectorSweep over the same FrameSource seed detects (blocks_fast with the sweep's keys, as baseline_tracking_point):
    per chunk the pilot of every block gives one fit (inputs and teacher scaled by 1 / sqrt(var_x), transient
    max(delay + cp, window - 1), pinv or `ridge`), then all data frames are predicted in one launch and counted by the
    detector tail.  slice "aligned": the tail reads rows [delay + cp, + N) of the output; "reference": rows [0, N) of
    the un-cut output, the slice the reference's ELM / FNN branches take (system_model_2_all_comparision.py:151-152,
    :570-571), delay + cp rows early.  weights "shared": one (W_in, b) = elm_weights(seed); "per_block": one per global
    block.  Returns (errors, bits): int64 [n_blocks] on the device; nothing is read back inside the chunk loop (a fit
    the Cholesky solve flags has the whole point redone with method="qr" after it)."""
    _check_windowed_point_args(slice, weights, precision, window, n_blocks, first_block, chunk_blocks, frames_per_block)
    if method not in ("auto", "qr", "chol"):
        raise ValueError(f"method must be 'auto', 'qr' or 'chol', not {method!r}")
    if not isinstance(n_hidden, int) or not 1 <= n_hidden <= 1024:
        raise ValueError(f"n_hidden must be an integer in 1..1024, not {n_hidden!r}")
    if not gain > 0:
        raise ValueError(f"gain = {gain} must be positive")
    if ridge is not None and not float(ridge) >= 0:
        raise ValueError(f"ridge = {ridge} must be None or non-negative")
    from .elm import ElmBank
    p = src.p
    n_in, n_out = 2 * p.n_r, 2 * p.n_t
    k, transient = window * n_in, max(p.forget, window - 1)
    if k > 256:
        raise ValueError(f"window * 2 n_r = {k}: the ELM kernels serve up to 256")
    shared = elm_weights(n_hidden, k, gain, seed) if weights == "shared" else None

    def point(method):
        bank = None
        flagged = src.torch.zeros((), dtype=src.torch.int64, device=src.device)

        def train(U, D, scaling, b0, g):
            nonlocal bank
            if shared is None:
                W_in, b = _stack_sets([elm_weights(n_hidden, k, gain, seed, b0 + i) for i in range(g)])
            else:
                W_in, b = shared
            if bank is None:
                bank = ElmBank(n_in, n_out, n_hidden, window, W_in, b, n_groups=g, device=src.device)
            elif shared is None:
                bank.set_weights(W_in, b)
            bank.set_scaling(*scaling)
            bank.fit(U, D, transient=transient, method=method, ridge=ridge, repair=False)
            flagged.add_(bank.fit_status.ne(0).sum())
            return bank

        return _windowed_point(src, ebno_db, snr_idx, n_blocks, first_block, frames_per_block, chunk_blocks, precision,
                               slice, train), flagged

    return _retry_with_qr(point, method)


def fnn_weights(n_hidden, k, n_out, seed, block=None):
    """(W1 [n_hidden, k], b1, W2 [n_out, n_hidden], b2), each U(+-1 / sqrt(fan_in)) -- the distribution of
    torch.nn.Linear -- drawn in that order from RandomState(seed) or, for the set of one global block,
    RandomState([seed, block])."""
    rs = np.random.RandomState(seed if block is None else [seed, block])
    a1, a2 = 1.0 / np.sqrt(k), 1.0 / np.sqrt(n_hidden)
    return (rs.uniform(-a1, a1, (n_hidden, k)), rs.uniform(-a1, a1, n_hidden),
            rs.uniform(-a2, a2, (n_out, n_hidden)), rs.uniform(-a2, a2, n_out))


def fnn_point(src, ebno_db, snr_idx, n_blocks, *, n_hidden=100, window=8, epochs=50, lr=0.01, precision="f64",
              slice="aligned", weights="shared", first_block=0, seed=0, frames_per_block=None, chunk_blocks=None):
    """One Eb/No point of the windowed FNN (fnn.FnnBank), the reference's Adam-trained comparator, on the frames
    elm_point and a DetectorSweep over the same FrameSource seed detect: per chunk the pilot of every block gives one
    training (inputs and teacher scaled by 1 / sqrt(var_x), transient max(delay + cp, window - 1), `epochs` Adam steps
    from fnn_weights), then all data frames are predicted in one launch and counted by the detector tail.  slice and
    weights as in elm_point ("reference": rows [0, N) of the un-cut output, the slice the reference's FNN branch
    takes).  precision is the prediction's; the training is float64.  Returns (errors, bits): int64 [n_blocks] on the
    device; nothing is read back inside the chunk loop."""
    _check_windowed_point_args(slice, weights, precision, window, n_blocks, first_block, chunk_blocks, frames_per_block)
    if not isinstance(n_hidden, int) or n_hidden < 1:
        raise ValueError(f"n_hidden must be a positive integer, not {n_hidden!r}")
    from .fnn import FnnBank, train_shape_error
    n_in, n_out = 2 * src.p.n_r, 2 * src.p.n_t
    return _trained_point(src, ebno_db, snr_idx, n_blocks,
                          lambda T: train_shape_error(n_in, n_hidden, window, n_out, T),
                          lambda g: FnnBank(n_in, n_out, n_hidden, window, n_groups=g, device=src.device),
                          lambda block: fnn_weights(n_hidden, window * n_in, n_out, seed, block),
                          max(src.p.forget, window - 1), epochs=epochs, lr=lr, precision=precision, slice=slice,
                          weights=weights, first_block=first_block, frames_per_block=frames_per_block,
                          chunk_blocks=chunk_blocks)


def cnn_weights(channels, kernel, n_in, n_out, seed, block=None):
    """(W1 [c1, n_in, k], b1, W2 [c2, c1, k], b2, W3 [n_out, c2, k], b3), each U(+-1 / sqrt(fan_in)) with
    fan_in = c_in k -- the distribution of torch.nn.Conv1d -- drawn in that order from RandomState(seed) or, for the set
    of one global block, RandomState([seed, block])."""
    rs = np.random.RandomState(seed if block is None else [seed, block])
    c = (n_in, channels[0], channels[1], n_out)
    out = []
    for l in range(3):
        a = 1.0 / np.sqrt(c[l] * kernel)
        out += [rs.uniform(-a, a, (c[l + 1], c[l], kernel)), rs.uniform(-a, a, c[l + 1])]
    return tuple(out)


def cnn_point(src, ebno_db, snr_idx, n_blocks, *, channels=(32, 64), kernel=5, epochs=50, lr=0.01, slice="aligned",
              weights="shared", first_block=0, seed=0, frames_per_block=None, chunk_blocks=None):
    """One Eb/No point of the windowed CNN (cnn.CnnBank), the reference's third learned comparator, on the frames
    elm_point, fnn_point and a DetectorSweep over the same FrameSource seed detect: per chunk the pilot of every block
    gives one training (inputs and teacher scaled by 1 / sqrt(var_x), the loss over rows from delay + cp on, `epochs`
    Adam steps from cnn_weights), then all data frames are predicted in one launch and counted by the detector tail.
    slice and weights as in elm_point ("reference": rows [0, N) of the un-cut output, the slice the reference's CNN
    branch takes, :535-536).  Float64 throughout.  Returns (errors, bits): int64 [n_blocks] on the device; nothing is
    read back inside the chunk loop."""
    _check_windowed_point_args(slice, weights, "f64", 1, n_blocks, first_block, chunk_blocks, frames_per_block)
    channels = tuple(channels)
    if len(channels) != 2 or not all(isinstance(c, int) and c >= 1 for c in channels):
        raise ValueError(f"channels must be two positive integers, not {channels!r}")
    if not isinstance(kernel, int):
        raise ValueError(f"kernel must be an integer, not {kernel!r}")
    from .cnn import CnnBank, train_shape_error
    n_in, n_out = 2 * src.p.n_r, 2 * src.p.n_t
    return _trained_point(src, ebno_db, snr_idx, n_blocks,
                          lambda T: train_shape_error(n_in, channels[0], channels[1], n_out, kernel, T),
                          lambda g: CnnBank(n_in, n_out, channels, kernel, n_groups=g, device=src.device),
                          lambda block: cnn_weights(channels, kernel, n_in, n_out, seed, block),
                          src.p.forget, epochs=epochs, lr=lr, precision="f64", slice=slice, weights=weights,
                          first_block=first_block, frames_per_block=frames_per_block, chunk_blocks=chunk_blocks)


def lstm_weights(n_hidden, n_in, n_out, seed, block=None):
    """(W_ih [4H, n_in], W_hh [4H, H], b_ih [4H], b_hh [4H], W_fc [n_out, H], b_fc [n_out]), each U(+-1 / sqrt(H)) -- the
    distribution of torch.nn.LSTM and of torch.nn.Linear(H, .) -- drawn in that order from RandomState(seed) or, for the
    set of one global block, RandomState([seed, block])."""
    rs = np.random.RandomState(seed if block is None else [seed, block])
    a, h = 1.0 / np.sqrt(n_hidden), n_hidden
    return tuple(rs.uniform(-a, a, s) for s in ((4 * h, n_in), (4 * h, h), (4 * h,), (4 * h,), (n_out, h), (n_out,)))


def lstm_point(src, ebno_db, snr_idx, n_blocks, *, n_hidden=100, epochs=50, lr=0.01, slice="aligned", weights="shared",
               first_block=0, seed=0, frames_per_block=None, chunk_blocks=None):
    """One Eb/No point of the LSTM (lstm.LstmBank), the reference's fourth learned comparator (its RNN curve), on the
    frames elm_point, fnn_point, cnn_point and a DetectorSweep over the same FrameSource seed detect: per chunk the pilot
    of every block gives one training (inputs and teacher scaled by 1 / sqrt(var_x), the loss over rows from delay + cp
    on, `epochs` Adam steps from lstm_weights), then all data frames are predicted in one launch and counted by the
    detector tail.  slice and weights as in elm_point ("reference": rows [0, N) of the un-cut output, the slice the
    reference's RNN branch takes, :544-545).  Float64 throughout.  Returns (errors, bits): int64 [n_blocks] on the device;
    nothing is read back inside the chunk loop."""
    _check_windowed_point_args(slice, weights, "f64", 1, n_blocks, first_block, chunk_blocks, frames_per_block)
    if not isinstance(n_hidden, int) or n_hidden < 1:
        raise ValueError(f"n_hidden must be a positive integer, not {n_hidden!r}")
    from .lstm import LstmBank, train_shape_error
    n_in, n_out = 2 * src.p.n_r, 2 * src.p.n_t
    return _trained_point(src, ebno_db, snr_idx, n_blocks, lambda T: train_shape_error(n_in, n_hidden, n_out, T),
                          lambda g: LstmBank(n_in, n_out, n_hidden, n_groups=g, device=src.device),
                          lambda block: lstm_weights(n_hidden, n_in, n_out, seed, block),
                          src.p.forget, epochs=epochs, lr=lr, precision="f64", slice=slice, weights=weights,
                          first_block=first_block, frames_per_block=frames_per_block, chunk_blocks=chunk_blocks)


MEMBER_SEED_STRIDE = 104729     # member k of an ensemble draws its reservoirs from reservoir_seed + MEMBER_SEED_STRIDE k
MEMBER_LEG_SHIFT = 24           # ... and its state noise from stream_seed(snr_idx, leg + (k << MEMBER_LEG_SHIFT))


def ensemble_point(src, ebno_db, snr_idx, n_blocks, *, n_members=4, n_reservoir=256, spectral_radius=0.9, sparsity=0.1,
                   noise=0.001, precision="f32", fit_precision="f64", method="auto", ridge=None, ridge_grid=None,
                   reservoirs="shared", pool=8, io="f64", first_block=0, frames_per_block=None, chunk_blocks=None,
                   member_counts=False):
    """One Eb/No point of a reservoir ensemble (ensemble.EnsembleBank) on the frames a DetectorSweep over the same
    FrameSource seed detects: K independently drawn ESNs per coherence block, each with its own read-out fitted on the
    block's one pilot (K harvests and solves per chunk), K predict launches over the chunk's data frames into the slabs
    of one Y [K, B, N, 2 n_t], and one esn_detect_count_ens launch that averages the slabs before the FFT.

    Member k's reservoirs follow the sweep's rule with reservoir_seed + 104729 k (host draw for "shared" / "per_block",
    reservoirs.generate(first_set=global block) for "fresh") and its state-noise streams are
    sweep.stream_seed(seed, snr_idx, leg + (k << 24)), leg 0 for training and 1 for detection: member 0 is the
    reservoir and the streams of DetectorSweep(seed=src.seed), and ensemble_point(n_members=1) returns the counters of
    that sweep's run() on the same blocks bit for bit.  Scalings, fit (method, ridge, ridge_grid, fit_precision and the
    float32 states of the fp16 Cholesky path), predict and io are the sweep's.  One pilot per block; params.continuation
    is refused.  Returns (errors, bits): int64 [n_blocks] on the device, and with member_counts also int64
    [n_blocks, K], each member's own errors on the same frames.  chunk_blocks defaults to min(n_blocks, 4096 // K) --
    a chunk holds K slabs of Y -- and under "fresh" to what keeps K reservoirs per block within the sweep's budget.
    The counters do not depend on chunk_blocks or on how first_block cuts the blocks; nothing is read back inside the
    chunk loop (a flagged fit has the whole point redone with method="qr" after it: _retry_with_qr)."""
    from .ensemble import MAX_MEMBERS, EnsembleBank
    K = n_members
    if not isinstance(K, int) or not 1 <= K <= MAX_MEMBERS:
        raise ValueError(f"n_members must be an integer in 1..{MAX_MEMBERS}, not {n_members!r}")
    if reservoirs not in ("shared", "per_block", "fresh"):
        raise ValueError(f"reservoirs must be 'shared', 'per_block' or 'fresh', not {reservoirs!r}")
    _check_esn_point_args(method, io, precision, ridge, ridge_grid)
    _check_block_args(n_blocks, first_block, chunk_blocks, frames_per_block)
    torch, p = src.torch, src.p
    if p.continuation:
        raise ValueError("ensemble_point does not go with params.continuation: every member predicts from a zero state")
    n_in, n_out, n = 2 * p.n_r, 2 * p.n_t, int(n_reservoir)
    F, n_blocks = int(frames_per_block or p.coherence_symbols), int(n_blocks)
    chunk = int(chunk_blocks or min(n_blocks, max(1, 4096 // K)))      # (Y holds K slabs per chunk)
    res_args = (n_in, n_out, n, float(spectral_radius), float(sparsity))
    res_seed = [reservoir_seed(src.seed) + MEMBER_SEED_STRIDE * k for k in range(K)]
    kw, fresh = dict(noise=noise, device=src.device), reservoirs == "fresh"
    if fresh and chunk_blocks is None:        # K reservoirs per block live on the device for the length of a chunk
        per_block = K * DetectorSweep.FRESH_BYTES_PER_BLOCK_N2 * n * n
        chunk = min(chunk, max(1, DetectorSweep.FRESH_BUDGET_BYTES // per_block))
    grid_t = None
    if ridge_grid is not None:
        grid_t = _lambdas(torch, src.device, np.array(ridge_grid, dtype=np.float64).reshape(-1), 1, grid=True)[0][0]
    seeds = [[stream_seed(src.seed, snr_idx, leg + (k << MEMBER_LEG_SHIFT)) for k in range(K)] for leg in (0, 1)]
    T = p.t_frame + p.delay

    def point(method):
        ens = None
        if not fresh:
            n_sets = 1 if reservoirs == "shared" else int(pool)
            ens = EnsembleBank([host_reservoir_bank(*res_args, [res_seed[k] + i for i in range(n_sets)], **kw)
                                for k in range(K)])
        errors, nbits = (torch.zeros(n_blocks, dtype=torch.int64, device=src.device) for _ in range(2))
        merr = torch.zeros((n_blocks, K), dtype=torch.int64, device=src.device) if member_counts else None
        flagged = torch.zeros((), dtype=torch.int64, device=src.device)
        for b0, g, lo in _chunks(first_block, n_blocks, chunk):
            data = src.blocks_fast(ebno_db, snr_idx, b0, g, F, io="c64" if io == "f32" else "c128")
            if fresh:       # block b in slot b % g, the set the kernels pick for it under group_offset = b0
                sets = [_reservoirs.generate(*res_args, seed=res_seed[k], first_set=b0, n_sets=g, device=src.device,
                                             check_status=method == "qr", n_squarings=24) for k in range(K)]
                if ens is None:
                    ens = EnsembleBank([ReservoirBank(n_in, n_out, n, *s[:3], teacher_forcing=True, **kw) for s in sets])
                else:
                    for m, s in zip(ens.members, sets):
                        m.set_weights(*s[:3])
                for s in sets:
                    flagged += s[4].ne(0).sum()
            ens.set_scaling(*group_scalings(g, n_in, p.input_scaling(ebno_db), n_out, p.teacher_scale, src.device))
            U, D = pilot_rows(data["pilot_y"], data["pilot_x"], p.delay)
            e_dtype = fit_e_dtype(ens.members[0], method, fit_precision, T - p.forget, n + n_in)
            ens.fit(U, D, transient=p.forget, precision=fit_precision, noise_mode="counter", seed=seeds[0], method=method,
                    e_dtype=e_dtype, group_offset=b0, ridge=None if ridge is None else float(ridge), ridge_grid=grid_t)
            flagged += ens.fit_status.ne(0).sum()
            Y = ens.predict(_view_real(data["data_y"]), F, T=T, transient=p.forget, precision=precision,
                            noise_mode="counter", seed=seeds[1], group_offset=b0, io=io)
            ens.detect_count(Y, data["data_bits"], src.p_i(ebno_db, g), F, p.n_sub, p.n_t, p.m,
                             err=errors[lo:lo + g], bits=nbits[lo:lo + g],
                             member_err=None if merr is None else merr[lo:lo + g])
        return ((errors, nbits, merr) if member_counts else (errors, nbits)), flagged

    return _retry_with_qr(point, method)


def _equalized_esn_sets(who, src, n_blocks, n_reservoir, ridge, method, delay, spectral_radius, sparsity, precision,
                        reservoirs, pool, io, first_block, frames_per_block, chunk_blocks):
    """What equalized_esn_point and coded_equalized_point (`who`) refuse alike, then the host-drawn reservoir sets."""
    if reservoirs not in ("shared", "per_block"):
        raise ValueError(f"reservoirs must be 'shared' or 'per_block', not {reservoirs!r} (device-drawn reservoirs are "
                         "not served behind the equaliser)")
    _check_esn_point_args(method, io, precision, ridge)
    _check_block_args(n_blocks, first_block, chunk_blocks, frames_per_block)
    if not isinstance(n_reservoir, int) or n_reservoir < 2:
        raise ValueError(f"n_reservoir must be an integer of at least 2, not {n_reservoir!r}")
    if not isinstance(delay, int) or delay < 0:
        raise ValueError(f"delay must be a non-negative integer, not {delay!r}")
    if reservoirs == "per_block" and int(pool) < 1:
        raise ValueError(f"pool = {pool} must be positive")
    p = src.p
    if p.continuation:
        raise ValueError(f"{who} does not go with params.continuation: every frame is predicted from a zero state")
    if p.n_t > 4:
        raise ValueError(f"n_t = {p.n_t}: the equaliser kernels serve up to 4 transmit antennas")
    n_io, n = 2 * p.n_t, n_reservoir
    with np.errstate(all="ignore"):
        sets = host_reservoirs(n_io, n_io, n, float(spectral_radius), float(sparsity),
                               [reservoir_seed(src.seed) + i for i in range(1 if reservoirs == "shared" else int(pool))])
    if not np.isfinite(sets[0]).all():
        raise ValueError(f"a drawn {n} x {n} reservoir has no finite spectral radius to scale to (all its eigenvalues "
                         "are zero): take more units or a smaller sparsity")
    return sets


def _equalized_esn_chunk(src, bank, H, pilot_y, pilot_x, data_y, ebno_db, F, b0, *, delay, ridge, method, precision, io,
                         seeds):
    """The detector chain behind the equaliser on one chunk of g = H.shape[0] blocks from global block b0 on: the
    equalised rows of the dense pilot and of the data frames, `bank` fitted on the pilot rows against the pre-PA pilot
    delayed by `delay` rows, one predict over the data rows.  Returns (Y, flagged): what a detector tail reads, and how
    many of the chunk's fits the kernel flagged (a device scalar)."""
    p, g, n_io = src.p, H.shape[0], 2 * src.p.n_t
    T, transient = p.t_frame + delay, delay + p.cp
    U = src.equalize_rows(H, pilot_y, 1, ebno_db, pad=delay)
    rows = src.equalize_rows(H, data_y, F, ebno_db, pad=delay, io=io)
    bank.set_scaling(*group_scalings(g, n_io, p.input_scaling(ebno_db), n_io, p.teacher_scale, src.device))
    _, D = pilot_rows(None, pilot_x, delay)
    bank.fit(U, D, transient=transient, precision="f64", noise_mode="counter", seed=seeds[0], method=method,
             group_offset=b0, ridge=None if ridge is None else float(ridge))
    flagged = bank.fit_status.ne(0).sum()
    Y = bank.predict(rows, F, T=T, transient=transient, precision=precision, noise_mode="counter", seed=seeds[1],
                     group_offset=b0, io=io)
    return Y, flagged


def equalized_esn_point(src, ebno_db, snr_idx, n_blocks, *, n_reservoir=8, ridge=1e-5, method="auto", delay=0,
                        spectral_radius=0.9, sparsity=0.1, noise=0.001, precision="f64", reservoirs="shared", pool=8,
                        io="f64", first_block=0, frames_per_block=None, chunk_blocks=None, want_mmse=False,
                        want_xhat=False):
    """One Eb/No point of an ESN that stands behind the LS-MMSE equaliser, on the frames a DetectorSweep over the same
    FrameSource seed and its baseline leg see: per chunk blocks_fast(with_ls_pilot=True), the pilot's channel estimate
    (estimate_channel), FrameSource.equalize_rows on the dense pilot (one frame per group) and on the data frames --
    the equalised signal back in the time domain, 2 n_t real columns -- and a ReservoirBank(2 n_t, 2 n_t, n_reservoir)
    fitted on the pilot rows against the pre-PA pilot delayed by `delay` rows (transient delay + cp; pinv with ridge=None,
    else `ridge`), then one predict over the chunk's data rows and the detector tail.

    Input scaling is the sweep's input_scaler / sqrt(var_x), teacher scaling its teacher_scale.  The reservoir is the
    host draw of the sweep (draw_reservoir(src.seed * 7919 + 17 + i): one set for "shared", `pool` sets picked by
    global block for "per_block") and the state-noise streams are stream_seed(src.seed, snr_idx, leg), leg 0 for training
    and 1 for detection: member 0's of ensemble_point.  The harvest is float64; `precision` and io ("f32": float32 rows
    into and out of predict) are the prediction's.  One pilot per block, block fading or not; params.continuation and
    n_t > 4 are refused.  Returns (errors, bits): int64 [n_blocks] on the device; with want_mmse also (errors, bits) of
    esn_mmse_detect_count on the same frames and the same H.  The counters do not depend on chunk_blocks or on how
    first_block cuts the blocks; nothing is read back inside the chunk loop (a flagged fit has the whole point redone
    with method="qr" after it).  want_xhat is test support, not part of a sweep: it appends the detector tail's X_hat,
    complex128 [n_blocks F, N, n_t], and keeps every chunk's alive until the end."""
    sets = _equalized_esn_sets("equalized_esn_point", src, n_blocks, n_reservoir, ridge, method, delay, spectral_radius,
                               sparsity, precision, reservoirs, pool, io, first_block, frames_per_block, chunk_blocks)
    torch, p = src.torch, src.p
    n_io = 2 * p.n_t
    F, n_blocks = int(frames_per_block or p.coherence_symbols), int(n_blocks)
    chunk = int(chunk_blocks or min(n_blocks, 4096))
    seeds = [stream_seed(src.seed, snr_idx, leg) for leg in (0, 1)]

    def point(method):
        bank = ReservoirBank(n_io, n_io, n_reservoir, *sets, teacher_forcing=True, noise=noise, device=src.device)
        errors, nbits = (torch.zeros(n_blocks, dtype=torch.int64, device=src.device) for _ in range(2))
        mm_err, mm_bits = (torch.zeros(n_blocks, dtype=torch.int64, device=src.device) if want_mmse else None
                           for _ in range(2))
        flagged = torch.zeros((), dtype=torch.int64, device=src.device)
        kept = []
        for b0, g, lo in _chunks(first_block, n_blocks, chunk):
            data = src.blocks_fast(ebno_db, snr_idx, b0, g, F, with_ls_pilot=True)
            H = src.estimate_channel(data["pilot_bits"], data["pilot_y_ls"], ebno_db)
            if want_mmse:
                src.mmse_detect_count(H, data["data_y"], data["data_bits"], F, ebno_db, err=mm_err[lo:lo + g],
                                      bits=mm_bits[lo:lo + g])
            Y, bad = _equalized_esn_chunk(src, bank, H, data["pilot_y"], data["pilot_x"], data["data_y"], ebno_db, F, b0,
                                          delay=delay, ridge=ridge, method=method, precision=precision, io=io,
                                          seeds=seeds)
            flagged += bad
            out = bank.detect_count(Y, data["data_bits"], src.p_i(ebno_db, g), F, p.n_sub, p.n_t, p.m,
                                    err=errors[lo:lo + g], bits=nbits[lo:lo + g], want_xhat=want_xhat)
            if want_xhat:
                kept.append(torch.view_as_complex(out[2].view(g * F, p.n_sub, p.n_t, 2).contiguous()))
        return (errors, nbits) + ((mm_err, mm_bits) if want_mmse else ()) + ((torch.cat(kept),) if kept else ()), flagged

    return _retry_with_qr(point, method)


def dcc_point(src, ebno_db, snr_idx, n_blocks, *, n_iter=2, a_clip_db_error=0.0, first_block=0, frames_per_block=None,
              chunk_blocks=None, want_mmse=False):
    """One Eb/No point of the amplifier-aware LS-MMSE baseline (FrameSource.mmse_dcc_detect_count: n_iter passes of
    decision-aided cancellation of the amplifier's distortion), on the frames equalized_esn_point sees: per chunk
    blocks_fast(with_ls_pilot=True) and the pilot's channel estimate (estimate_channel).  The detector is told the clip
    level p.a_clip(ebno_db) times 10^(a_clip_db_error / 20): 0 the generator's own, anything else a mismatch study.
    Returns (errors, bits, iter_errors): int64 [n_blocks], [n_blocks] and [n_iter + 1] on the device -- the counters of
    X^{n_iter} per block and the point's bit errors after 0 .. n_iter passes; with want_mmse also (errors, bits) of
    esn_mmse_detect_count on the same frames and the same H, which n_iter=0 equals bit for bit.  The counters do not
    depend on chunk_blocks or on how first_block cuts the blocks; nothing is read back.  n_t > 4 is refused."""
    _check_block_args(n_blocks, first_block, chunk_blocks, frames_per_block)
    if not isinstance(n_iter, int) or not 0 <= n_iter <= 8:
        raise ValueError(f"n_iter must be an integer in 0..8, not {n_iter!r}")
    if not np.isfinite(float(a_clip_db_error)):
        raise ValueError(f"a_clip_db_error = {a_clip_db_error} must be finite")
    torch, p = src.torch, src.p
    if p.n_t > 4:
        raise ValueError(f"n_t = {p.n_t}: the equaliser kernels serve up to 4 transmit antennas")
    F, n_blocks = int(frames_per_block or p.coherence_symbols), int(n_blocks)
    chunk = int(chunk_blocks or min(n_blocks, 4096))
    a_clip = p.a_clip(ebno_db) * 10.0 ** (float(a_clip_db_error) / 20.0)
    errors, nbits = (torch.zeros(n_blocks, dtype=torch.int64, device=src.device) for _ in range(2))
    mm_err, mm_bits = (torch.zeros(n_blocks, dtype=torch.int64, device=src.device) if want_mmse else None
                       for _ in range(2))
    iter_errors = torch.zeros(n_iter + 1, dtype=torch.int64, device=src.device)
    for b0, g, lo in _chunks(first_block, n_blocks, chunk):
        data = src.blocks_fast(ebno_db, snr_idx, b0, g, F, with_ls_pilot=True)
        H = src.estimate_channel(data["pilot_bits"], data["pilot_y_ls"], ebno_db)
        if want_mmse:
            src.mmse_detect_count(H, data["data_y"], data["data_bits"], F, ebno_db, err=mm_err[lo:lo + g],
                                  bits=mm_bits[lo:lo + g])
        out = src.mmse_dcc_detect_count(H, data["data_y"], data["data_bits"], F, ebno_db, n_iter=n_iter, a_clip=a_clip,
                                        err=errors[lo:lo + g], bits=nbits[lo:lo + g], want_iter_counts=True)
        iter_errors += out[2].sum(dim=0)
    return (errors, nbits, iter_errors) + ((mm_err, mm_bits) if want_mmse else ())


def coded_equalized_point(src, code, ebno_db, snr_idx, n_blocks, *, llr="sinr", n_reservoir=8, ridge=1e-5, delay=0,
                          cal_frac=0.3, seed=0, method="auto", spectral_radius=0.9, sparsity=0.1, noise=0.001,
                          precision="f64", reservoirs="shared", pool=8, io="f64", frames_per_block=None, want_xhat=False):
    """One Eb/No point of the coded comparison for the ESN behind the LS-MMSE equaliser: the payloads, taps, pilot and
    data frames of coded_ber_point (_coded_block_data: same generator key, salt 12345), the pilot's channel estimate,
    the detector chain of equalized_esn_point (_equalized_esn_chunk: same reservoir draw, state-noise streams
    stream_seed(src.seed, snr_idx, leg) + seed) into the fused soft tail (detect_llr), and the LS-MMSE detector on the
    same frames (mmse_detect_count, LdpcCode.llrs); then, per detector, the logistic calibration fitted on the first
    cal_frac of the blocks and sum-product decoding of the rest, as coded_ber_point.

    llr="flat": one decision-directed sigma^2 per frame for every symbol of it, the reference's LLRs -- the MMSE leg is
    then coded_ber_point's, bit for bit.  llr="sinr": the LLRs of both detectors weighted by the equaliser's SINR per
    subcarrier and stream over the block's mean, on the symbol with the equaliser's bias taken out
    (FrameSource.mmse_sinr on the same H); the uncoded columns do not depend on it.  The raw SINR as the scale is not
    offered: LLRs of magnitude 10^3 make the calibration's gradient steps diverge from 15 dB on.

    One chunk: all n_blocks blocks at once, block 0 first.  Refused arguments are equalized_esn_point's.  Returns
    coded_ber_point's dictionary: ESN_uncoded, MMSE_uncoded, ESN_coded, MMSE_coded, a_esn, b_esn, a_mmse, b_mmse;
    want_xhat (test support) adds x_esn, the soft tail's X_hat, complex128 [n_blocks F, N, n_t]."""
    if llr not in ("sinr", "flat"):
        raise ValueError(f"llr must be 'sinr' or 'flat', not {llr!r}")
    if not 0.0 < float(cal_frac) < 1.0:
        raise ValueError(f"cal_frac = {cal_frac} must be inside (0, 1)")
    sets = _equalized_esn_sets("coded_equalized_point", src, n_blocks, n_reservoir, ridge, method, delay, spectral_radius,
                               sparsity, precision, reservoirs, pool, io, 0, frames_per_block, None)
    torch, p = src.torch, src.p
    n_io, G = 2 * p.n_t, int(n_blocks)
    F = int(frames_per_block or p.coherence_symbols)
    n_cal = max(1, int(round(cal_frac * G))) * F                             # frames used for calibration
    if n_cal >= G * F:
        raise ValueError(f"n_blocks = {G} leaves no block to decode behind the {n_cal // F} calibration blocks")
    if code.n != p.n_sub * p.m:
        raise ValueError(f"the code's length {code.n} is not the frame's N m = {p.n_sub * p.m} bits per stream")
    seeds = [stream_seed(src.seed, snr_idx, leg) + int(seed) for leg in (0, 1)]
    u, tx_bits, _, (pbits, px, py), py_ls, dy = _coded_block_data(src, code, ebno_db, snr_idx, G, F, seed, 12345)
    H = src.estimate_channel(pbits, py_ls, ebno_db)
    w, mu = src.mmse_sinr(H, ebno_db)[:2] if llr == "sinr" else (None, None)
    e_mm, n_mm, x_mm = src.mmse_detect_count(H, dy, tx_bits, F, ebno_db, want_xhat=True)
    llr_mm = code.llrs(x_mm, p.m, weights=w, bias=mu, frames_per_group=F)[0]

    def esn_leg(method):
        bank = ReservoirBank(n_io, n_io, n_reservoir, *sets, teacher_forcing=True, noise=noise, device=src.device)
        Y, flagged = _equalized_esn_chunk(src, bank, H, py, px, dy, ebno_db, F, 0, delay=delay, ridge=ridge,
                                          method=method, precision=precision, io=io, seeds=seeds)
        return bank.detect_llr(Y, tx_bits, src.p_i(ebno_db, G), F, p.n_sub, p.n_t, p.m, weights=w, bias=mu,
                               want_xhat=want_xhat), flagged

    tail = _retry_with_qr(esn_leg, method)
    e_esn, n_esn, llr_esn = tail[:3]
    out = dict(ESN_uncoded=float(e_esn.sum()) / float(n_esn.sum()), MMSE_uncoded=float(e_mm.sum()) / float(n_mm.sum()))
    for name, l in (("ESN", llr_esn), ("MMSE", llr_mm)):
        _calibrated_leg(out, name, code, l, tx_bits, u, n_cal, p.n_t * F, p.m)
    if want_xhat:
        out["x_esn"] = torch.view_as_complex(tail[4].view(G * F, p.n_sub, p.n_t, 2).contiguous())
    return out
