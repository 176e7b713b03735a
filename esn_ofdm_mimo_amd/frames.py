"""The frame side of the Monte-Carlo harness (montecarlo.py tells the whole chain): FrameSource, the HIP frame generator
with the baseline equalisers and channel metrics that read its taps and frames; percentiles_linear and
summarize_channel_metrics, the per-Eb/No channel record reduced on the device; _view_real / complex_as_io, complex
frames as the interleaved real rows the ESN reads; pilot_rows and group_scalings, the padded pilot rows and the
scalings of a chunk of blocks, for the sweep and the points alike.  torch is imported where it is used: no GPU is needed
to import."""
from __future__ import annotations

from . import _lib
from ._lib import check, ptr
from .link import LinkParams


class FrameSource:
    """HIP frame generator (esn_gen_taps / esn_gen_frames of include/esn_hip.h).  Counter-based
    random streams: frame f of block b at SNR index s is a pure function of (seed, s, b, f)."""

    CHANNEL_KIND = {"tdlb": 0, "exp": 1, "awgn": 2}

    def __init__(self, params: LinkParams, device=None, seed=0):
        torch = _lib.require_gpu()
        self.torch, self.p = torch, params
        self.lib = _lib.load()
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self.seed = int(seed)
        self._track_reg = {}                 # Eb/No -> reg [isi] on the device (track_channel)

    def _key(self, *parts):
        h = self.seed & (2 ** 64 - 1)
        for k in parts:
            h = (h * 6364136223846793005 + int(k) + 0x9E3779B97F4A7C15) % (2 ** 64)
        return h

    def _per_group(self, value, g):
        """float64 [g] on the device, every entry `value`: the kernels take Pi and the clip level per group."""
        return self.torch.full((g,), value, dtype=self.torch.float64, device=self.device)

    def p_i(self, ebno_db, g):
        """Pi of g blocks at this Eb/No, float64 [g] on the device: the generator scales by it, the tails divide by it."""
        return self._per_group(self.p.p_i(ebno_db), g)

    def taps(self, n_blocks, snr_idx, first_block, gains=None):
        """[G, n_r, n_t, isi] complex128.  Link l of block b draws from counter (first_block + b)."""
        torch, p = self.torch, self.p
        with torch.cuda.device(self.device):
            out = torch.empty((n_blocks, p.n_r, p.n_t, p.isi), dtype=torch.complex128, device=self.device)
            check(self.lib.esn_gen_taps(self.CHANNEL_KIND[p.channel], n_blocks, p.n_r, p.n_t, p.isi, p.fs, p.ds_ns,
                                        ptr(gains), self._key(snr_idx, 1), int(first_block) * p.n_r * p.n_t,
                                        ptr(out), _lib.stream_handle()), "esn_gen_taps")
        return out

    def taps_doppler(self, n_blocks, n_sym, snr_idx, first_block, angles=None):
        """[G, n_sym, n_r, n_t, isi] complex128: the taps of symbols 0 .. n_sym - 1 of every block under Jakes fading
        with params.fd_tsym cycles per symbol (esn_gen_taps_doppler; key and link counters of taps()).  angles:
        optional float64 [G n_r n_t, n_paths, 16, 2] = (a, phi) in half-turns instead of the device's draws."""
        torch, p = self.torch, self.p
        with torch.cuda.device(self.device):
            out = torch.empty((n_blocks, n_sym, p.n_r, p.n_t, p.isi), dtype=torch.complex128, device=self.device)
            check(self.lib.esn_gen_taps_doppler(self.CHANNEL_KIND[p.channel], n_blocks, n_sym, p.n_r, p.n_t, p.isi,
                                                p.fs, p.ds_ns, p.fd_tsym, ptr(angles), self._key(snr_idx, 1),
                                                int(first_block) * p.n_r * p.n_t, ptr(out), _lib.stream_handle()),
                  "esn_gen_taps_doppler")
        return out

    def frames(self, taps, frames_per_block, ebno_db, snr_idx, first_frame, stream_id, want_x=False,
               bits_in=None, noise_in=None, ls_pattern=False, io="c128"):
        """frames_per_block frames per block of `taps` -> (bits uint8 [B,N*m,n_t], x_cp or None, y_cp).
        stream_id separates pilots (0) from data (1); first_frame is the global frame counter.
        io="c64": x_cp / y_cp complex64 (esn_gen_frames_c64), bitwise the complex128 frames rounded."""
        torch, p = self.torch, self.p
        if io not in ("c128", "c64"):
            raise ValueError(f"io must be 'c128' or 'c64', not {io!r}")
        cdt = torch.complex64 if io == "c64" else torch.complex128
        g = taps.shape[0]
        b = g * frames_per_block
        with torch.cuda.device(self.device):
            p_i = self.p_i(ebno_db, g)
            a_clip = self._per_group(p.a_clip(ebno_db), g)
            bits = torch.empty((b, p.n_sub * p.m, p.n_t), dtype=torch.uint8, device=self.device)
            x_cp = torch.empty((b, p.t_frame, p.n_t), dtype=cdt, device=self.device) if want_x else None
            y_cp = torch.empty((b, p.t_frame, p.n_r), dtype=cdt, device=self.device)
            name = "esn_gen_frames_c64" if io == "c64" else "esn_gen_frames"
            check(getattr(self.lib, name)(b, frames_per_block, p.n_sub, p.cp, p.n_t, p.n_r, p.isi, p.m,
                                          1 if ls_pattern else 0, ptr(p_i),
                                          ptr(a_clip), p.no, ptr(taps), ptr(bits_in), ptr(noise_in),
                                          self._key(snr_idx, 2 + stream_id), int(first_frame), ptr(bits), ptr(x_cp),
                                          ptr(y_cp), _lib.stream_handle()), name)
        return bits, x_cp, y_cp

    def blocks(self, ebno_db, snr_idx, block_ids, frames_per_block, with_ls_pilot=False, io="c128", n_pilots=1):
        """Pilot + data frames of the given coherence blocks (any subset, any order: every block is
        generated from its own global index, so the result does not depend on the rank that asks).
        Returns pilot_y [G,T,n_r], pilot_x [G,T,n_t] (pre-PA teacher), data_y [G*F,T,n_r], data_bits."""
        torch = self.torch
        ids = list(block_ids)
        runs, start = [], 0                          # contiguous runs of block ids -> one launch each
        for i in range(1, len(ids) + 1):
            if i == len(ids) or ids[i] != ids[i - 1] + 1:
                runs.append((ids[start], i - start)); start = i
        outs = [self.blocks_fast(ebno_db, snr_idx, b0, n, frames_per_block, with_ls_pilot, io, n_pilots=n_pilots)
                for b0, n in runs]
        return {k: torch.cat([o[k] for o in outs]) for k in outs[0]}

    PILOT_STREAM0 = 2                        # stream id of pilot 1 (0: pilot 0, 1: data); pilot p >= 1 has 1 + p

    def blocks_fast(self, ebno_db, snr_idx, first_block, n_blocks, frames_per_block, with_ls_pilot=False, io="c128",
                    want_data_x=False, n_pilots=1):
        """Blocks first_block .. first_block + n_blocks - 1 in three launches (taps, pilots, data).
        io="c64": the DATA frames are complex64; pilots stay complex128 (training is unchanged).
        params.fading == "jakes": the taps move inside the block (taps_doppler, 1 + F symbols): the pilots pass
        through symbol 0, data frame k through symbol k + 1 -- one frames() call over the per-frame taps with one frame
        per "block"; frame counters and streams are those of block fading, so bits and noise are the same for the same
        seed.  `taps` stays the pilot-instant taps [G, n_r, n_t, isi]; `taps_sym` [G, 1 + F, n_r, n_t, isi] is added.
        want_data_x: `data_x` [G F, T, n_t] is added, the pre-PA transmit signal of every data frame (what pilot_x is to
        the pilot: the teacher a genie-aided re-fit would use).
        n_pilots = P > 1 (an extension: the reference sends one pilot per block): pilot 0 is the pilot above, same key
        and counter; pilot p >= 1 is one more frames() call over the block's taps under stream id 1 + p, a function of
        (seed, Eb/No index, global block, p) alone.  The dict gains `pilots_y` [G, P, T, n_r], `pilots_x` [G, P, T, n_t],
        `pilots_bits` [G, P, N m, n_t] and, with with_ls_pilot, `pilots_y_ls` [G, P, T, n_r]; the other keys are what
        they are with one pilot.  Under "jakes" the block has P + F symbols: pilot p passes through symbol p and data
        frame k through symbol P + k (`taps_sym` [G, P + F, ...])."""
        p, F, P = self.p, frames_per_block, int(n_pilots)
        if P < 1:
            raise ValueError(f"n_pilots must be at least 1, not {n_pilots}")
        if p.fading == "jakes":
            taps_sym = self.taps_doppler(n_blocks, P + F, snr_idx, first_block)
            taps = taps_sym[:, 0].contiguous()
            data_taps, per_taps = taps_sym[:, P:].reshape(n_blocks * F, p.n_r, p.n_t, p.isi), 1
        else:
            taps_sym, taps = None, self.taps(n_blocks, snr_idx, first_block)
            data_taps, per_taps = taps, F
        pbits, px, py = self.frames(taps, 1, ebno_db, snr_idx, first_block, 0, want_x=True)
        bits, dx, dy = self.frames(data_taps, per_taps, ebno_db, snr_idx, first_block * F, 1, io=io,
                                   want_x=want_data_x)
        out = dict(pilot_y=py, pilot_x=px, pilot_bits=pbits, data_y=dy, data_bits=bits, taps=taps)
        if want_data_x:
            out["data_x"] = dx
        if taps_sym is not None:
            out["taps_sym"] = taps_sym
        if with_ls_pilot:     # same bits, same noise, sparse pattern (driver:330-356)
            _, _, out["pilot_y_ls"] = self.frames(taps, 1, ebno_db, snr_idx, first_block, 0, ls_pattern=True)
        if P > 1:
            more = [(pbits, px, py, out.get("pilot_y_ls"))]
            for q in range(1, P):
                tq = taps if taps_sym is None else taps_sym[:, q].contiguous()
                sid = self.PILOT_STREAM0 + q - 1
                bq, xq, yq = self.frames(tq, 1, ebno_db, snr_idx, first_block, sid, want_x=True)
                ls = self.frames(tq, 1, ebno_db, snr_idx, first_block, sid, ls_pattern=True)[2] if with_ls_pilot else None
                more.append((bq, xq, yq, ls))
            torch = self.torch
            out["pilots_bits"], out["pilots_x"], out["pilots_y"] = (torch.stack([m[i] for m in more], dim=1)
                                                                    for i in range(3))
            if with_ls_pilot:
                out["pilots_y_ls"] = torch.stack([m[3] for m in more], dim=1)
        return out

    # ---- baseline equaliser ------------------------------------------------------
    def estimate_channel(self, pilot_bits, pilot_y_ls, ebno_db, ls_only=False):
        """LS + time-domain MMSE channel estimate H [G, N, n_r, n_t] (driver:358-382); ls_only: the interpolated
        LS estimate H_LS of the block-fading drivers' LS-ZF detector (OFDM_MIMO_2-2_NBF_LDPC.py:321-333)."""
        torch, p = self.torch, self.p
        g = pilot_bits.shape[0]
        with torch.cuda.device(self.device):
            p_i = self.p_i(ebno_db, g)
            H = torch.empty((g, p.n_sub, p.n_r, p.n_t), dtype=torch.complex128, device=self.device)
            check(self.lib.esn_channel_estimate(g, p.n_sub, p.cp, p.n_t, p.n_r, p.isi, p.m, ptr(p_i), p.no,
                                                ptr(pilot_bits.contiguous()), ptr(pilot_y_ls.contiguous()),
                                                1 if ls_only else 0, ptr(H), _lib.stream_handle()),
                  "esn_channel_estimate")
        return H

    def true_channel(self, taps):
        """H_true [G, N, n_r, n_t] = FFT_N of the zero-padded taps (OFDM_MIMO_2-2_NBF_LDPC.py:273-279)."""
        torch, p = self.torch, self.p
        g = taps.shape[0]
        with torch.cuda.device(self.device):
            H = torch.empty((g, p.n_sub, p.n_r, p.n_t), dtype=torch.complex128, device=self.device)
            check(self.lib.esn_taps_to_freq(g, p.n_sub, p.n_t, p.n_r, p.isi, ptr(taps.contiguous()), ptr(H),
                                            _lib.stream_handle()), "esn_taps_to_freq")
        return H

    def mmse_detect_count(self, H, data_y, data_bits, frames_per_block, ebno_db, err=None, bits=None,
                          want_xhat=False, zf=False):
        """Per-subcarrier MMSE detector + error counters (driver:444-456); zf=True: equalize_zf (driver:34-39),
        LS-ZF with an estimated H, Perfect-ZF with `true_channel` (OFDM_MIMO_2-2_NBF_LDPC.py:450-460)."""
        torch, p = self.torch, self.p
        g, b = H.shape[0], data_y.shape[0]
        with torch.cuda.device(self.device):
            p_i = self.p_i(ebno_db, g)
            if err is None:
                err = torch.zeros(g, dtype=torch.int64, device=self.device)
            if bits is None:
                bits = torch.zeros(g, dtype=torch.int64, device=self.device)
            xh = torch.empty((b, p.n_sub, p.n_t), dtype=torch.complex128, device=self.device) if want_xhat else None
            if zf:
                check(self.lib.esn_zf_detect_count(b, int(frames_per_block), p.n_sub, p.cp, p.n_t, p.n_r, p.m,
                                                   ptr(p_i), ptr(H), ptr(data_y.contiguous()),
                                                   ptr(data_bits.contiguous()), ptr(err), ptr(bits), ptr(xh),
                                                   _lib.stream_handle()), "esn_zf_detect_count")
            else:
                check(self.lib.esn_mmse_detect_count(b, int(frames_per_block), p.n_sub, p.cp, p.n_t, p.n_r, p.m,
                                                     ptr(p_i), p.no, ptr(H), ptr(data_y.contiguous()),
                                                     ptr(data_bits.contiguous()), ptr(err), ptr(bits), ptr(xh),
                                                     _lib.stream_handle()), "esn_mmse_detect_count")
        return (err, bits, xh) if want_xhat else (err, bits)

    def mmse_dcc_detect_count(self, H, data_y, data_bits, frames_per_block, ebno_db, n_iter=2, a_clip=None, err=None,
                              bits=None, want_xhat=False, want_iter_counts=False):
        """The LS-MMSE detector with n_iter passes of decision-aided cancellation of the amplifier's distortion
        (esn_mmse_dcc_detect_count): slice, re-modulate, pass the decisions through x / sqrt(1 + (|x|/A)^2), subtract the
        predicted distortion behind the same equaliser.  n_iter=0 is mmse_detect_count bit for bit.  a_clip: None, the
        generator's p.a_clip(ebno_db) for every group; a number, or float64 [G] (host or device), a clip level of the
        caller's -- a wrong one is allowed (mismatch studies), a non-finite or non-positive one is not.  data_bits=None:
        nothing is counted (then want_xhat must be set).  Returns (err, bits[, X_hat][, err_iter]): the counters of
        X^{n_iter} per group, X_hat complex128 [B, N, n_t], err_iter int64 [G, n_iter + 1] the errors of X^0 .. X^{n_iter}."""
        torch, p = self.torch, self.p
        n_iter = int(n_iter)
        if not 0 <= n_iter <= 8:
            raise ValueError(f"n_iter = {n_iter} must be in 0..8")
        g, b = H.shape[0], data_y.shape[0]
        if data_bits is None and not want_xhat:
            raise ValueError("data_bits=None counts nothing: ask for X_hat")
        with torch.cuda.device(self.device):
            p_i = self.p_i(ebno_db, g)
            if a_clip is None:
                a_clip = self._per_group(p.a_clip(ebno_db), g)
            else:
                host = torch.as_tensor(a_clip, dtype=torch.float64).reshape(-1).cpu()
                if host.numel() not in (1, g):
                    raise ValueError(f"a_clip must be one number or one per group ({g}), not {host.numel()} entries")
                if not bool((torch.isfinite(host) & (host > 0)).all()):
                    raise ValueError("a_clip must be finite and positive")
                a_clip = host.expand(g).contiguous().to(self.device)
            if data_bits is not None:
                if err is None:
                    err = torch.zeros(g, dtype=torch.int64, device=self.device)
                if bits is None:
                    bits = torch.zeros(g, dtype=torch.int64, device=self.device)
            it = torch.zeros((g, n_iter + 1), dtype=torch.int64, device=self.device) \
                if want_iter_counts and data_bits is not None else None
            xh = torch.empty((b, p.n_sub, p.n_t), dtype=torch.complex128, device=self.device) if want_xhat else None
            check(self.lib.esn_mmse_dcc_detect_count(b, int(frames_per_block), p.n_sub, p.cp, p.n_t, p.n_r, p.m, n_iter,
                                                     ptr(p_i), ptr(a_clip), p.no, ptr(H.contiguous()),
                                                     ptr(data_y.contiguous()),
                                                     ptr(None if data_bits is None else data_bits.contiguous()),
                                                     ptr(err), ptr(bits), ptr(it), ptr(xh), _lib.stream_handle()),
                  "esn_mmse_dcc_detect_count")
        return (err, bits) + ((xh,) if want_xhat else ()) + ((it,) if want_iter_counts else ())

    def mmse_sinr(self, H, ebno_db):
        """What the MMSE equaliser under H [G, N, n_r, n_t] does to every stream of every subcarrier (esn_mmse_sinr):
        with t = lam [(H_k^H H_k + lam I)^-1]_ii, lam = No / Pi, returns (w, mu, gamma_mean) -- mu = 1 - t the bias,
        w the SINR (1 - t) / t over the block's mean SINR gamma_mean [G]; w and mu float64 [G, N, n_t], what
        LdpcCode.llrs and the banks' detect_llr take as weights and bias."""
        torch, p = self.torch, self.p
        if H.dtype != torch.complex128 or H.dim() != 4 or tuple(H.shape[1:]) != (p.n_sub, p.n_r, p.n_t):
            raise ValueError(f"H must be complex128 [G, {p.n_sub}, {p.n_r}, {p.n_t}], not {H.dtype} {tuple(H.shape)}")
        g = H.shape[0]
        with torch.cuda.device(self.device):
            p_i = self.p_i(ebno_db, g)
            w, mu = (torch.empty((g, p.n_sub, p.n_t), dtype=torch.float64, device=self.device) for _ in range(2))
            mean = torch.empty((g,), dtype=torch.float64, device=self.device)
            check(self.lib.esn_mmse_sinr(g, p.n_sub, p.n_t, p.n_r, ptr(p_i), p.no, ptr(H.contiguous()), ptr(w), ptr(mu),
                                         ptr(mean), _lib.stream_handle()), "esn_mmse_sinr")
        return w, mu, mean

    def equalize_rows(self, H, y, frames_per_block, ebno_db, pad=0, io="f64", want_xhat=False):
        """The MMSE equaliser's output back in the time domain (esn_mmse_equalize_rows): y [B, T, n_r] complex128 and
        H [G, N, n_r, n_t] -> U_eq [B, T + pad, 2 n_t], the rows z = sqrt(Pi) N IFFT(X) behind their cyclic prefix and
        `pad` zero rows, Re/Im interleaved -- what an ESN behind the equaliser reads.  X is what mmse_detect_count
        computes, bit for bit (want_xhat adds it, complex128 [B, N, n_t]).  io="f32": the rows rounded to float32."""
        torch, p = self.torch, self.p
        if io not in ("f64", "f32"):
            raise ValueError(f"io must be 'f64' or 'f32', not {io!r}")
        if int(pad) < 0:
            raise ValueError(f"pad = {pad} must be non-negative")
        if int(frames_per_block) < 1:
            raise ValueError(f"frames_per_block = {frames_per_block} must be positive")
        g, b = H.shape[0], y.shape[0]
        if H.dtype != torch.complex128 or tuple(H.shape[1:]) != (p.n_sub, p.n_r, p.n_t):
            raise ValueError(f"H must be complex128 [G, {p.n_sub}, {p.n_r}, {p.n_t}], not {H.dtype} {tuple(H.shape)}")
        if y.dtype != torch.complex128 or tuple(y.shape[1:]) != (p.t_frame, p.n_r):
            raise ValueError(f"y must be complex128 [B, {p.t_frame}, {p.n_r}], not {y.dtype} {tuple(y.shape)}")
        if (b + int(frames_per_block) - 1) // int(frames_per_block) > g:
            raise ValueError(f"{b} frames of {frames_per_block} per block need more than the {g} blocks of H")
        f32 = io == "f32"
        with torch.cuda.device(self.device):
            p_i = self.p_i(ebno_db, g)
            rows = torch.empty((b, p.t_frame + int(pad), 2 * p.n_t), dtype=torch.float32 if f32 else torch.float64,
                               device=self.device)
            xh = torch.empty((b, p.n_sub, p.n_t), dtype=torch.complex128, device=self.device) if want_xhat else None
            name = "esn_mmse_equalize_rows_f32" if f32 else "esn_mmse_equalize_rows"
            check(getattr(self.lib, name)(b, int(frames_per_block), p.n_sub, p.cp, int(pad), p.n_t, p.n_r, ptr(p_i),
                                          p.no, ptr(H.contiguous()), ptr(y.contiguous()), ptr(rows), ptr(xh),
                                          _lib.stream_handle()), name)
        return (rows, xh) if want_xhat else rows

    def track_prior(self, ebno_db):
        """reg [isi] of track_channel: the MAP weight T No / (N Pi r_h[l]) of the exponential prior r_h that
        esn_channel_estimate shrinks with (exp(-l / (cp / 9)) normalised over cp + 1 taps), T = N + cp."""
        import math
        p = self.p
        tc = max(p.cp / 9.0, 1e-12)
        rsum = sum(math.exp(-j / tc) for j in range(p.cp + 1))
        return [p.t_frame * p.no / (p.n_sub * p.p_i(ebno_db) * (math.exp(-l / tc) / rsum)) for l in range(p.isi)]

    def track_channel(self, y_cp, ebno_db, X_hat=None, bits=None, window=1, est_per_group=1, want_taps=False):
        """Decision-directed channel estimate (esn_channel_track): estimate e from the `window` consecutive frames
        e window .. e window + window - 1 of y_cp [n_est window, T, n_r] and the points decided on them -- X_hat complex
        [n_est window, N, n_t] (sliced as the detectors slice) or bits uint8 [n_est window, N m, n_t], exactly one.
        Returns (H [n_est, N, n_r, n_t], status int32 [n_est][, taps [n_est, n_r, n_t, isi]]); a flagged estimate
        (status 1: singular normal equations) is NaN."""
        torch, p = self.torch, self.p
        if (X_hat is None) == (bits is None):
            raise ValueError("track_channel takes exactly one of X_hat and bits")
        if not 1 <= int(window) <= 8:
            raise ValueError(f"window must be in 1..8, not {window}")
        if y_cp.shape[0] % int(window):
            raise ValueError(f"{y_cp.shape[0]} frames are no multiple of window = {window}")
        n_est = y_cp.shape[0] // int(window)
        g = (n_est + int(est_per_group) - 1) // int(est_per_group)
        with torch.cuda.device(self.device):
            p_i = self.p_i(ebno_db, g)
            row = self._track_reg.get(float(ebno_db))      # one upload per Eb/No: the tracking loop calls per data symbol
            if row is None:
                row = self._track_reg[float(ebno_db)] = torch.tensor(self.track_prior(ebno_db), dtype=torch.float64,
                                                                     device=self.device)
            reg = row.repeat(g, 1)
            H = torch.empty((n_est, p.n_sub, p.n_r, p.n_t), dtype=torch.complex128, device=self.device)
            status = torch.empty((n_est,), dtype=torch.int32, device=self.device)
            taps = torch.empty((n_est, p.n_r, p.n_t, p.isi), dtype=torch.complex128, device=self.device) if want_taps \
                else None
            xh = None if X_hat is None else X_hat.contiguous()
            bt = None if bits is None else bits.contiguous()
            check(self.lib.esn_channel_track(ptr(y_cp.contiguous()), ptr(xh), ptr(bt), n_est, int(window),
                                             int(est_per_group), p.n_sub, p.cp, p.n_t, p.n_r, p.isi, p.m, ptr(p_i),
                                             ptr(reg), ptr(taps), ptr(H), ptr(status), _lib.stream_handle()),
                  "esn_channel_track")
        return (H, status, taps) if want_taps else (H, status)

    def channel_metrics(self, H, ebno_db, want_s=False):
        """Per-subcarrier SVD metrics of H [G, N, n_r, n_t] (OFDM_MIMO_2-2_NBF_LDPC.py:369-385; esn_channel_metrics):
        cond [G, N] float64, rank [G, N] uint8, cap [G] float64 (the block's mean capacity per subcarrier), and with
        want_s the singular values S [G, N, min(n_t, n_r)], descending.  Device tensors; nothing is read back."""
        torch, p = self.torch, self.p
        g, n = H.shape[0], H.shape[1]
        if H.dtype != torch.complex128 or tuple(H.shape[2:]) != (p.n_r, p.n_t):
            raise ValueError(f"H must be complex128 [G, N, {p.n_r}, {p.n_t}], not {H.dtype} {tuple(H.shape)}")
        with torch.cuda.device(self.device):
            p_i = self.p_i(ebno_db, g)
            cond = torch.empty((g, n), dtype=torch.float64, device=self.device)
            rank = torch.empty((g, n), dtype=torch.uint8, device=self.device)
            cap = torch.empty((g,), dtype=torch.float64, device=self.device)
            S = torch.empty((g, n, min(p.n_t, p.n_r)), dtype=torch.float64, device=self.device) if want_s else None
            check(self.lib.esn_channel_metrics(g, n, p.n_t, p.n_r, ptr(H.contiguous()), ptr(p_i), p.no, ptr(S),
                                               ptr(cond), ptr(rank), ptr(cap), _lib.stream_handle()),
                  "esn_channel_metrics")
        return (cond, rank, cap, S) if want_s else (cond, rank, cap)


def percentiles_linear(x, qs):
    """np.percentile(x, qs) with its default linear rule, on the tensor's own device: sorted value at the virtual index
    (n - 1) q / 100, interpolated between its two neighbours as NumPy does (a + (b - a) t below the midpoint,
    b - (b - a)(1 - t) from it on).  One torch.sort, no torch.quantile (which refuses large inputs).  Returns a float64
    tensor [len(qs)]."""
    import torch
    v = torch.sort(x.reshape(-1).to(torch.float64)).values
    n = v.numel()
    if n == 0:
        raise ValueError("percentiles of an empty tensor")
    q = torch.tensor([float(a) for a in qs], dtype=torch.float64) / 100.0
    vi = q * (n - 1)                                  # host arithmetic, as NumPy's: the index must not depend on the device
    lo = torch.floor(vi).clamp(0, n - 1)
    t = (vi - lo).to(v.device)
    lo = lo.to(torch.int64).to(v.device)
    hi = (lo + 1).clamp(max=n - 1)
    a, b = v[lo], v[hi]
    d = b - a
    return torch.where(t >= 0.5, b - d * (1 - t), a + d * t)


def summarize_channel_metrics(cond, rank, cap, n_t, n_r):
    """The per-Eb/No channel record of the block-fading drivers (OFDM_MIMO_2-2_NBF_LDPC.py:515-521) from the outputs
    of FrameSource.channel_metrics, reduced on the device; only these four floats are read back."""
    import torch
    pct = percentiles_linear(cond, (50, 90))
    full = rank.reshape(-1).ge(min(n_t, n_r)).to(torch.float64).mean()
    vals = torch.stack([cap.to(torch.float64).mean(), full, pct[0], pct[1]]).cpu().tolist()
    return dict(zip(("capacity_bits_per_sc", "frac_rank_ge_full", "cond_p50", "cond_p90"), vals))


def _view_real(z):
    """complex128 [..., T, n] -> float64 view [..., T, 2n] (Re/Im interleaved; driver:433-436); complex64 ->
    float32."""
    import torch
    z = z.contiguous()
    return torch.view_as_real(z).reshape(*z.shape[:-1], 2 * z.shape[-1])


complex_as_io = _view_real


def pilot_rows(pilot_y, pilot_x, delay, out=None):
    """The zero-padded training rows of pilots: pilot_y complex128 [..., t, n_r] and pilot_x [..., t, n_t] -> float64
    (U [..., t + d, 2 n_r], D [..., t + d, 2 n_t]), d = delay: pilot_y in rows [0, t) of U, the teacher pilot_x in rows
    [d, d + t) of D, zeros elsewhere.  out=(U, D): buffers of that shape to fill instead of new ones (the padding rows
    are never written, so they can be kept between calls).  pilot_y=None: D alone, (None, D)."""
    import torch
    t, d = pilot_x.shape[-2], delay
    U, D = out or (None if z is None else torch.zeros((*z.shape[:-2], t + d, 2 * z.shape[-1]), dtype=torch.float64,
                                                      device=z.device) for z in (pilot_y, pilot_x))
    if pilot_y is not None:
        U[..., :t, :] = _view_real(pilot_y)
    D[..., d:d + t, :] = _view_real(pilot_x)
    return U, D


def group_scalings(g, n_in, in_scale, n_out, t_scale, device):
    """set_scaling's arguments for g groups of one input and one teacher scale: ([g, n_in], None, [g, n_out], None)."""
    import torch
    return (torch.full((g, n_in), in_scale, dtype=torch.float64, device=device), None,
            torch.full((g, n_out), t_scale, dtype=torch.float64, device=device), None)

