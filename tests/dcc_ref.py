"""NumPy restatement of the amplifier-aware LS-MMSE detector (esn_mmse_dcc_detect_count, FrameSource.mmse_dcc_detect_count,
montecarlo.dcc_point): the LS-MMSE solution, then n_iter passes of slice -> re-modulate -> known amplifier -> subtract the
predicted distortion behind the same equaliser.  np.fft and np.linalg.solve, float64 / complex128 throughout.  Beside it
what tests/test_dcc_reference_cpu.py and tests/test_gpu_dcc.py share: the shapes the kernel is held to the model at, their
supplied inputs (made once, never changed) and the model's answers.  No GPU, no torch."""
import functools
import math

import numpy as np

XHAT_BOUND = 1e-9                # X_hat against the model: of max|X_hat| per frame (the project's bound for MMSE X_hat)
MARGIN_MIN = 1e-7                # least slicer margin of the model, in grid spacings: 100 x XHAT_BOUND
LDS_MAX = 150 * 1024

# (N, n_t, n_r, m, cp, n_iter)
SHAPES = [(8, 1, 1, 2, 0, 1), (16, 3, 5, 4, 3, 3), (64, 2, 2, 6, 9, 2), (128, 4, 8, 4, 10, 2), (32, 4, 3, 2, 7, 8)]
BIG_SHAPE = (512, 4, 8, 4, 10, 2)            # 135,168 bytes of LDS: the largest 4x8 shape served
REFUSED_SHAPE = (1024, 4, 8, 4, 10, 2)       # 270,336 bytes
FRAMES, PER_GROUP = 7, 3                     # a ragged last group
CLIP_OVER_RMS = (0.3, 3.0, 0.3)              # a_clip of group g over the transmit signal's rms: heavy, light, heavy
NO = 1e-5


def lds_bytes(n_sub, n_t, n_r):
    return 16 * ((n_r + 2 * n_t) * n_sub + n_sub // 2)


def qam_norm(m):
    side = 1 << (m // 2)
    return side, math.sqrt(2.0 * (side * side - 1) / 3.0)


def slice_levels(X, m):
    """(i, j): the level indices of the grid point nearest each entry of X (det_slice per axis: rint, clamped)."""
    side, norm = qam_norm(m)

    def level(v):
        return np.clip(np.rint((v * norm + (side - 1)) * 0.5), 0, side - 1).astype(np.int64)

    return level(X.real), level(X.imag)


def points_of(i, j, m):
    side, norm = qam_norm(m)
    return ((2 * i - (side - 1)) + 1j * (2 * j - (side - 1))) / norm


def bits_of(i, j, m):
    """[N m, n_t] uint8 of the decisions (i, j) [N, n_t]: index i side + j, natural binary, LSB first."""
    side, _ = qam_norm(m)
    idx = i * side + j
    b = (idx[:, :, None] >> np.arange(m)[None, None, :]) & 1
    return b.transpose(0, 2, 1).reshape(idx.shape[0] * m, idx.shape[1]).astype(np.uint8)


def points_from_bits(bits, n_sub, m):
    """X [N, n_t] of bits [N m, n_t]."""
    side, _ = qam_norm(m)
    idx = (bits.reshape(n_sub, m, -1).astype(np.int64) * (1 << np.arange(m))[None, :, None]).sum(axis=1)
    return points_of(idx // side, idx % side, m)


def amplifier(x, a_clip):
    return x / np.sqrt(1.0 + (np.abs(x) / a_clip) ** 2)


def mmse_apply(H, lam, V):
    """(H_k^H H_k + lam I)^-1 H_k^H V_k per subcarrier: H [N, n_r, n_t], V [N, n_r] -> [N, n_t]."""
    hh = np.conj(np.swapaxes(H, -1, -2))
    return np.linalg.solve(hh @ H + lam * np.eye(H.shape[-1]), hh @ V[:, :, None])[:, :, 0]


def slicer_margin(X, m):
    """Least distance of a Re or Im part of X from a decision boundary, in grid spacings (2 / norm)."""
    side, norm = qam_norm(m)
    v = np.concatenate([X.real.ravel(), X.imag.ravel()]) * norm * 0.5      # levels at the half-odd integers
    bounds = np.arange(-(side - 2), side - 1, 2) * 0.5
    return float(np.abs(v[:, None] - bounds[None, :]).min())


def dcc_frame(y_cp, H, p_i, a_clip, no, cp, m, n_iter, decisions=None):
    """X^0 .. X^{n_iter}, each [N, n_t], of one frame y_cp [cp + N, n_r] under H [N, n_r, n_t].  decisions: the points
    S [N, n_t] every pass re-modulates instead of its own slicer's (a genie, for the model's own checks)."""
    n = y_cp.shape[0] - cp
    lam, sp = no / p_i, math.sqrt(p_i)
    Y = np.fft.fft(y_cp[cp:], axis=0) / n
    X0 = mmse_apply(H, lam, Y) / sp
    out = [X0]
    for _ in range(n_iter):
        S = points_of(*slice_levels(out[-1], m), m) if decisions is None else decisions
        xt = sp * n * np.fft.ifft(S, axis=0)
        d = amplifier(xt, a_clip) - xt
        D = np.fft.fft(d, axis=0) / (n * sp)
        HD = (H @ D[:, :, None])[:, :, 0]
        out.append(X0 - mmse_apply(H, lam, HD))
    return out


def dcc_batch(y_cp, H, p_i, a_clip, no, cp, m, n_iter, tx_bits=None, frames_per_group=1):
    """The batch: y_cp [B, cp + N, n_r], H [G, N, n_r, n_t], p_i and a_clip [G], tx_bits [B, N m, n_t] or None.
    Returns dict(X [B, n_iter + 1, N, n_t], err_iter [G, n_iter + 1], err [G], bits [G], margin): the counters as the
    entry point adds them up, and the least slicer margin of any X^{it}, it < n_iter (inf at n_iter = 0)."""
    b, g = y_cp.shape[0], H.shape[0]
    n_sub, n_t = H.shape[1], H.shape[3]
    X = np.zeros((b, n_iter + 1, n_sub, n_t), dtype=np.complex128)
    err_iter, nbits, margin = np.zeros((g, n_iter + 1), dtype=np.int64), np.zeros(g, dtype=np.int64), math.inf
    for f in range(b):
        q = f // frames_per_group
        xs = dcc_frame(y_cp[f], H[q], p_i[q], a_clip[q], no, cp, m, n_iter)
        for it, x in enumerate(xs):
            X[f, it] = x
            if it < n_iter:
                margin = min(margin, slicer_margin(x, m))
            if tx_bits is not None:
                err_iter[q, it] += int((bits_of(*slice_levels(x, m), m) != tx_bits[f]).sum())
        if tx_bits is not None:
            nbits[q] += tx_bits[f].size
    return dict(X=X, err_iter=err_iter, err=err_iter[:, -1].copy(), bits=nbits, margin=margin)


# ---- supplied inputs of a shape, made once ---------------------------------------------------------------------------
def transmit(X, p_i, a_clip, cp):
    """(x_cp pre-amplifier, x_cp behind the amplifier) [cp + N, n_t] of the points X [N, n_t]: the frame recipe."""
    n = X.shape[0]
    x = math.sqrt(p_i) * n * np.fft.ifft(X, axis=0)
    x_cp = np.concatenate([x[n - cp:], x], axis=0)
    return x_cp, amplifier(x_cp, a_clip)


def through_channel(x_pa, taps):
    """y [T, n_r] = sum_tx taps[rx, tx] * x_pa[:, tx], zero initial state; taps [n_r, n_t, L]."""
    t, (n_r, n_t, _) = x_pa.shape[0], taps.shape
    y = np.zeros((t, n_r), dtype=np.complex128)
    for rx in range(n_r):
        for tx in range(n_t):
            y[:, rx] += np.convolve(x_pa[:, tx], taps[rx, tx])[:t]
    return y


@functools.lru_cache(maxsize=None)
def inputs(shape, frames=FRAMES, per_group=PER_GROUP, seed=0):
    """The supplied inputs of (N, n_t, n_r, m, cp, n_iter): per group a channel of cp + 1 exponentially decaying taps, its
    own Pi (20, 23.5, 27 dB over NO ..) and a clip level of CLIP_OVER_RMS times the transmit rms sqrt(Pi N); frames of
    random bits through amplifier, channel and noise; H the true channel's DFT, a few per cent off (an estimate is).
    RandomState(4242 + N + 10 n_t + n_r + seed)."""
    n, n_t, n_r, m, cp, n_iter = shape
    rs = np.random.RandomState(4242 + n + 10 * n_t + n_r + seed)
    g = (frames + per_group - 1) // per_group
    t = n + cp
    p_i = np.array([NO * 10.0 ** ((20.0 + 3.5 * q) / 10.0) for q in range(g)])
    a_clip = np.array([CLIP_OVER_RMS[q % len(CLIP_OVER_RMS)] * math.sqrt(p_i[q] * n) for q in range(g)])
    pdp = np.exp(-np.arange(cp + 1) / max(cp / 3.0, 1e-12))
    pdp /= pdp.sum()
    taps = (rs.randn(g, n_r, n_t, cp + 1) + 1j * rs.randn(g, n_r, n_t, cp + 1)) * np.sqrt(pdp / 2.0)
    H_true = np.fft.fft(taps, n, axis=-1).transpose(0, 3, 1, 2)                      # [G, N, n_r, n_t]
    H = H_true * (1.0 + 0.03 * (rs.randn(*H_true.shape) + 1j * rs.randn(*H_true.shape)))
    bits = (rs.rand(frames, n * m, n_t) > 0.5).astype(np.uint8)
    y = np.zeros((frames, t, n_r), dtype=np.complex128)
    for f in range(frames):
        q = f // per_group
        _, x_pa = transmit(points_from_bits(bits[f], n, m), p_i[q], a_clip[q], cp)
        y[f] = through_channel(x_pa, taps[q]) + math.sqrt(t * NO / 2.0) * (rs.randn(t, n_r) + 1j * rs.randn(t, n_r))
    out = dict(p_i=p_i, a_clip=a_clip, taps=taps, H_true=np.ascontiguousarray(H_true), H=np.ascontiguousarray(H),
               bits=bits, y=y)
    for a in out.values():
        a.setflags(write=False)
    out.update(shape=shape, per_group=per_group)
    return out


@functools.lru_cache(maxsize=None)
def answers(shape, frames=FRAMES, per_group=PER_GROUP, seed=0):
    """dcc_batch of inputs(shape, ...)."""
    d = inputs(shape, frames, per_group, seed)
    _, _, _, m, cp, n_iter = shape
    return dcc_batch(d["y"], d["H"], d["p_i"], d["a_clip"], NO, cp, m, n_iter, d["bits"], per_group)


# ---- the finding dcc_point's device test asserts, on the oracle's frames ---------------------------------------------
POINT_SEED, POINT_EBNO, POINT_BLOCKS, POINT_FRAMES, POINT_GAIN = 11, 21.0, 16, 8, 5


def oracle_point_errors(n_iter, ebno=POINT_EBNO, blocks=POINT_BLOCKS, frames=POINT_FRAMES, seed=POINT_SEED):
    """Bit errors after 0 .. n_iter passes, [n_iter + 1], and the bits: 4x8 / TDL-B / N = 128 / 16-QAM frames and the
    pilot's LS-MMSE channel estimate of oracle/, block b from RandomState(7000 + 1000 seed + b) and the taps of seed
    1234 + int(ebno) + 75 (1000 seed + b) + 1."""
    from oracle import baselines as bl
    from oracle.ofdm_frames import LinkConfig, make_frame, tdlb_mimo_taps
    cfg = LinkConfig()
    p_i, a_clip = cfg.p_i(ebno), cfg.a_clip(ebno)
    errs, nbits = np.zeros(n_iter + 1, dtype=np.int64), 0
    for b in range(blocks):
        blk = 1000 * seed + b
        rs = np.random.RandomState(7000 + blk)
        taps = tdlb_mimo_taps(cfg, 1234 + int(ebno) + blk * 75 + 1)
        pilot = bl.pilot_frames(cfg, ebno, taps, rs)
        H = bl.estimate_channel(cfg, ebno, pilot["X_LS"], pilot["y_ls_cp"])
        for _ in range(frames):
            fr = make_frame(cfg, ebno, taps, rs)
            for it, x in enumerate(dcc_frame(fr["y_cp"], H, p_i, a_clip, cfg.no, cfg.cp, cfg.m, n_iter)):
                errs[it] += int((bits_of(*slice_levels(x, cfg.m), cfg.m) != fr["bits"]).sum())
            nbits += fr["bits"].size
    return errs, nbits
