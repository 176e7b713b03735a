"""NumPy restatement of the equaliser's time-domain rows (esn_mmse_equalize_rows, FrameSource.equalize_rows) and of the
chain behind them (montecarlo.equalized_esn_point): rows -> OracleESN with supplied weights, ridge read-out in the primal
or dual form -> time_to_freq -> hard_bits.  float64 / complex128 throughout."""
import math

import numpy as np

from oracle import esn_oracle as eo


def spectrum(y_cp, cp):
    """Y [N, n_r]: Y_k[rx] = (1/N) sum_i y[cp + i][rx] e^{-2 pi i ik/N}."""
    n = y_cp.shape[0] - cp
    return np.fft.fft(y_cp[cp:], axis=0) / n


def solve(Y, H, p_i, no):
    """X [N, n_t]: X_k = (H_k^H H_k + (no / Pi) I)^-1 H_k^H Y_k / sqrt(Pi), H [N, n_r, n_t]."""
    n, _, n_t = H.shape
    X = np.zeros((n, n_t), dtype=np.complex128)
    for k in range(n):
        hh = H[k].conj().T
        X[k] = np.linalg.solve(hh @ H[k] + (no / p_i) * np.eye(n_t), hh @ Y[k]) / math.sqrt(p_i)
    return X


def time_signal(X, p_i):
    """z [N, n_t]: z_i[tx] = sqrt(Pi) sum_k X_k[tx] e^{+2 pi i ik/N}, the sum written out (the exponent reduced mod N
    before the product with 2 pi / N, so that it is as exact at N = 2048 as at N = 4)."""
    n = X.shape[0]
    ik = np.outer(np.arange(n), np.arange(n)) % n
    return math.sqrt(p_i) * (np.exp(2j * np.pi * ik / n) @ X)


def rows_of(z, cp, pad):
    """[cp + N + pad, 2 n_t]: the last cp samples of z, z, pad zero rows; Re/Im interleaved per antenna."""
    n, n_t = z.shape
    zc = np.concatenate([z[n - cp:], z, np.zeros((pad, n_t), dtype=z.dtype)], axis=0)
    out = np.zeros((cp + n + pad, 2 * n_t))
    out[:, 0::2], out[:, 1::2] = zc.real, zc.imag
    return out


def equalize_frame(y_cp, H, p_i, no, cp, pad=0):
    """(X [N, n_t], rows [cp + N + pad, 2 n_t]) of one frame y_cp [cp + N, n_r] under H [N, n_r, n_t]."""
    X = solve(spectrum(y_cp, cp), H, p_i, no)
    return X, rows_of(time_signal(X, p_i), cp, pad)


def equalize(y_cp, H, p_i, no, cp, pad=0, frames_per_group=1):
    """The batch: y_cp [B, cp + N, n_r], H [G, N, n_r, n_t], p_i [G]; frame f belongs to group f // frames_per_group.
    Returns (X [B, N, n_t], rows [B, cp + N + pad, 2 n_t])."""
    out = [equalize_frame(y_cp[f], H[f // frames_per_group], p_i[f // frames_per_group], no, cp, pad)
           for f in range(y_cp.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


class RidgeESN(eo.OracleESN):
    """OracleESN whose read-out is argmin |E W^T - D_s|^2 + ridge |W|^2 over rows [transient, T): the primal form
    (E^T E + ridge I)^-1 E^T D_s where the rows are at least the columns, else the dual one E^T (E E^T + ridge I)^-1 D_s;
    ridge None: the reference's pinv."""

    def __init__(self, *args, ridge=None, **kw):
        super().__init__(*args, **kw)
        self.ridge = ridge

    def fit(self, inputs, outputs, transient=0):
        pred = super().fit(inputs, outputs, transient)
        if self.ridge is None:
            return pred
        E = self._ext_states[transient:]
        Ds = self.scale_teacher(np.asarray(outputs))[transient:]
        if E.shape[0] >= E.shape[1]:
            self.W_out = np.linalg.solve(E.T @ E + self.ridge * np.eye(E.shape[1]), E.T @ Ds).T
        else:
            self.W_out = np.linalg.solve(E @ E.T + self.ridge * np.eye(E.shape[0]), Ds).T @ E
        return self.unscale_teacher(self._ext_states @ self.W_out.T)


def make_esn(n_t, n_res, in_scale, t_scale, ridge, noise=0.0, weights=None, random_state=None, spectral_radius=0.9,
             sparsity=0.1):
    n_io = 2 * n_t
    return RidgeESN(n_io, n_io, n_res, spectral_radius=spectral_radius, sparsity=sparsity, noise=noise,
                    input_scaling=in_scale * np.ones(n_io), input_shift=np.zeros(n_io),
                    teacher_scaling=t_scale * np.ones(n_io), teacher_shift=np.zeros(n_io), weights=weights,
                    random_state=random_state, ridge=ridge)


def chain_block(esn, pilot_rows, pilot_x_cp, data_rows, n_sub, cp, delay, p_i, m):
    """One coherence block behind the equaliser: `esn` is fitted on the pilot's rows [cp + N + delay, 2 n_t] against the
    pre-PA pilot x_cp [cp + N, n_t] delayed by `delay` rows (transient delay + cp), then every frame of data_rows
    [F, cp + N + delay, 2 n_t] is predicted from a zero state and taken to the frequency domain.
    Returns (X_hat [F, N, n_t], bits [F, N m, n_t])."""
    n_t = pilot_x_cp.shape[1]
    t = n_sub + cp
    teacher = np.zeros((t + delay, 2 * n_t))
    teacher[delay:delay + t, 0::2], teacher[delay:delay + t, 1::2] = pilot_x_cp.real, pilot_x_cp.imag
    esn.fit(pilot_rows, teacher, delay + cp)
    const = eo.unit_qam(m)
    xs, bits = [], []
    for u in data_rows:
        y = esn.predict(u, delay + cp, continuation=False)
        X = eo.time_to_freq([y[:n_sub, 2 * a] + 1j * y[:n_sub, 2 * a + 1] for a in range(n_t)], n_sub, p_i)
        xs.append(X)
        bits.append(eo.hard_bits(X, const, m))
    return np.stack(xs), np.stack(bits)


def slicer_margin(X, m):
    """The smallest distance of a component of X from a decision threshold of the unit-power square QAM grid (the
    outermost levels have none beyond them)."""
    side = 1 << (m // 2)
    norm = math.sqrt(2.0 * (side * side - 1) / 3.0)
    v = np.concatenate([X.real.ravel(), X.imag.ravel()]) * norm          # levels at the odd integers
    thresholds = np.arange(-(side - 2), side - 1, 2)
    if thresholds.size == 0:
        return float(np.min(np.abs(v)) / norm)
    return float(np.min(np.abs(v[:, None] - thresholds[None, :])) / norm)


def block_errors(cfg, ebno, block, n_res, frames, ridge, delay=0, noise=0.001):
    """(ESN errors, MMSE errors, bits) of one coherence block of the finding the feature rests on, all on the oracle:
    RandomState(7000 + block) gives the pilot (with its sparse LS companion) and then the data frames, the taps come
    from the seed 1234 + int(ebno) + 75 block + 1, the reservoir and its state noise from RandomState(9000 + block);
    the LS-MMSE channel estimate of the pilot equalises pilot and data."""
    from oracle import baselines as bl
    from oracle.ofdm_frames import make_frame, tdlb_mimo_taps
    rs = np.random.RandomState(7000 + block)
    taps = tdlb_mimo_taps(cfg, 1234 + int(ebno) + block * 75 + 1)
    p_i = cfg.p_i(ebno)
    pilot = bl.pilot_frames(cfg, ebno, taps, rs)
    H = bl.estimate_channel(cfg, ebno, pilot["X_LS"], pilot["y_ls_cp"])
    esn = make_esn(cfg.n_t, n_res, cfg.input_scaling(ebno), cfg.teacher_scale, ridge, noise=noise,
                   random_state=np.random.RandomState(9000 + block))
    _, pilot_rows = equalize_frame(pilot["y_cp"], H, p_i, cfg.no, cfg.cp, delay)
    frames_ = [make_frame(cfg, ebno, taps, rs) for _ in range(frames)]
    eq = [equalize_frame(fr["y_cp"], H, p_i, cfg.no, cfg.cp, delay) for fr in frames_]
    const = eo.unit_qam(cfg.m)
    _, bits = chain_block(esn, pilot_rows, pilot["x_cp"], [e[1] for e in eq], cfg.n_sub, cfg.cp, delay, p_i, cfg.m)
    e_esn = sum(eo.count_bit_errors(fr["bits"], b) for fr, b in zip(frames_, bits))
    e_mm = sum(eo.count_bit_errors(fr["bits"], eo.hard_bits(e[0], const, cfg.m)) for fr, e in zip(frames_, eq))
    return e_esn, e_mm, sum(fr["bits"].size for fr in frames_)
