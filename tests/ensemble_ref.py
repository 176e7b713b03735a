"""NumPy restatement of the reservoir ensemble (esn_detect_count_ens, ensemble.EnsembleBank): the ordered weighted sum
of the members' outputs, the oracle's tail (time_to_freq / hard_bits) on it, and a K-member OracleESN ensemble whose
members are fitted on the same pilot."""
import numpy as np

from oracle import esn_oracle as eo


def combine(Y, weights=None, frames_per_group=1):
    """Y [K, B, N, 2 n_t] (float64, or float32: widened first) -> [B, N, 2 n_t] float64:
    acc = w[g, 0] y_0, then acc = acc + w[g, k] y_k for k = 1 .. K-1 in this order, every product rounded before the
    add (NumPy float64 does exactly that).  weights [G, K] or None: 1 / K each."""
    Y = np.asarray(Y).astype(np.float64)
    K, B = Y.shape[:2]
    G = (B + frames_per_group - 1) // frames_per_group
    w = np.full((G, K), 1.0 / K) if weights is None else np.asarray(weights, dtype=np.float64)
    wf = w[np.arange(B) // frames_per_group]                 # [B, K]
    acc = wf[:, 0, None, None] * Y[0]
    for k in range(1, K):
        acc = acc + wf[:, k, None, None] * Y[k]
    return acc


def detect(y, p_i, tx_bits, frames_per_group, m):
    """y [B, N, 2 n_t] float64, p_i [G], tx_bits [B, N m, n_t] -> (errors [G], bits [G], X_hat [B, N, 2 n_t]) by the
    oracle's tail, zero output delay."""
    B, N, n2 = y.shape
    n_t = n2 // 2
    G = (B + frames_per_group - 1) // frames_per_group
    const = eo.unit_qam(m)
    err, nb = np.zeros(G, dtype=np.int64), np.zeros(G, dtype=np.int64)
    xh = np.zeros((B, N, n2))
    for f in range(B):
        g = f // frames_per_group
        seqs = [y[f, :, 2 * t] + 1j * y[f, :, 2 * t + 1] for t in range(n_t)]
        X = eo.time_to_freq(seqs, N, p_i[g])
        xh[f, :, 0::2], xh[f, :, 1::2] = X.real, X.imag
        err[g] += eo.count_bit_errors(tx_bits[f], eo.hard_bits(X, const, m))
        nb[g] += N * m * n_t
    return err, nb, xh


def detect_ensemble(Y, p_i, tx_bits, frames_per_group, m, weights=None):
    return detect(combine(Y, weights, frames_per_group), p_i, tx_bits, frames_per_group, m)


class RidgeOracleESN(eo.OracleESN):
    """OracleESN whose read-out is the ridge solution argmin |E W^T - D_s|^2 + ridge |W|^2 in its dual form
    W = D_s^T (E E^T + ridge I)^-1 E (rows < columns at one pilot); ridge None: the reference's pinv."""

    def __init__(self, *args, ridge=None, **kw):
        super().__init__(*args, **kw)
        self.ridge = ridge

    def fit(self, inputs, outputs, transient=0):
        pred = super().fit(inputs, outputs, transient)
        if self.ridge is None:
            return pred
        E = self._ext_states[transient:]
        Ds = self.scale_teacher(np.asarray(outputs))[transient:]
        self.W_out = np.linalg.solve(E @ E.T + self.ridge * np.eye(E.shape[0]), Ds).T @ E
        return self.unscale_teacher(self._ext_states @ self.W_out.T)


class OracleEnsemble:
    """K RidgeOracleESN members of one shape, their weights (and their state noise) drawn one after another from the
    one RandomState; each is fitted on the same pilot and their outputs are averaged before the FFT."""

    def __init__(self, n_members, n_inputs, n_outputs, n_reservoir, random_state, ridge=None, weights=None, **kw):
        self.members = [RidgeOracleESN(n_inputs, n_outputs, n_reservoir, random_state=random_state, ridge=ridge,
                                       weights=None if weights is None else weights[k], **kw)
                        for k in range(n_members)]

    def fit(self, x_in, x_out, transient):
        for m in self.members:
            m.fit(x_in, x_out, transient)

    def predict(self, u, transient):
        """[K, T - transient, n_out]"""
        return np.stack([m.predict(u, transient, continuation=False) for m in self.members])


def ensemble_block_ber(cfg, ebno, block, n_members, n_res, frames, ridge):
    """(errors, bits) of one coherence block of the finding the ensemble rests on: RandomState(7000 + block) gives, in
    this order, the pilot, the members' weights one after another, then the data frames (state noise from the same
    stream as it is consumed); taps from the seed 1234 + int(ebno) + 75 block + 1; fixed delay (min + max) // 2."""
    from oracle.ofdm_frames import make_frame, tdlb_mimo_taps
    n_in, n_out = 2 * cfg.n_r, 2 * cfg.n_t
    rs = np.random.RandomState(7000 + block)
    taps = tdlb_mimo_taps(cfg, 1234 + int(ebno) + block * 75 + 1)
    pilot = make_frame(cfg, ebno, taps, rs)
    ens = OracleEnsemble(n_members, n_in, n_out, n_res, rs, ridge=ridge, spectral_radius=0.9, sparsity=0.1, noise=0.001,
                         input_scaling=cfg.input_scaling(ebno) * np.ones(n_in), input_shift=np.zeros(n_in),
                         teacher_scaling=cfg.teacher_scale * np.ones(n_out), teacher_shift=np.zeros(n_out))
    d = int((cfg.min_delay + cfg.max_delay) // 2)
    x_in, x_out = eo.pack_delay_io(pilot["y_cp"], pilot["x_cp"], d, cfg.n_sub, cfg.cp, cfg.n_t, cfg.n_r)
    forget = d + cfg.cp
    ens.fit(x_in, x_out, forget)
    errs = tot = 0
    p_i = np.array([cfg.p_i(ebno)])
    for _ in range(frames):
        fr = make_frame(cfg, ebno, taps, rs)
        Y = ens.predict(eo.pack_rx(fr["y_cp"], d), forget)[:, None, :cfg.n_sub]          # [K, 1, N, 2 n_t]
        e, nb, _ = detect_ensemble(Y, p_i, fr["bits"][None], 1, cfg.m)
        errs += int(e[0])
        tot += int(nb[0])
    return errs, tot
