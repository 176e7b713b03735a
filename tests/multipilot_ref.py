"""Several pilots per coherence block in NumPy float64 (a helper of test_holdout_reference_cpu / test_gpu_holdout /
test_gpu_multipilot, not a test): the hold-out score and choice of esn_readout_holdout_score as DESIGN 3.3d defines
them, the P-pilot fit of ReservoirBank.fit_pilots, and the experiment behind the section on the CPU oracle.

Conventions: E [rows, cols] are extended states with the transient already cut, Ds [rows, n_out] the SCALED teacher,
W [L, n_out, cols] candidate read-outs, lam >= 0 absolute (units of the Gram matrix of the scaled states)."""
import numpy as np

GRID = (1e-5, 1e-4, 1e-3, 1e-2, 1e-1)      # candidates of the oracle experiment and the sweep tests


def holdout_scores(E, Ds, W, status=None):
    """score[l] = sum_i sum_o (E W[l]^T - Ds)[i, o]^2; +inf where status[l] != 0 or the sum is not finite."""
    out = np.full(len(W), np.inf)
    for l, w in enumerate(W):
        if status is not None and status[l] != 0:
            continue
        with np.errstate(all="ignore"):
            r = E @ w.T - Ds
            s = float(np.sum(r * r))
        if np.isfinite(s):
            out[l] = s
    return out


def choose(scores):
    """The lowest index with the smallest finite score, -1 if there is none."""
    return int(np.argmin(scores)) if np.any(np.isfinite(scores)) else -1


def score_bound(E, Ds, W):
    """[L]: how far a float64 evaluation of score[l] in any summation order may sit from the exact value.  Each
    residual is a dot product of `cols` terms, one scaling and one subtraction: |r - r_exact| <= b[i, o] =
    (cols + 2) 2^-53 (sum_c |E[i, c] W[l, o, c]| + |Ds[i, o]|); then |sum r^2 - sum r_exact^2| <= 2 sqrt(score) |b|_2
    + |b|_2^2 (Cauchy-Schwarz; the rounding of the outer sum is second order beside it)."""
    u = (E.shape[1] + 2) * 2.0 ** -53
    out = np.zeros(len(W))
    for l, w in enumerate(W):
        b = u * (np.abs(E) @ np.abs(w).T + np.abs(Ds))
        nb = float(np.sqrt(np.sum(b * b)))
        r = E @ w.T - Ds
        out[l] = 2.0 * float(np.sqrt(np.sum(r * r))) * nb + nb * nb
    return out


def ridge(E, Ds, lam):
    """[n_out, cols] = argmin |E W^T - Ds|^2 + lam |W|^2 by an SVD; lam = 0 is the pinv solve (NumPy's rank cut)."""
    U, s, Vt = np.linalg.svd(E, full_matrices=False)
    live = s > np.finfo(np.float64).eps * max(E.shape) * s[0]
    f = np.where(live, s / np.where(live, s * s + lam, 1.0), 0.0)
    return ((Vt.T * f) @ (U.T @ Ds)).T


def fit_pilots(Es, Dss, lam=None, grid=None):
    """Es, Dss: P arrays [rows, cols] / [rows, n_out], one per pilot.  lam (None: pinv) fits all P stacked.  grid with
    P >= 2: candidates fitted on pilots 0 .. P - 2, scored on pilot P - 1, the winner refitted on all P.  Returns
    dict(W_out, choice, scores, lam)."""
    E_all, D_all = np.concatenate(Es), np.concatenate(Dss)
    if grid is None:
        return dict(W_out=ridge(E_all, D_all, 0.0 if lam is None else float(lam)), choice=None, scores=None, lam=lam)
    if len(Es) < 2:
        raise ValueError("the hold-out choice needs two pilots")
    E_fit, D_fit = np.concatenate(Es[:-1]), np.concatenate(Dss[:-1])
    W = np.stack([ridge(E_fit, D_fit, float(l)) for l in grid])
    scores = holdout_scores(Es[-1], Dss[-1], W)
    c = choose(scores)
    if c < 0:
        return dict(W_out=np.zeros_like(W[0]), choice=-1, scores=scores, lam=np.nan)
    return dict(W_out=ridge(E_all, D_all, float(grid[c])), choice=c, scores=scores, lam=float(grid[c]))


def oracle_finding(n_pilots_max=4, n_blocks=2, n_frames=6, ebno=21.0, n_res=512, seed=0, grid=GRID, cases=None):
    """BER of the CPU oracle at 4x8 TDL-B, 16-QAM, delay 3, state noise 1e-3, a fresh reservoir per block: every pilot
    harvested from a zero state (OracleESN states), rows [forget, T + d) of the pilots stacked into one solve.  Returns
    {(P, fit): BER} for P = 1 .. n_pilots_max and fit in "pinv", "grid" (P >= 2: the hold-out choice), each over the
    same n_blocks x n_frames data frames; `cases` keeps only those keys."""
    from oracle import esn_oracle as eo
    from oracle.ofdm_frames import LinkConfig, make_frame, tdlb_mimo_taps
    cfg = LinkConfig()
    n_in, n_out, d = 2 * cfg.n_r, 2 * cfg.n_t, cfg.delay
    forget, const = d + cfg.cp, eo.unit_qam(cfg.m)
    errs, bits = {}, 0
    for b in range(n_blocks):
        rs = np.random.RandomState(7000 + 131 * seed + b)
        taps = tdlb_mimo_taps(cfg, 1234 + 75 * b + seed)
        esn = eo.OracleESN(n_in, n_out, n_res, spectral_radius=0.9, sparsity=0.1, noise=0.001,
                           input_scaling=cfg.input_scaling(ebno) * np.ones(n_in),
                           teacher_scaling=cfg.teacher_scale * np.ones(n_out), random_state=rs)
        Es, Dss = [], []
        for _ in range(n_pilots_max):
            pilot = make_frame(cfg, ebno, taps, rs)
            x_in, x_out = eo.pack_delay_io(pilot["y_cp"], pilot["x_cp"], d, cfg.n_sub, cfg.cp, cfg.n_t, cfg.n_r)
            esn.fit(x_in, x_out, forget)                   # (its own W_out is not used: the states are)
            Es.append(esn._ext_states[forget:].copy())
            Dss.append(esn.scale_teacher(x_out)[forget:])
        frames = [make_frame(cfg, ebno, taps, rs) for _ in range(n_frames)]
        fits = {}
        for P in range(1, n_pilots_max + 1):
            for fit in ("pinv", "grid")[:1 if P < 2 else 2]:
                if cases is None or (P, fit) in cases:
                    fits[P, fit] = fit_pilots(Es[:P], Dss[:P], grid=grid if fit == "grid" else None)["W_out"]
        for key, W_out in fits.items():
            esn.W_out = W_out
            for fr in frames:
                y = esn.predict(eo.pack_rx(fr["y_cp"], d), forget, continuation=False)
                x_hat = eo.time_to_freq(eo.outputs_to_time_signals(y, np.full(n_out, d), d, cfg.n_sub, cfg.n_t),
                                        cfg.n_sub, cfg.p_i(ebno))
                errs[key] = errs.get(key, 0) + eo.count_bit_errors(fr["bits"], eo.hard_bits(x_hat, const, cfg.m))
        bits += sum(fr["bits"].size for fr in frames)
    return {k: v / bits for k, v in errs.items()}
