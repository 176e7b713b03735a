"""Running normal equations in NumPy float64 (a helper of test_gram_reference_cpu / test_gpu_gram /
test_gpu_gram_tracking, not a test): the state of esn_gram_accumulate, the solve of esn_gram_solve, the explicitly
weighted stacked fit they must equal, and the bounds the tests hold them to.

Conventions (multipilot_ref's): E [rows, cols] are extended states with the transient already cut, Ds [rows, n_out] the
SCALED teacher, G [cols, cols], C [n_out, cols], W [n_out, cols], lam >= 0 absolute."""
import numpy as np

EPS = 2.0 ** -52


def accumulate(E, Ds, state=None, decay=1.0):
    """(G, C) <- (decay G + E^T E, decay C + Ds^T E); state None starts a new sum."""
    G, C = E.T @ E, Ds.T @ E
    if state is None or decay == 0.0:
        return G, C
    return decay * state[0] + G, decay * state[1] + C


def solve(G, C, lam):
    """W [n_out, cols] of (G + lam I) W^T = C^T."""
    return np.linalg.solve(G + lam * np.eye(G.shape[0]), C.T).T


def weighted_stack(segments, gamma):
    """segments: [(E, Ds)], oldest first.  The rows of segment s scaled by gamma^(age / 2), age = 0 for the newest, so
    that the stacked Gram matrix is sum_s gamma^age E_s^T E_s; a segment whose weight is 0 is left out."""
    n = len(segments)
    w = [float(gamma) ** ((n - 1 - s) / 2.0) if (gamma > 0.0 or s == n - 1) else 0.0 for s in range(n)]
    keep = [s for s in range(n) if w[s] > 0.0]
    return np.vstack([w[s] * segments[s][0] for s in keep]), np.vstack([w[s] * segments[s][1] for s in keep])


def stacked_ridge(E, Ds, lam):
    """The dual route to the same W: the least-squares solution of [E; sqrt(lam) I] W^T = [Ds; 0] by an SVD
    (multipilot_ref.ridge's formula), which never forms E^T E."""
    U, s, Vt = np.linalg.svd(E, full_matrices=False)
    live = s > np.finfo(np.float64).eps * max(E.shape) * s[0]
    f = np.where(live, s / np.where(live, s * s + lam, 1.0), 0.0)
    return ((Vt.T * f) @ (U.T @ Ds)).T


def cond_aug(E, lam):
    """cond([E; sqrt(lam) I]) from the singular values of E: those of the augmented matrix are sqrt(s^2 + lam), with
    cols - rank(E) further ones equal to sqrt(lam)."""
    s = np.linalg.svd(E, compute_uv=False)
    s2 = np.concatenate([s * s, np.zeros(max(0, E.shape[1] - len(s)))]) + lam
    return float(np.sqrt(s2.max() / s2.min())) if s2.min() > 0.0 else np.inf


def primal_bound(E, lam):
    """How far (relative to max |W|) the normal-equations solution may sit from the stacked one: 10 cond^2 eps."""
    return 10.0 * cond_aug(E, lam) ** 2 * EPS


def accumulate_bound(rows, max_e, max_d, prior=0.0, factor=4.0):
    """Per element of G and C: a dot product of `rows` terms of size <= max_e * max(max_e, max_d) carries at most
    rows eps of that in any summation order; the device and NumPy each carry one, the scaled teacher is rounded twice
    more on either side (factor 4 covers the sum), and a decayed prior state of size `prior` adds two roundings."""
    return factor * (rows * EPS * max_e * max(max_e, max_d) + 2.0 * EPS * prior)


def track_block_gram(esn, pilots_y, pilots_x, data_y, data_bits, data_x, n_sub, cp, n_t, n_r, delay, p_i, m, track, gamma,
                     lam=None, grid=None):
    """The loop of DetectorSweep(solve_method="gram") for ONE coherence block on the CPU oracle (tracking_ref.track_block
    is its stacked-rows twin).  esn: an OracleESN (weights, scalings, noise 0); pilots_y [P, T, n_r], pilots_x [P, T, n_t];
    data_y [F, T, n_r], data_bits [F, N m, n_t], data_x [F, T, n_t] (read for "genie" only).  Every pilot is accumulated
    with decay 1; `grid` (P >= 2) solves the candidates from pilots 0 .. P - 2, scores them on pilot P - 1
    (multipilot_ref) and keeps the winner as the block's lambda.  track None: the pilot fit detects every symbol;
    "decisions" / "genie": after data symbol k its rows are accumulated with decay gamma and the read-out solved again.
    Returns dict(errors int [F], x_hat [F, N, n_t], margin, cond [fits] of the weighted stacks [E; sqrt(lam) I], lam,
    choice, scores, score_bound, W_out)."""
    import multipilot_ref
    import remod_ref
    import tracking_ref
    from oracle import esn_oracle as eo
    forget, const, F = delay + cp, eo.unit_qam(m), len(data_y)
    dvec = np.full(2 * n_t, delay)
    segs, state = [], None
    choice = scores = sbound = None
    for q in range(len(pilots_y)):
        x_in, x_out = eo.pack_delay_io(pilots_y[q], pilots_x[q], delay, n_sub, cp, n_t, n_r)
        esn.fit(x_in, x_out, forget)                                                           # (for the states)
        E, Ds = esn._ext_states[forget:].copy(), esn.scale_teacher(x_out)[forget:]
        if grid is not None and q == len(pilots_y) - 1:
            W = np.stack([solve(*state, float(l)) for l in grid])
            scores = multipilot_ref.holdout_scores(E, Ds, W)
            sbound = multipilot_ref.score_bound(E, Ds, W)
            choice = multipilot_ref.choose(scores)
            lam = float(grid[choice])
        segs.append((E, Ds))
        state = accumulate(E, Ds, state, 1.0)
    weights = [1.0] * len(segs)                 # the weight of every segment's Gram matrix in the state

    def stack():
        keep = [s for s in range(len(segs)) if weights[s] > 0.0]
        return np.vstack([np.sqrt(weights[s]) * segs[s][0] for s in keep])

    esn.W_out = solve(*state, lam)
    errors, x_hats, conds = [], [], [cond_aug(stack(), lam)]
    for k in range(F):
        x_hat, bits = eo.detect_frame(esn, data_y[k], dvec, delay, delay, forget, n_sub, n_t, p_i, const, m)
        errors.append(eo.count_bit_errors(np.asarray(data_bits[k]).astype(int), bits))
        x_hats.append(x_hat)
        if k == F - 1 or track is None:
            continue
        if track == "genie":
            teacher = eo.pack_delay_io(data_y[k], data_x[k], delay, n_sub, cp, n_t, n_r)[1]
        else:
            idx = np.argmin(np.abs(x_hat[:, :, None] - const[None, None, :]), axis=2)          # hard_bits' decision
            teacher = remod_ref.remodulate(idx[None], m, np.array([p_i]), cp, delay)[0]
        esn.fit(eo.pack_rx(data_y[k], delay), teacher, forget)                                 # (for the states)
        E, Ds = esn._ext_states[forget:].copy(), esn.scale_teacher(teacher)[forget:]
        state = accumulate(E, Ds, state, gamma)
        weights = [w * gamma for w in weights] + [1.0]
        segs.append((E, Ds))
        esn.W_out = solve(*state, lam)
        conds.append(cond_aug(stack(), lam))
    x_hats = np.stack(x_hats)
    return dict(errors=np.array(errors), x_hat=x_hats, margin=tracking_ref.boundary_margin(x_hats, m),
                cond=np.array(conds), lam=lam, choice=choice, scores=scores, score_bound=sbound, W_out=esn.W_out)
