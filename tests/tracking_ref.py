"""The tracked loop of DetectorSweep(track=...) for ONE coherence block on the CPU oracle (oracle.esn_oracle.OracleESN):
fit on the pilot, then for data symbol k = 0 .. F - 1 detect it with the current read-out (detect_frame, offset 0), and
unless it is the last one harvest it against a teacher -- the re-modulated decisions (tests/remod_ref.py) or, for
"genie", the frame's own transmit signal -- and solve the read-out again over the rows [forget, T + d) of the most recent
`track_window` training sets (the pilot is one), by np.linalg.pinv or the ridge normal equations.  OracleESN.fit gives
the states (_ext_states); its own W_out is replaced by the stacked solve."""
import numpy as np

import remod_ref
from oracle import esn_oracle as eo


def boundary_margin(x_hat, m):
    """smallest distance of Re / Im of any element of x_hat to a decision boundary of the unit-power grid"""
    side, norm = remod_ref.slicer_constants(m)
    bnd = (2.0 * (np.arange(side - 1) + 0.5) - (side - 1)) / norm
    v = np.concatenate([x_hat.real.ravel(), x_hat.imag.ravel()])
    return float(np.abs(v[:, None] - bnd[None, :]).min())


def stacked_solve(window, ridge=None):
    """window: [(E rows, scaled teacher rows)] -> W_out [n_out, cols]"""
    E = np.vstack([w[0] for w in window])
    D = np.vstack([w[1] for w in window])
    if ridge is None:
        return (np.linalg.pinv(E) @ D).T, E
    return np.linalg.solve(E.T @ E + ridge * np.eye(E.shape[1]), E.T @ D).T, E


def track_block(esn, pilot_y, pilot_x, data_y, data_bits, data_x, n_sub, cp, n_t, n_r, delay, p_i, m,
                track, track_window, ridge=None):
    """esn: an OracleESN (weights, scalings, noise 0).  pilot_y [T, n_r], pilot_x [T, n_t], data_y [F, T, n_r],
    data_bits [F, N m, n_t], data_x [F, T, n_t] (read for "genie" only).  Returns dict(errors int [F], x_hat [F, N, n_t],
    margin (boundary_margin over all symbols), cond [fits]: cond of every stacked E, W_out: the last read-out)."""
    forget, const, F = delay + cp, eo.unit_qam(m), len(data_y)
    dvec = np.full(2 * n_t, delay)
    x_in, x_out = eo.pack_delay_io(pilot_y, pilot_x, delay, n_sub, cp, n_t, n_r)
    esn.fit(x_in, x_out, forget)
    window = [(esn._ext_states[forget:], esn.scale_teacher(x_out)[forget:])]
    W_out, E = stacked_solve(window, ridge)
    esn.W_out = W_out
    errors, x_hats, conds = [], [], [np.linalg.cond(E)]
    for k in range(F):
        x_hat, bits = eo.detect_frame(esn, data_y[k], dvec, delay, delay, forget, n_sub, n_t, p_i, const, m)
        errors.append(eo.count_bit_errors(np.asarray(data_bits[k]).astype(int), bits))
        x_hats.append(x_hat)
        if k == F - 1:
            break
        if track == "genie":
            teacher = eo.pack_delay_io(data_y[k], data_x[k], delay, n_sub, cp, n_t, n_r)[1]
        else:
            idx = np.argmin(np.abs(x_hat[:, :, None] - const[None, None, :]), axis=2)          # hard_bits' decision
            teacher = remod_ref.remodulate(idx[None], m, np.array([p_i]), cp, delay)[0]
        u = eo.pack_rx(data_y[k], delay)
        esn.fit(u, teacher, forget)                                                            # (for the states)
        window = (window + [(esn._ext_states[forget:], esn.scale_teacher(teacher)[forget:])])[-track_window:]
        esn.W_out, E = stacked_solve(window, ridge)
        conds.append(np.linalg.cond(E))
    x_hats = np.stack(x_hats)
    return dict(errors=np.array(errors), x_hat=x_hats, margin=boundary_margin(x_hats, m), cond=np.array(conds),
                W_out=esn.W_out)
