"""NumPy restatement of esn_channel_track (include/esn_hip.h): np.fft, the slicer of tests/remod_ref.py, np.linalg.

    Y_f[k, r] = (1/N) FFT_N(y_f[cp:, r])[k] / sqrt(Pi)
    X_f[k, t] = unit_qam[idx], idx sliced from X_hat or read from bits (natural binary, LSB first)
    R[t, t', d] = sum_f sum_k conj(X_f[k, t]) X_f[k, t'] w^{kd},  d = 0 .. L - 1,  w = exp(-2 pi i / N)
    G[(t,l),(t',l')] = R[t, t', l' - l] (l' >= l), conj(R[t', t, l - l']) (l' < l), + reg[l] on the diagonal
    b[(t,l), r] = sum_f sum_k conj(X_f[k, t]) w^{-kl} Y_f[k, r]
    c[r] = G^-1 b[:, r] (Cholesky),  H[k, r, t] = sum_l c[r, t, l] w^{kl}

Unknown (t, l) has index t L + l.  A pivot of the factorisation that is not finite or not above 64 2^-52 times its
original diagonal entry fails the estimate: status 1, taps and H NaN."""
import numpy as np

from oracle.esn_oracle import unit_qam

import remod_ref

EPS = 2.0 ** -52


def bits_to_indices(bits, m):
    """bits uint8 [B, N m, n_t] -> idx [B, N, n_t]"""
    B, nm, n_t = bits.shape
    b = bits.reshape(B, nm // m, m, n_t).astype(np.int64)
    return (b << np.arange(m)[None, None, :, None]).sum(axis=2)


def spectrum(y_cp, cp, p_i_frame):
    """y_cp complex [B, cp + N, n_r], p_i_frame [B] -> Y [B, N, n_r]"""
    n = y_cp.shape[1] - cp
    return np.fft.fft(y_cp[:, cp:], axis=1) / n / np.sqrt(p_i_frame)[:, None, None]


def design(X, L):
    """X complex [W, N, n_t] -> A [W N, n_t L], A[(f, k), (t, l)] = X_f[k, t] w^{kl}"""
    W, N, n_t = X.shape
    ph = np.exp(-2j * np.pi * np.outer(np.arange(N), np.arange(L)) / N)           # [N, L]
    return (X[:, :, :, None] * ph[None, :, None, :]).reshape(W * N, n_t * L)


def lag_sums(X, L):
    """X complex [W, N, n_t] -> R [n_t, n_t, L]"""
    W, N, n_t = X.shape
    ph = np.exp(-2j * np.pi * np.outer(np.arange(N), np.arange(L)) / N)
    return np.einsum("fkt,fku,kd->tud", X.conj(), X, ph)


def gram_from_lags(R, reg):
    """the block-Toeplitz G [n_t L, n_t L] of the n_t^2 L lag sums, reg [L] on the diagonal"""
    n_t, _, L = R.shape
    G = np.zeros((n_t, L, n_t, L), dtype=np.complex128)
    for l in range(L):
        for l2 in range(L):
            G[:, l, :, l2] = R[:, :, l2 - l] if l2 >= l else R[:, :, l - l2].conj().T
    G = G.reshape(n_t * L, n_t * L)
    return G + np.diag(np.tile(np.asarray(reg, dtype=np.float64), n_t))


def rhs(X, Y, L):
    """b [n_t L, n_r]"""
    W, N, n_t = X.shape
    return design(X, L).conj().T @ Y.reshape(W * N, -1)


def pivots_ok(G):
    """the factorisation's acceptance rule on a plain column Cholesky: every pivot finite and above 64 eps diag"""
    A = np.array(G, dtype=np.complex128)
    d0 = A.diagonal().real.copy()
    for j in range(A.shape[0]):
        d = A[j, j].real
        if not np.isfinite(d) or not d > 64 * EPS * d0[j]:
            return False
        col = A[j + 1:, j] / d
        A[j + 1:, j + 1:] -= np.outer(col, A[j + 1:, j].conj())
    return True


def solve_estimate(X, Y, L, reg):
    """X [W, N, n_t], Y [W, N, n_r], reg [L] -> dict(taps [n_r, n_t, L], H [N, n_r, n_t], status, G, cond)"""
    W, N, n_t = X.shape
    n_r = Y.shape[2]
    G = gram_from_lags(lag_sums(X, L), reg)
    b = rhs(X, Y, L)
    out = dict(G=G, b=b, status=0)
    if not (np.isfinite(G).all() and np.isfinite(b).all() and pivots_ok(G)):
        out.update(status=1, cond=np.inf, taps=np.full((n_r, n_t, L), np.nan + 0j), H=np.full((N, n_r, n_t), np.nan + 0j))
        return out
    out["cond"] = float(np.linalg.cond(G))
    Lc = np.linalg.cholesky(G)
    c = np.linalg.solve(Lc.conj().T, np.linalg.solve(Lc, b))                      # [n_t L, n_r]
    taps = c.T.reshape(n_r, n_t, L)
    out["taps"] = taps
    out["H"] = np.transpose(np.fft.fft(taps, N, axis=2), (2, 0, 1))
    return out


def channel_track(y_cp, window, est_per_group, cp, n_t, L, m, p_i, reg, X_hat=None, bits=None):
    """y_cp complex [n_est W, cp + N, n_r], X_hat complex [n_est W, N, n_t] or bits uint8 [n_est W, N m, n_t], p_i [G],
    reg [G, L] -> dict(taps [n_est, n_r, n_t, L], H [n_est, N, n_r, n_t], status [n_est], cond [n_est])"""
    assert (X_hat is None) != (bits is None)
    idx = remod_ref.slice_indices(X_hat, m) if bits is None else bits_to_indices(bits, m)
    X = unit_qam(m)[idx]
    n_est = y_cp.shape[0] // window
    group = np.arange(n_est) // est_per_group
    Y = spectrum(y_cp, cp, np.asarray(p_i, dtype=np.float64)[np.repeat(group, window)])
    res = [solve_estimate(X[e * window:(e + 1) * window], Y[e * window:(e + 1) * window], L, np.asarray(reg)[group[e]])
           for e in range(n_est)]
    return {k: np.stack([np.asarray(r[k]) for r in res]) for k in ("taps", "H", "status", "cond")}


def map_reg(n_sub, cp, isi, no, p_i):
    """reg [isi] the harness passes: T No / (N Pi r_h[l]) with r_h of oracle.baselines.isi_magnitude"""
    t = cp / 9
    mag = np.exp(-np.arange(cp + 1) / max(t, 1e-12))
    r_h = (mag / mag.sum())[:isi]
    return (n_sub + cp) * no / (n_sub * p_i * r_h)
