"""NumPy restatement of the SINR-weighted soft outputs (esn_mmse_sinr, esn_qam_llr_weighted, esn_detect_llr): the
equaliser's bias and SINR per subcarrier and stream by np.linalg.inv, and the weighted max-log LLRs on the oracle's
qam_llrs_maxlog and sigma2_from_decisions.  float64 / complex128 throughout."""
import numpy as np

from oracle import ldpc_oracle as lo

T_MIN, T_MAX = 1e-12, 1.0 - 1e-12


def sinr_weights(H, p_i, no):
    """H [G, N, n_r, n_t], p_i [G] -> (w [G, N, n_t], mu [G, N, n_t], gamma_mean [G]): with lam = no / p_i[g],
    t = lam [(H_k^H H_k + lam I)^-1]_ii clamped to [1e-12, 1 - 1e-12], mu = 1 - t, gamma = (1 - t) / t and
    w = gamma over its mean over the block."""
    G, N, _, n_t = H.shape
    t = np.empty((G, N, n_t))
    for g in range(G):
        lam = no / p_i[g]
        for k in range(N):
            A = np.linalg.inv(H[g, k].conj().T @ H[g, k] + lam * np.eye(n_t))
            t[g, k] = lam * np.real(np.diag(A))
    t = np.clip(t, T_MIN, T_MAX)
    mu = 1.0 - t
    gamma = mu / t
    mean = gamma.reshape(G, -1).mean(axis=1)
    return gamma / mean[:, None, None], mu, mean


def llr_weighted(X, w, mu, m, frames_per_group):
    """X complex [B, N, n_t], w / mu [G, N, n_t] -> (llr [B, n_t, N m], sigma2 [B]): sigma2 of frame f on X as it is,
    llr[f, i, k m + b] = w[g, k, i] (d1 - d0)(X[f, k, i] / mu[g, k, i]) / sigma2[f], g = f // frames_per_group."""
    B, N, n_t = X.shape
    llr, s2 = np.empty((B, n_t, N * m)), np.empty(B)
    for f in range(B):
        g = f // frames_per_group
        s2[f] = lo.sigma2_from_decisions(X[f].reshape(-1), m)
        for i in range(n_t):
            llr[f, i] = (w[g, :, i, None] * lo.qam_llrs_maxlog(X[f, :, i] / mu[g, :, i], m, s2[f])).reshape(-1)
    return llr, s2
