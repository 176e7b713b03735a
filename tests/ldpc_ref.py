"""NumPy helpers for the tests of the coded leg (esn_coded.hip, coded.py) and of its oracle (oracle/ldpc_oracle.py):

    bp_trace         the message passing of ldpc_oracle.decode_bp WITHOUT the early stop: the posteriors of every
                     iteration and how close any check product X came to +-1, i.e. the margins a comparison of hard
                     decisions between two implementations of tanh / log rests on
    graph_arrays     the four index arrays esn_ldpc_decode_count takes, for an arbitrary parity-check matrix
    exact_bit_llrs   bitwise MAP by enumeration of the code: what sum-product computes exactly on a cycle-free graph
    llr_longdouble   max-log LLRs by brute force over the whole 2-D constellation in np.longdouble, with the labels of
                     oracle.esn_oracle (unit_qam, bit_labels_lsb_first), i.e. the uncoded detector's own mapping
    tree_code        the cycle-free graph and the observations both tree tests use"""
import numpy as np

from oracle.esn_oracle import bit_labels_lsb_first, unit_qam


def graph_arrays(H):
    """H [m, n] -> chk_ptr [m + 1], edge_var [E], var_ptr [n + 1], var_edge [E] (int32): edges in check-major order,
    var_edge lists the edges of each variable (the construction of LdpcCode.__init__)."""
    H = np.asarray(H)
    m, n = H.shape
    ci, vi = np.nonzero(H)
    chk_ptr = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=m))]).astype(np.int32)
    var_edge = np.argsort(vi, kind="stable").astype(np.int32)
    var_ptr = np.concatenate([[0], np.cumsum(np.bincount(vi, minlength=n))]).astype(np.int32)
    return chk_ptr, vi.astype(np.int32), var_ptr, var_edge


def bp_trace(H, y, snr_db, maxiter):
    """Flooding log-domain sum-product as ldpc_oracle.decode_bp runs it, every word through all maxiter sweeps.
    Returns (L_post [maxiter, n_cw, n], margin [maxiter, n_cw]) with margin = min over the edges of 1 - |X|."""
    H = np.asarray(H)
    var = 10.0 ** (-snr_db / 10.0)
    Lc = 2.0 * np.asarray(y, dtype=np.float64) / var
    n_cw, n = Lc.shape
    ci, vi = np.nonzero(H)
    dc = np.bincount(ci, minlength=H.shape[0])
    starts = np.concatenate([[0], np.cumsum(dc)])[:-1]
    Lq = Lc[:, vi].copy()
    posts, margins = [], []
    for _ in range(maxiter):
        t = np.tanh(0.5 * Lq)
        Lr = np.empty_like(Lq)
        margin = np.full(n_cw, np.inf)
        for e in range(len(ci)):
            s, cnt = starts[ci[e]], dc[ci[e]]
            X = np.prod(t[:, [q for q in range(s, s + cnt) if q != e]], axis=1)
            margin = np.minimum(margin, 1.0 - np.abs(X))
            num, den = 1.0 + X, 1.0 - X
            with np.errstate(divide="ignore", invalid="ignore"):
                v = np.log(num / den)
            Lr[:, e] = np.where(num == 0, -1.0, np.where(den == 0, 1.0, v))
        tot = np.zeros((n_cw, n))
        np.add.at(tot, (slice(None), vi), Lr)
        L_post = Lc + tot
        Lq = L_post[:, vi] - Lr
        posts.append(L_post)
        margins.append(margin)
    return np.stack(posts), np.stack(margins)


def trace_decision(H, L_post):
    """What decode_bp returns, read off a trace: the hard decision of the first iteration with zero syndrome, else of
    the last.  Also returns that iteration's index per word."""
    H = np.asarray(H).astype(np.int64)
    x = (L_post <= 0).astype(np.uint8)                                  # [it, n_cw, n]
    ok = ~((x.astype(np.int64) @ H.T) % 2).any(axis=2)                  # [it, n_cw]
    stop = np.where(ok.any(axis=0), ok.argmax(axis=0), L_post.shape[0] - 1)
    return x[stop, np.arange(x.shape[1])], stop


def exact_bit_llrs(H, Lc):
    """L_v = logsumexp(ll | c_v = 0) - logsumexp(ll | c_v = 1) over all codewords c of H, ll(c) = sum_v Lc_v (1 - 2 c_v) / 2:
    the bitwise MAP log-ratio for channel LLRs Lc [n_cw, n].  A bit that is 0 (1) in every codeword gets +inf (-inf)."""
    H = np.asarray(H).astype(np.int64)
    n = H.shape[1]
    if n > 20:
        raise ValueError("enumeration is meant for n <= 20")
    words = (np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1
    words = words[~((words @ H.T) % 2).any(axis=1)]                     # [C, n]
    ll = 0.5 * np.asarray(Lc, dtype=np.float64) @ (1.0 - 2.0 * words).T  # [n_cw, C]

    def lse(a):
        if a.shape[1] == 0:
            return np.full(a.shape[0], -np.inf)
        top = a.max(axis=1)
        return top + np.log(np.exp(a - top[:, None]).sum(axis=1))

    out = np.empty((ll.shape[0], n))
    for v in range(n):
        out[:, v] = lse(ll[:, words[:, v] == 0]) - lse(ll[:, words[:, v] == 1])
    return out


def llr_longdouble(z, m, sigma2):
    """z complex [S] -> (llr [S, m], dsum [S, m]) in np.longdouble: llr = (d1 - d0) / max(sigma2, 1e-12) with d0 (d1) the
    squared distance to the nearest point of unit_qam(m) whose bit b is 0 (1); dsum = d0 + d1."""
    z = np.asarray(z).reshape(-1)
    const = unit_qam(m)
    labels = bit_labels_lsb_first(m)
    dre = z.real.astype(np.longdouble)[:, None] - const.real.astype(np.longdouble)[None, :]
    dim = z.imag.astype(np.longdouble)[:, None] - const.imag.astype(np.longdouble)[None, :]
    d = dre * dre + dim * dim                                            # [S, 2^m]
    s2 = np.longdouble(max(float(sigma2), 1e-12))
    llr = np.empty((z.size, m), dtype=np.longdouble)
    dsum = np.empty((z.size, m), dtype=np.longdouble)
    for b in range(m):
        d0 = d[:, labels[:, b] == 0].min(axis=1)
        d1 = d[:, labels[:, b] == 1].min(axis=1)
        llr[:, b] = (d1 - d0) / s2
        dsum[:, b] = d0 + d1
    return llr, dsum


TREE_ROWS = ((0, 1, 2), (2, 3, 4, 5), (5, 6), (4, 7, 8, 9), (10,))


def tree_code(seed=0, n_cw=256, gadget=True):
    """A cycle-free graph, 5 checks x 11 variables with check degrees 3, 4, 2, 4 (and 1), and observations for it.
    Variable 10 hangs on a check of its own and shares no edge with the tree: observed as -5 it reads 1, its check
    never holds, and no decoder stops early.  With gadget=False it is observed as +5 and decoders may stop.
    Returns (H uint8 [5, 11], y [n_cw, 11]) for snr = 1.0."""
    H = np.zeros((len(TREE_ROWS), 11), dtype=np.uint8)
    for r, cols in enumerate(TREE_ROWS):
        H[r, list(cols)] = 1
    rs = np.random.RandomState(seed)
    y = 0.9 * rs.randn(n_cw, 11) + np.where(rs.rand(n_cw, 11) > 0.5, 0.6, -0.6)
    y[:, 10] = -5.0 if gadget else 5.0
    return H, y
