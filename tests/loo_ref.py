"""Leave-one-out scores of a ridge fit in NumPy float64 (a helper of the test_loo_* / test_gpu_ridge_loo files, not a
test).  E [n, c] are the fit rows, Ds [n, n_out] the scaled teacher, lam >= 0 absolute.

closed_form: the two expressions of DESIGN 3.3c -- the wide one through K = E E^T + lam I, the tall one through
G = E^T E + lam I -- each by a Cholesky factorisation.  brute_force: delete row i, refit by an SVD ridge, take the
residual of row i.  They share no algebra beyond the definition of the ridge fit."""
import numpy as np


def ridge_svd(E, Ds, lam):
    """[n_out, cols]: V diag(s / (s^2 + lam)) U^T Ds, with NumPy's matrix_rank cut on round-off singular values."""
    U, s, Vt = np.linalg.svd(E, full_matrices=False)
    live = s > np.finfo(np.float64).eps * max(E.shape) * s[0]
    f = np.where(live, s / np.where(live, s * s + lam, 1.0), 0.0)
    return ((Vt.T * f) @ (U.T @ Ds)).T


def loo_wide(E, Ds, lam):
    """loo[i, o] = A[i, o] / (K^-1)[i, i],  K = E E^T + lam I,  A = K^-1 Ds."""
    n = E.shape[0]
    L = np.linalg.cholesky(E @ E.T + lam * np.eye(n))
    X = np.linalg.solve(L, np.eye(n))                   # L^-1
    A = X.T @ (X @ Ds)
    return A / np.sum(X * X, axis=0)[:, None]


def loo_tall(E, Ds, lam):
    """loo[i, o] = R[i, o] / (1 - h_i),  G = E^T E + lam I,  R = Ds - E G^-1 E^T Ds,  h_i = e_i^T G^-1 e_i."""
    c = E.shape[1]
    L = np.linalg.cholesky(E.T @ E + lam * np.eye(c))
    Y = np.linalg.solve(L, E.T)                         # L^-1 E^T, [c, n]
    W = np.linalg.solve(L.T, Y @ Ds)
    return (Ds - E @ W) / (1.0 - np.sum(Y * Y, axis=0))[:, None]


def loo_residuals(E, Ds, lam, form=None):
    if form is None:
        form = "wide" if E.shape[0] <= E.shape[1] else "tall"
    return loo_wide(E, Ds, lam) if form == "wide" else loo_tall(E, Ds, lam)


def closed_form(E, Ds, lam, form=None):
    """score = sum_i sum_o loo[i, o]^2; form None takes the wide expression for n <= c, as the kernel does."""
    r = loo_residuals(E, Ds, lam, form)
    return float(np.sum(r * r))


def brute_force(E, Ds, lam):
    """The definition: for each row i, the ridge fit on the other n - 1 rows (SVD), its squared residual on row i."""
    n = E.shape[0]
    total = 0.0
    for i in range(n):
        keep = np.arange(n) != i
        W = ridge_svd(E[keep], Ds[keep], lam)
        r = Ds[i] - W @ E[i]
        total += float(r @ r)
    return total


def scores(E, Ds, lams, form=None):
    """[L] closed-form scores; +inf for a negative or non-finite candidate."""
    out = np.full(len(lams), np.inf)
    for l, lam in enumerate(lams):
        if np.isfinite(lam) and lam >= 0:
            out[l] = closed_form(E, Ds, float(lam), form)
    return out


def choose(E, Ds, lams, form=None):
    """(index of the lowest candidate with the smallest finite score, or -1; the scores)."""
    s = scores(E, Ds, lams, form)
    if not np.any(np.isfinite(s)):
        return -1, s
    return int(np.argmin(np.where(np.isfinite(s), s, np.inf))), s


GRID_MULT = (1e-6, 1e-4, 1e-2, 1e-1, 1.0, 10.0, 100.0)      # candidates of the GPU tests, x the mean Gram diagonal


def _draw(rs, T, cols, n_out):
    E = rs.randn(T, cols) * 10.0 ** rs.uniform(-2.5, 0.0, size=cols)       # uneven column scales ...
    E[:, :3] *= 1e-3                                                        # ... and three columns x 1e-3
    clean = E @ rs.randn(cols, n_out)
    D = clean + 0.3 * np.std(clean) * rs.randn(T, n_out)                    # a linear map of E plus 30 % noise
    return E, D, rs.rand(n_out) + 0.5


def margin(s):
    """(second best - best) / best of the finite scores."""
    f = np.sort(s[np.isfinite(s)])
    return float((f[1] - f[0]) / f[0])


def make_case(rows, cols, n_out, n_groups, seed, transient=0, min_margin=None, f32=False):
    """Inputs in the manner of test_gpu_ridge.py: random E with uneven column scales and three columns x 1e-3, the
    teacher a random linear map of E plus 30 % noise, a per-output teacher scale.  Returns E [G, T, cols],
    D [G, T, n_out], t_scale [G, n_out] with T = rows + transient.

    min_margin: a group is redrawn (next seed) until the reference scores over GRID_MULT x its mean Gram diagonal
    have a winner that far ahead of the runner-up -- a choice test needs inputs on which the choice is a fact of the
    data and not of the last bits; the draw looks at the reference alone.  f32: the margin is taken on E rounded to
    float32, which is what the kernel is then given."""
    Es, Ds, ts = [], [], []
    for g in range(n_groups):
        for attempt in range(64):
            rs = np.random.RandomState((seed + 104729 * g + 7919 * attempt) % (2 ** 31))
            E, D, t = _draw(rs, rows + transient, cols, n_out)
            if min_margin is None:
                break
            Ef = E.astype(np.float32).astype(np.float64)[transient:] if f32 else E[transient:]
            lams = gram_mean_diag(Ef) * np.array(GRID_MULT)
            if margin(scores(Ef, D[transient:] * t, lams)) >= min_margin:
                break
        else:
            raise RuntimeError("no draw with a clear winner")
        Es.append(E), Ds.append(D), ts.append(t)
    return np.stack(Es), np.stack(Ds), np.stack(ts)


def gram_mean_diag(E):
    """Mean diagonal of the Gram matrix the kernel factorises for fit rows E [n, c] (E E^T for n <= c, else E^T E)."""
    n, c = E.shape
    return float(np.sum(E * E) / min(n, c))
