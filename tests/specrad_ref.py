"""NumPy restatement of the spectral radius by repeated squaring (include/esn_hip.h, esn_spectral_radius_batch):
a helper of the reservoir tests, not a test.  |.| is the Frobenius norm.

    f_0 = |W|, A_0 = W / f_0, l_0 = ln f_0
    k = 1..K:  B = A_{k-1} A_{k-1};  f_k = |B|;  l_k = 2 l_{k-1} + ln f_k;  A_k = B / f_k
    radius = exp((l_{K-1} + ln f_K) / 2^(K-1))
"""
import numpy as np


def specrad(W, n_squarings=24):
    """(radius, status): status 1 and radius 0.0 when some f_k is zero or not finite."""
    a = np.array(W, dtype=np.float64)
    with np.errstate(all="ignore"):
        f = np.linalg.norm(a)
        if not (f > 0.0 and np.isfinite(f)):
            return 0.0, 1
        a = a / f
        l_prev = np.log(f)                      # l_0
        for k in range(1, n_squarings + 1):
            b = a @ a
            f = np.linalg.norm(b)
            if not (f > 0.0 and np.isfinite(f)):
                return 0.0, 1
            if k == n_squarings:
                r = float(np.exp((l_prev + np.log(f)) / 2.0 ** (n_squarings - 1)))
                return (r, 0) if (r > 0.0 and np.isfinite(r)) else (0.0, 1)
            l_prev = 2.0 * l_prev + np.log(f)   # l_k
            a = b / f
    raise ValueError("n_squarings must be at least 1")


def reference_matrix(n, sparsity, seed):
    """The reference's unscaled W (pyESN.py:96-100): rand - 0.5, zeroed where a second rand < sparsity."""
    rs = np.random.RandomState(seed)
    w = rs.rand(n, n) - 0.5
    w[rs.rand(n, n) < sparsity] = 0
    return w


SIZES = (5, 16, 33, 100, 130, 300)
SPARSITIES = (0.0, 0.1, 0.9)
N_SEEDS = 5


def has_cycle(w):
    """Whether the graph of w's non-zero pattern has a cycle.  Without one w is nilpotent: its spectral radius is 0,
    there is nothing to scale (the reference itself would divide by zero), and the restatement must flag it."""
    p = (np.asarray(w) != 0).astype(np.float64)
    for _ in range(int(np.ceil(np.log2(max(2, p.shape[0])))) + 1):      # walks of length >= n exist iff a cycle does
        p = np.minimum(p @ p, 1.0)
    return bool(p.any())


def cases():
    """(n, sparsity, seed) of the shared matrix set: every size x sparsity x 5 seeds, and one n = 512.  The seeds of a
    (size, sparsity) count up from a fixed base; a draw without a cycle (two of the 5 x 5 matrices at sparsity 0.9) has
    no radius to compare and gives way to the next seed, so every case listed here is checked, none skipped."""
    out = []
    for n in SIZES:
        for si, sp in enumerate(SPARSITIES):
            seed, kept = 1000 * n + 10 * si, 0
            while kept < N_SEEDS:
                if has_cycle(reference_matrix(n, sp, seed)):
                    out.append((n, sp, seed))
                    kept += 1
                seed += 1
    out.append((512, 0.1, 512001))
    return out
