"""Access to the driver-loop fixtures (tests/golden/loop_*.npz) -- TEST INFRASTRUCTURE ONLY.

The fixtures hold what the reference's own driver loops computed (tests/golden/make_golden.py,
case_driver_loop): per coherence block the pilot, the channel and its estimates, per recorded data
frame the bits, the frames, every detector's X_hat and the running error counters, and the state
of the global NumPy stream wherever the driver is about to draw from it.  Nothing here computes an
expected value; this file only unpacks, and replays plain NumPy draws from a recorded state.
Besides arrays, integers and stream states the fixtures hold a few strings the generator wrote itself
(`layout`, `overrides`, `counter_names`, `xhat_names`)."""
from __future__ import annotations

import numpy as np

from .ofdm_frames import LinkConfig

# running error counter of each recorded X_hat, by the fixtures' own names
COUNTER_OF = {
    "v2": {"X_hat_ESN": "Err_uncoded_ESN", "X_hat_MMSE": "Err_uncoded_MMSE"},
    "nbf": {"X_hat_ESN_m": "TotalErr_ESN_matched", "X_hat_ESN_f": "TotalErr_ESN_trainFixed",
            "X_hat_PerfZF": "TotalErr_PerfectZF", "X_hat_LS_ZF": "TotalErr_LS_ZF", "X_hat_MMSE": "TotalErr_MMSE"},
    "siso": {"X_hat_ESN": "TotalErr_ESN", "X_hat_MMSE": "TotalErr_MMSE", "X_hat_ZF": "TotalErr_ZF",
             "X_hat_LS": "TotalErr_LS"},
}
BIT_COUNTERS = ("TotalBits", "TotalBits_uncoded_ESN", "TotalBits_uncoded_MMSE")
TRAIN_EBNO_FIXED_DB = 12.0          # the block-fading driver's second ESN is scaled for this point
# Bound on X_hat_ESN (of max) for a readout solved by QR / Cholesky instead of the reference's pinv: ten times the
# larger of cond(E) * 2**-52 and the deviation of a float64 NumPy QR solve, no tighter than 1e-10.  The CPU test
# recomputes cond(E) of every fixture block and asserts that the floor of 1e-10 is what decides.
ESN_BOUND = 1e-10


def rng_state(fx, key):
    """The tuple np.random.set_state takes, from the three arrays stored under `key`."""
    pos = fx[key + "_pos"]
    return ("MT19937", fx[key + "_keys"], int(pos[0]), int(pos[1]), float(fx[key + "_gauss"]))


def same_state(a, b):
    return a[2] == b[2] and a[3] == b[3] and np.array_equal(a[1], b[1]) and (a[3] == 0 or a[4] == b[4])


def bits(fx, key):
    shape = tuple(int(v) for v in fx[key + "_shape"])
    return np.unpackbits(fx[key])[:int(np.prod(shape))].reshape(shape)


def link_config(fx):
    """LinkConfig of the driver that wrote the fixture (the SISO driver has no CP and one tap)."""
    def p(name, default):
        return int(fx["param_" + name]) if "param_" + name in fx.files else default
    isi = p("IsiDuration", p("CP", 0) + 1)
    return LinkConfig(n_t=p("N_t", 1), n_r=p("N_r", 1), n_sub=p("N", 128), m=p("m", 4), isi=isi)


def blocks(fx):
    """[(point, block, kk of the pilot, Eb/No dB)]"""
    return [(int(j), int(b), int(kk), float(fx["ebno_db"][j])) for j, b, kk in fx["blocks"]]


def frames_of(fx, point, block):
    return [int(kk) for j, kk, b in fx["frames"] if (j, b) == (point, block)]


def counters(fx, key):
    return dict(zip([str(n) for n in fx["counter_names"]], [int(v) for v in fx[key]]))


def code_generator(fx):
    """The test-made sparse systematic G the coded drivers were given (seed and shape are stored)."""
    n, k = (int(v) for v in fx["g_shape"])
    rs = np.random.RandomState(int(fx["g_seed"]))
    return np.vstack([np.eye(k, dtype=np.int64), (rs.rand(n - k, k) < 0.02).astype(np.int64)])


def decision_margin(x, const):
    """Smallest distance of a real / imaginary part of x from a decision boundary of the grid.  Second copy of
    make_golden.py's function of the same name, on the ORACLE's constellation: the CPU test cross-checks the
    margins the generator stored (the generator itself does not depend on the oracle)."""
    lv = np.unique(np.round(const.real, 12))
    b = (lv[1:] + lv[:-1]) / 2
    x = np.asarray(x).ravel()
    return float(np.abs(np.r_[x.real, x.imag][:, None] - b[None, :]).min())
