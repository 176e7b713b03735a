"""NumPy restatement of esn_gen_taps_doppler (include/esn_hip.h) in closed form: no recurrence, every phasor is
np.exp(1j * pi * (2 fd_tsym s cos(pi a) + phi)) at the symbol asked for.  The angles (a, phi) are supplied; the paths,
powers and delays are those of esn_gen_taps kinds 0 (TDL-B, oracle/ofdm_frames.py's tables) and 1 (exponential PDP)."""
import numpy as np
from scipy.special import j0

from oracle.ofdm_frames import TDLB_NORM_DELAYS, TDLB_POW_DB

M = 16                      # ESN_DOPPLER_SINUSOIDS
# statistics of 16 384 links of the exponential PDP at fd_tsym = 0.01, symbols {0, 10, 20, 38, 60, 76}: the worst
# deviations of the restatement over RandomState seeds 0 .. 7 are 0.017 (autocorrelation) and 0.022 (power): the bounds
# leave a factor 2.3
ACF_TOL, POW_TOL = 0.05, 0.05


def pdp(kind, isi, fs=2 * 1.024e6, ds_ns=300.0):
    """(P [n_paths] path powers, place [n_paths, isi]: the share of every path on every tap)."""
    if kind == 0:
        p = 10.0 ** (TDLB_POW_DB / 10.0)
        p = p / p.sum()
        d = TDLB_NORM_DELAYS * ds_ns * 1e-9 * fs
        place = np.zeros((len(p), isi))
        for q in range(len(p)):
            i0 = int(np.floor(d[q]))
            frac = d[q] - i0
            if 0 <= i0 < isi:
                place[q, i0] += 1.0 - frac
            if 0 <= i0 + 1 < isi:
                place[q, i0 + 1] += frac
        return p, place
    if kind == 1:
        p = np.exp(-np.arange(isi) / max((isi - 1) / 9, 1e-12))
        return p / p.sum(), np.eye(isi)
    raise ValueError("kind must be 0 or 1")


def n_paths(kind, isi):
    return 23 if kind == 0 else isi


def draw_angles(rs, n_links, kind, isi):
    """(a, phi) uniform on [0, 2) half-turns: [n_links, n_paths, M, 2]."""
    return rs.uniform(0.0, 2.0, size=(n_links, n_paths(kind, isi), M, 2))


def path_gains(angles, power, fd_tsym, symbols):
    """g [n_links, n_sym, n_paths] = sqrt(P_p / M) sum_m exp(j pi (2 fd_tsym s cos(pi a) + phi))."""
    a, phi = angles[..., 0], angles[..., 1]
    s = np.asarray(symbols, dtype=np.float64)[None, :, None, None]
    z = np.exp(1j * np.pi * (2.0 * fd_tsym * s * np.cos(np.pi * a)[:, None] + phi[:, None]))
    return np.sqrt(power / M)[None, None, :] * z.sum(axis=-1)


def taps(kind, angles, isi, fd_tsym, symbols, fs=2 * 1.024e6, ds_ns=300.0):
    """taps [n_links, n_sym, isi] at the given symbol indices; kind 0 is scaled by the unit-energy factor of s = 0."""
    power, place = pdp(kind, isi, fs, ds_ns)
    h = path_gains(angles, power, fd_tsym, symbols) @ place
    if kind == 0:
        h0 = path_gains(angles, power, fd_tsym, [0]) @ place
        h = h / np.sqrt(np.sum(np.abs(h0) ** 2, axis=-1, keepdims=True))
    return h


def autocorrelation(h, h0):
    """Per tap: mean over links of h(s) conj(h(0)) over the mean power at s = 0 -> complex [n_sym, isi]."""
    return np.mean(h * np.conj(h0), axis=0) / np.mean(np.abs(h0) ** 2, axis=0)


def check_statistics(h, isi, fd_tsym, symbols):
    """h [n_links, len(symbols), isi] of kind 1 with symbols[0] == 0: the normalised autocorrelation of every tap within
    ACF_TOL of J0(2 pi fd_tsym s), the tap powers within POW_TOL (relative) of the exponential PDP at every symbol."""
    assert symbols[0] == 0
    acf = autocorrelation(h, h[:, :1])
    want = j0(2 * np.pi * fd_tsym * np.asarray(symbols, dtype=np.float64))
    dev = np.abs(acf - want[:, None]).max()
    pdev = np.abs(np.mean(np.abs(h) ** 2, axis=0) / pdp(1, isi)[0][None, :] - 1).max()
    print(f"autocorrelation: worst |R - J0| = {dev:.4f}; power: worst relative deviation = {pdev:.4f}")
    assert dev <= ACF_TOL, dev
    assert pdev <= POW_TOL, pdev
