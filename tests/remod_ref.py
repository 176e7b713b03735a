"""NumPy restatement of esn_detect_remod (include/esn_hip.h): np.fft, the slicer rule of
tests/test_gpu_detect_fixed.py::test_fixed_against_numpy and oracle.esn_oracle.unit_qam.

    X     = FFT_N(y) / (N sqrt(Pi[group]))
    idx   = i side + j,  i, j = clip(rint(((Re, Im) X norm + side - 1) / 2), 0, side - 1)
    x_t   = N IFFT_N(unit_qam[idx]) sqrt(Pi[group])
    D_hat = [delay zero rows | last cp samples of x_t | x_t], Re/Im interleaved per antenna
            (oracle.esn_oracle.pack_delay_io's teacher)"""
import numpy as np

from oracle.esn_oracle import unit_qam


def slicer_constants(m):
    side = 1 << (m // 2)
    return side, np.sqrt(2.0 * (side * side - 1) / 3.0)


def slice_indices(X, m):
    """constellation index of every element of complex X"""
    side, norm = slicer_constants(m)
    lev = lambda v: np.clip(np.rint((v * norm + (side - 1)) * 0.5), 0, side - 1).astype(np.int64)
    return lev(X.real) * side + lev(X.imag)


def index_bits(idx, m):
    """idx [B, N, n_t] -> bits uint8 [B, N m, n_t], natural binary, LSB first (the layout of tx_bits)"""
    B, N, n_t = idx.shape
    bits = (idx[:, :, None, :] >> np.arange(m)[None, None, :, None]) & 1
    return bits.reshape(B, N * m, n_t).astype(np.uint8)


def remodulate(idx, m, p_i_frame, cp, delay):
    """idx [B, N, n_t], p_i_frame [B] -> D_hat float64 [B, delay + cp + N, 2 n_t]"""
    B, N, n_t = idx.shape
    x_t = N * np.fft.ifft(unit_qam(m)[idx], axis=1) * np.sqrt(p_i_frame)[:, None, None]
    x_cp = np.concatenate([x_t[:, N - cp:], x_t], axis=1) if cp else x_t
    D = np.zeros((B, delay + cp + N, 2 * n_t))
    D[:, delay:, 0::2] = x_cp.real
    D[:, delay:, 1::2] = x_cp.imag
    return D


def detect_remod(Y, frames_per_group, n_sub, cp, delay, n_t, m, p_i, tx_bits=None):
    """Y float64 [B, N, 2 n_t], p_i [G] -> dict(X_hat complex [B, N, n_t], idx, dec_bits, D_hat, and with tx_bits
    [B, N m, n_t]: err [G], bits [G])"""
    Y = np.asarray(Y, dtype=np.float64)
    B = Y.shape[0]
    group = np.arange(B) // frames_per_group
    p_f = np.asarray(p_i, dtype=np.float64)[group]
    y = Y.reshape(B, n_sub, n_t, 2)
    X = np.fft.fft(y[..., 0] + 1j * y[..., 1], axis=1) * (1.0 / (n_sub * np.sqrt(p_f)))[:, None, None]
    idx = slice_indices(X, m)
    out = dict(X_hat=X, idx=idx, dec_bits=index_bits(idx, m), D_hat=remodulate(idx, m, p_f, cp, delay))
    if tx_bits is not None:
        G = (B + frames_per_group - 1) // frames_per_group
        wrong = (out["dec_bits"] != np.asarray(tx_bits).reshape(B, n_sub * m, n_t)).reshape(B, -1).sum(axis=1)
        out["err"] = np.bincount(group, weights=wrong, minlength=G).astype(np.int64)
        out["bits"] = np.bincount(group, minlength=G).astype(np.int64) * (n_sub * m * n_t)
    return out
