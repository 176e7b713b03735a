"""NumPy restatement of the windowed ELM (include/esn_hip.h: esn_elm_features / esn_elm_predict), float64 throughout.

fp16_operands=True rounds W_in, the scaled inputs, the hidden rows and W_out through np.float16 (what the ESN_F16 kernel
feeds its matrix instructions) and keeps every sum, the bias add and tanh in float64: the kernel's result differs from
it by float32 accumulation and the device tanh only."""
import numpy as np


def _h(x, fp16):
    return x.astype(np.float16).astype(np.float64) if fp16 else x


def scaled_inputs(U, T, in_scale=None, in_shift=None):
    """U [T_in, n_in] -> us [T, n_in]: zero rows appended BEFORE scaling."""
    U = np.asarray(U, dtype=np.float64)
    us = np.zeros((T, U.shape[1]))
    us[:U.shape[0]] = U
    if in_scale is not None:
        us = us * in_scale
    if in_shift is not None:
        us = us + in_shift
    return us


def windows(us, window):
    """[T, n_in] -> [T - window + 1, window n_in]: row j is us[j:j + window].flatten(), oldest sample first."""
    T = us.shape[0]
    return np.stack([us[j:j + window].reshape(-1) for j in range(T - window + 1)])


def rows(U, T, W_in, b, window, bias_col=True, e_cols=None, in_scale=None, in_shift=None, fp16_operands=False):
    """The extended rows E [T, e_cols] of one sequence: zeros for t < window - 1, tanh | 1 | zero pad from there."""
    W_in, b = np.asarray(W_in, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n_hidden = W_in.shape[0]
    cols = n_hidden + int(bool(bias_col))
    e_cols = cols if e_cols is None else e_cols
    us = _h(scaled_inputs(U, T, in_scale, in_shift), fp16_operands)
    hidden = _h(np.tanh(windows(us, window) @ _h(W_in, fp16_operands).T + b), fp16_operands)
    E = np.zeros((T, e_cols))
    E[window - 1:, :n_hidden] = hidden
    if bias_col:
        E[window - 1:, n_hidden] = 1.0
    return E


def features(U, T, W_in, b, window, bias_col=True, e_cols=None, in_scale=None, in_shift=None, group_offset=0):
    """esn_elm_features: U [G, T_in, n_in], W_in [S, n_hidden, K], b [S, n_hidden], scalings [G, n_in] -> [G, T, e_cols]."""
    W_in, b = np.asarray(W_in), np.asarray(b)
    out = []
    for g in range(len(U)):
        s = (group_offset + g) % W_in.shape[0]
        out.append(rows(U[g], T, W_in[s], b[s], window, bias_col, e_cols,
                        None if in_scale is None else in_scale[g], None if in_shift is None else in_shift[g]))
    return np.stack(out)


def fit(E, D, transient, t_scale=None, t_shift=None, ridge=None):
    """W_out [n_out, cols] from rows transient.. of one group: pinv, or ridge (lambda absolute, Gram of E)."""
    Ds = np.asarray(D, dtype=np.float64)
    if t_scale is not None:
        Ds = Ds * t_scale
    if t_shift is not None:
        Ds = Ds + t_shift
    A, B = E[transient:], Ds[transient:]
    if ridge is None:
        return (np.linalg.pinv(A) @ B).T
    return np.linalg.solve(A.T @ A + ridge * np.eye(A.shape[1]), A.T @ B).T


def predict(U, frames_per_group, T, transient, W_in, b, W_out, window, bias_col=True, in_scale=None, in_shift=None,
            t_scale=None, t_shift=None, group_offset=0, fp16_operands=False):
    """esn_elm_predict: U [B, T_in, n_in], W_out [G, n_out, e_cols] -> Y [B, T - transient, n_out]."""
    W_in, b, W_out = np.asarray(W_in), np.asarray(b), np.asarray(W_out, dtype=np.float64)
    out = []
    for f in range(len(U)):
        g = f // frames_per_group
        s = (group_offset + g) % W_in.shape[0]
        E = rows(U[f], T, W_in[s], b[s], window, bias_col, W_out.shape[2],
                 None if in_scale is None else in_scale[g], None if in_shift is None else in_shift[g], fp16_operands)
        ys = E @ _h(W_out[g], fp16_operands).T
        if t_shift is not None:
            ys = ys - t_shift[g]
        if t_scale is not None:
            ys = ys / t_scale[g]
        ys[:window - 1] = 0.0
        out.append(ys[transient:])
    return np.stack(out)
