"""NumPy restatement of the windowed FNN (include/esn_hip.h: esn_fnn_train / esn_fnn_predict).

train        one group's Adam training in any NumPy float type, with the trained rows in ascending or reversed order
             (the same sums, taken in another order): the parameters, the loss before each step and the smallest
             |pre-activation| met -- a ReLU on its kink would make the result depend on rounding.
predict      the ELM's prediction with max(., 0) for tanh and W_out = [W2 | b2]; fp16_operands=True rounds W1, the scaled
             inputs, the hidden rows, W2 and b2 through np.float16 (what the ESN_F16 kernel feeds its matrix
             instructions) and keeps every sum and the bias add in float64."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elm_ref  # noqa: E402


def trained_rows(U, D, window, transient, in_scale=None, in_shift=None, t_scale=None, t_shift=None):
    """X [|R|, K] and Ds [|R|, n_out] of one group: rows max(transient, window - 1) .. T - 1."""
    D = np.asarray(D, dtype=np.float64)
    T = D.shape[0]
    us = elm_ref.scaled_inputs(U, T, in_scale, in_shift)
    r0 = max(int(transient), window - 1)
    X = elm_ref.windows(us, window)[r0 - (window - 1):]
    Ds = D
    if t_scale is not None:
        Ds = Ds * t_scale
    if t_shift is not None:
        Ds = Ds + t_shift
    return X, Ds[r0:]


def train_rows(X, Ds, init, epochs=50, lr=0.01, betas=(0.9, 0.999), eps=1e-8, dtype=np.float64, reverse=False):
    """Adam on already-windowed rows.  Returns dict(W1, b1, W2, b2, loss [epochs], min_pre)."""
    X, Ds = np.asarray(X, dtype=dtype), np.asarray(Ds, dtype=dtype)
    if reverse:
        X, Ds = X[::-1].copy(), Ds[::-1].copy()
    prm = [np.array(t, dtype=dtype) for t in init]                      # W1, b1, W2, b2
    m = [np.zeros_like(t) for t in prm]
    v = [np.zeros_like(t) for t in prm]
    one, two = dtype(1), dtype(2)
    beta1, beta2, lr, eps = dtype(betas[0]), dtype(betas[1]), dtype(lr), dtype(eps)
    n = dtype(Ds.shape[0] * Ds.shape[1])
    loss, min_pre = [], np.inf
    for e in range(1, epochs + 1):
        W1, b1, W2, b2 = prm
        pre = X @ W1.T + b1
        min_pre = min(min_pre, float(np.abs(pre).min()))
        h = np.maximum(pre, dtype(0))
        diff = h @ W2.T + b2 - Ds
        loss.append((diff * diff).sum() / n)
        dy = two * diff / n
        dh = (dy @ W2) * (pre > 0)
        grads = [dh.T @ X, dh.sum(axis=0), dy.T @ h, dy.sum(axis=0)]
        step = lr / (one - beta1 ** e)
        rs2 = np.sqrt(one - beta2 ** e)
        for i, q in enumerate(grads):
            m[i] = beta1 * m[i] + (one - beta1) * q
            v[i] = beta2 * v[i] + (one - beta2) * (q * q)
            prm[i] = prm[i] - step * (m[i] / (np.sqrt(v[i]) / rs2 + eps))
    return dict(W1=prm[0], b1=prm[1], W2=prm[2], b2=prm[3], loss=np.array(loss), min_pre=min_pre)


def train(U, D, init, window, transient, in_scale=None, in_shift=None, t_scale=None, t_shift=None, **kw):
    """esn_fnn_train for one group: U [T_in, n_in], D [T, n_out], init = (W1, b1, W2, b2) of that group."""
    X, Ds = trained_rows(U, D, window, transient, in_scale, in_shift, t_scale, t_shift)
    return train_rows(X, Ds, init, **kw)


def train_groups(U, D, init, window, transient, group_offset=0, in_scale=None, in_shift=None, t_scale=None,
                 t_shift=None, groups=None, **kw):
    """U [G, T_in, n_in], D [G, T, n_out], init four arrays [n_isets, ...]: the stacked results of `groups` (all)."""
    n_isets = len(init[0])
    out = []
    for g in (range(len(U)) if groups is None else groups):
        s = (group_offset + g) % n_isets
        out.append(train(U[g], D[g], [t[s] for t in init], window, transient,
                         None if in_scale is None else in_scale[g], None if in_shift is None else in_shift[g],
                         None if t_scale is None else t_scale[g], None if t_shift is None else t_shift[g], **kw))
    res = {k: np.stack([o[k] for o in out]) for k in ("W1", "b1", "W2", "b2", "loss")}
    res["min_pre"] = min(o["min_pre"] for o in out)
    return res


def predict(U, frames_per_group, T, transient, W1, b1, W2, b2, window, in_scale=None, in_shift=None, t_scale=None,
            t_shift=None, fp16_operands=False):
    """esn_fnn_predict: U [B, T_in, n_in], parameters [G, ...] -> Y [B, T - transient, n_out]."""
    h16 = elm_ref._h
    out = []
    for f in range(len(U)):
        g = f // frames_per_group
        us = h16(elm_ref.scaled_inputs(U[f], T, None if in_scale is None else in_scale[g],
                                       None if in_shift is None else in_shift[g]), fp16_operands)
        W1g, W2g, b2g = (h16(np.asarray(t[g], dtype=np.float64), fp16_operands) for t in (W1, W2, b2))
        hid = h16(np.maximum(elm_ref.windows(us, window) @ W1g.T + b1[g], 0.0), fp16_operands)
        ys = np.zeros((T, W2g.shape[0]))
        ys[window - 1:] = hid @ W2g.T + b2g
        if t_shift is not None:
            ys = ys - t_shift[g]
        if t_scale is not None:
            ys = ys / t_scale[g]
        ys[:window - 1] = 0.0
        out.append(ys[transient:])
    return np.stack(out)
