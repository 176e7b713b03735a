"""NumPy restatement of the windowed CNN (include/esn_hip.h: esn_cnn_train / esn_cnn_predict).

A Conv1d layer with zero padding p = (k - 1) / 2 is a matrix product: rows(x, k) [T, k c_in] holds, in row t, the input
rows t - p .. t + p (zeros outside [0, T)), column j c_in + i; wmat(W) [c_out, k c_in] the weights in that order.

train        one group's Adam training in any NumPy float type, with every sum's terms in ascending or reversed order
             (the same sums, taken in another order): the six parameters in torch's Conv1d layout, the loss before each
             step and the smallest |pre-activation| met -- a ReLU on its kink would make the result depend on rounding.
predict      the forward pass of frames grouped like esn_cnn_predict's."""
import numpy as np

NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")


def scaled_inputs(U, T, in_scale=None, in_shift=None, dtype=np.float64):
    """x_0 [T, n_in]: zero rows appended to U [T_in, n_in] BEFORE scaling."""
    U = np.asarray(U, dtype=dtype)
    x = np.zeros((T, U.shape[1]), dtype=dtype)
    x[:U.shape[0]] = U
    if in_scale is not None:
        x = x * np.asarray(in_scale, dtype=dtype)
    if in_shift is not None:
        x = x + np.asarray(in_shift, dtype=dtype)
    return x


def rows(x, k):
    """[T, k c]: row t is x[t - p .. t + p] flattened, zeros outside [0, T)."""
    T, c = x.shape
    p = (k - 1) // 2
    xp = np.zeros((T + 2 * p, c), dtype=x.dtype)
    xp[p:p + T] = x
    return np.concatenate([xp[j:j + T] for j in range(k)], axis=1)


def fold(dX, k):
    """The transpose of rows: dX [T, k c] -> dx [T, c], dx[t + j - p] += dX[t, j c .. (j + 1) c)."""
    T, c = dX.shape[0], dX.shape[1] // k
    p = (k - 1) // 2
    dxp = np.zeros((T + 2 * p, c), dtype=dX.dtype)
    for j in range(k):
        dxp[j:j + T] += dX[:, j * c:(j + 1) * c]
    return dxp[p:p + T]


def wmat(W):
    """W [c_out, c_in, k] -> [c_out, k c_in], column j c_in + i."""
    return np.ascontiguousarray(W.transpose(0, 2, 1).reshape(W.shape[0], -1))


def unwmat(Wm, c_in, k):
    return np.ascontiguousarray(Wm.reshape(Wm.shape[0], k, c_in).transpose(0, 2, 1))


def _mm(a, b, reverse):
    """a [m, n] @ b [n, q], the inner index ascending or reversed."""
    return (a[:, ::-1].copy() @ b[::-1].copy()) if reverse else a @ b


def forward(x0, prm, k, reverse=False):
    """(pre1, pre2, ys, X0, X1, X2) of one sequence x0 [T, n_in] under prm = (W1, b1, W2, b2, W3, b3)."""
    W1, b1, W2, b2, W3, b3 = prm
    zero = x0.dtype.type(0)
    X0 = rows(x0, k)
    pre1 = _mm(X0, wmat(W1).T, reverse) + b1
    X1 = rows(np.maximum(pre1, zero), k)
    pre2 = _mm(X1, wmat(W2).T, reverse) + b2
    X2 = rows(np.maximum(pre2, zero), k)
    ys = _mm(X2, wmat(W3).T, reverse) + b3
    return pre1, pre2, ys, X0, X1, X2


def train(U, D, init, kernel, transient=0, in_scale=None, in_shift=None, t_scale=None, t_shift=None, epochs=50,
          lr=0.01, betas=(0.9, 0.999), eps=1e-8, dtype=np.float64, reverse=False):
    """esn_cnn_train for one group: U [T_in, n_in], D [T, n_out], init = the six arrays of that group.  Returns
    dict(W1 .. b3, loss [epochs], min_pre)."""
    k = int(kernel)
    D = np.asarray(D, dtype=dtype)
    T, n_out = D.shape
    x0 = scaled_inputs(U, T, in_scale, in_shift, dtype)
    Ds = D
    if t_scale is not None:
        Ds = Ds * np.asarray(t_scale, dtype=dtype)
    if t_shift is not None:
        Ds = Ds + np.asarray(t_shift, dtype=dtype)
    prm = [np.array(t, dtype=dtype) for t in init]
    m = [np.zeros_like(t) for t in prm]
    v = [np.zeros_like(t) for t in prm]
    one, two = dtype(1), dtype(2)
    beta1, beta2, lr, eps = dtype(betas[0]), dtype(betas[1]), dtype(lr), dtype(eps)
    n = dtype((T - transient) * n_out)
    on = (np.arange(T) >= transient)[:, None]
    loss, min_pre = [], np.inf
    c = [prm[0].shape[1], prm[0].shape[0], prm[2].shape[0]]
    for e in range(1, epochs + 1):
        W1, b1, W2, b2, W3, b3 = prm
        pre1, pre2, ys, X0, X1, X2 = forward(x0, prm, k, reverse)
        min_pre = min(min_pre, float(np.abs(pre1).min()), float(np.abs(pre2).min()))
        diff = np.where(on, ys - Ds, dtype(0))
        loss.append((diff * diff).sum() / n)
        dz3 = two * diff / n
        dz2 = fold(_mm(dz3, wmat(W3), reverse), k) * (pre2 > 0)
        dz1 = fold(_mm(dz2, wmat(W2), reverse), k) * (pre1 > 0)
        grads = []
        for dz, X, cin in ((dz1, X0, c[0]), (dz2, X1, c[1]), (dz3, X2, c[2])):
            grads += [unwmat(_mm(np.ascontiguousarray(dz.T), X, reverse), cin, k),
                      (dz[::-1] if reverse else dz).sum(axis=0)]
        step = lr / (one - beta1 ** e)
        rs2 = np.sqrt(one - beta2 ** e)
        for i, q in enumerate(grads):
            m[i] = beta1 * m[i] + (one - beta1) * q
            v[i] = beta2 * v[i] + (one - beta2) * (q * q)
            prm[i] = prm[i] - step * (m[i] / (np.sqrt(v[i]) / rs2 + eps))
    out = dict(zip(NAMES, prm))
    out.update(loss=np.array(loss), min_pre=min_pre)
    return out


def train_groups(U, D, init, kernel, transient=0, group_offset=0, in_scale=None, in_shift=None, t_scale=None,
                 t_shift=None, groups=None, **kw):
    """U [G, T_in, n_in], D [G, T, n_out], init six arrays [n_isets, ...]: the stacked results of `groups` (all)."""
    n_isets = len(init[0])
    out = []
    for g in (range(len(U)) if groups is None else groups):
        s = (group_offset + g) % n_isets
        out.append(train(U[g], D[g], [t[s] for t in init], kernel, transient,
                         None if in_scale is None else in_scale[g], None if in_shift is None else in_shift[g],
                         None if t_scale is None else t_scale[g], None if t_shift is None else t_shift[g], **kw))
    res = {n: np.stack([o[n] for o in out]) for n in NAMES + ("loss",)}
    res["min_pre"] = min(o["min_pre"] for o in out)
    return res


def predict(U, frames_per_group, T, transient, prm, kernel, in_scale=None, in_shift=None, t_scale=None, t_shift=None,
            dtype=np.float64):
    """esn_cnn_predict: U [B, T_in, n_in], prm six arrays [G, ...] -> Y [B, T - transient, n_out] in `dtype`."""
    out = []
    for f in range(len(U)):
        g = f // frames_per_group
        x0 = scaled_inputs(U[f], T, None if in_scale is None else in_scale[g], None if in_shift is None else in_shift[g],
                           dtype)
        ys = forward(x0, [np.asarray(t[g], dtype=dtype) for t in prm], int(kernel))[2]
        if t_shift is not None:
            ys = ys - np.asarray(t_shift[g], dtype=dtype)
        if t_scale is not None:
            ys = ys / np.asarray(t_scale[g], dtype=dtype)
        out.append(ys[transient:])
    return np.stack(out)
