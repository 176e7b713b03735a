"""NumPy restatement of the LSTM comparator (include/esn_hip.h: esn_lstm_train / esn_lstm_predict).

train        one group's Adam training (exact backpropagation through time) in any NumPy float type.  reverse=True takes
             every inner product and every sum over t with its terms in reversed order (the same sums, taken in another
             order); nudge=True moves every tanh and sigma result one ulp up -- the device's tanh and exp are not
             NumPy's, and this puts that difference into a sensitivity.  Returns the six parameters in torch's layout and
             the loss before each step.
train_groups the stacked results of several groups, with the rotation of initial sets.
predict      the forward pass of frames grouped like esn_lstm_predict's, every frame from h = c = 0."""
import numpy as np

NAMES = ("W_ih", "W_hh", "b_ih", "b_hh", "W_fc", "b_fc")


def scaled_inputs(U, T, in_scale=None, in_shift=None, dtype=np.float64):
    """x [..., T, n_in]: zero rows appended to U [..., T_in, n_in] BEFORE scaling."""
    U = np.asarray(U, dtype=dtype)
    x = np.zeros(U.shape[:-2] + (T, U.shape[-1]), dtype=dtype)
    x[..., :U.shape[-2], :] = U
    if in_scale is not None:
        x = x * np.asarray(in_scale, dtype=dtype)
    if in_shift is not None:
        x = x + np.asarray(in_shift, dtype=dtype)
    return x


def _mm(a, b, reverse=False):
    """a [m, n] @ b [n, q], the inner index ascending or reversed."""
    return (a[:, ::-1].copy() @ b[::-1].copy()) if reverse else a @ b


def _up(y, nudge):
    return np.nextafter(y, y.dtype.type(np.inf)) if nudge else y


def sigma(a, nudge=False):
    one = a.dtype.type(1)
    return _up(one / (one + np.exp(-a)), nudge)


def tanh(a, nudge=False):
    return _up(np.tanh(a), nudge)


def forward(x, prm, reverse=False, nudge=False):
    """x [B, T, n_in] (B sequences under one parameter set) -> dict of i, f, g, o, c, tc = tanh(c), h [B, T, H] and
    ys [B, T, n_out]."""
    W_ih, W_hh, b_ih, b_hh, W_fc, b_fc = prm
    B, T, _ = x.shape
    H = W_hh.shape[1]
    out = {k: np.zeros((B, T, H), dtype=x.dtype) for k in "ifgoch"}
    out["tc"] = np.zeros((B, T, H), dtype=x.dtype)
    h = np.zeros((B, H), dtype=x.dtype)
    c = np.zeros((B, H), dtype=x.dtype)
    for t in range(T):
        z = (_mm(x[:, t], W_ih.T, reverse) + b_ih) + (_mm(h, W_hh.T, reverse) + b_hh)
        i, f = sigma(z[:, :H], nudge), sigma(z[:, H:2 * H], nudge)
        g, o = tanh(z[:, 2 * H:3 * H], nudge), sigma(z[:, 3 * H:], nudge)
        c = f * c + i * g
        tc = tanh(c, nudge)
        h = o * tc
        for k, v in zip(("i", "f", "g", "o", "c", "tc", "h"), (i, f, g, o, c, tc, h)):
            out[k][:, t] = v
    out["ys"] = np.stack([_mm(out["h"][b], W_fc.T, reverse) + b_fc for b in range(B)])
    return out


def train(U, D, init, transient=0, in_scale=None, in_shift=None, t_scale=None, t_shift=None, epochs=50, lr=0.01,
          betas=(0.9, 0.999), eps=1e-8, dtype=np.float64, reverse=False, nudge=False):
    """esn_lstm_train for one group: U [T_in, n_in], D [T, n_out], init = the six arrays of that group.  Returns
    dict(W_ih .. b_fc, loss [epochs])."""
    D = np.asarray(D, dtype=dtype)
    T, n_out = D.shape
    x = scaled_inputs(U, T, in_scale, in_shift, dtype)
    Ds = D
    if t_scale is not None:
        Ds = Ds * np.asarray(t_scale, dtype=dtype)
    if t_shift is not None:
        Ds = Ds + np.asarray(t_shift, dtype=dtype)
    prm = [np.array(t, dtype=dtype) for t in init]
    m = [np.zeros_like(t) for t in prm]
    v = [np.zeros_like(t) for t in prm]
    one, two, zero = dtype(1), dtype(2), dtype(0)
    beta1, beta2, lr, eps = dtype(betas[0]), dtype(betas[1]), dtype(lr), dtype(eps)
    n = dtype((T - transient) * n_out)
    on = (np.arange(T) >= transient)[:, None]
    H = prm[1].shape[1]
    tsum = (lambda a: a[::-1].sum(axis=0)) if reverse else (lambda a: a.sum(axis=0))
    loss = []
    for e in range(1, epochs + 1):
        W_ih, W_hh, b_ih, b_hh, W_fc, b_fc = prm
        fw = {k: a[0] for k, a in forward(x[None], prm, reverse, nudge).items()}
        diff = np.where(on, fw["ys"] - Ds, zero)
        loss.append((diff * diff).sum() / n)
        dys = two * diff / n
        dz = np.zeros((T, 4 * H), dtype=dtype)
        dz_next = np.zeros((1, 4 * H), dtype=dtype)
        dc_next = np.zeros(H, dtype=dtype)
        for t in range(T - 1, -1, -1):
            i, f, g, o, tc = fw["i"][t], fw["f"][t], fw["g"][t], fw["o"][t], fw["tc"][t]
            c_prev = fw["c"][t - 1] if t > 0 else np.zeros(H, dtype=dtype)
            dh = _mm(dys[t:t + 1], W_fc, reverse)[0] + _mm(dz_next, W_hh, reverse)[0]
            d_o = dh * tc
            dc = dc_next + dh * o * (one - tc * tc)
            d_i, d_g, d_f = dc * g, dc * i, dc * c_prev
            dc_next = dc * f
            dz[t] = np.concatenate([d_i * i * (one - i), d_f * f * (one - f), d_g * (one - g * g), d_o * o * (one - o)])
            dz_next = dz[t:t + 1]
        h_prev = np.concatenate([np.zeros((1, H), dtype=dtype), fw["h"][:-1]])
        db = tsum(dz)
        grads = [_mm(np.ascontiguousarray(dz.T), x, reverse), _mm(np.ascontiguousarray(dz.T), h_prev, reverse), db, db,
                 _mm(np.ascontiguousarray(dys.T), fw["h"], reverse), tsum(dys)]
        step = lr / (one - beta1 ** e)
        rs2 = np.sqrt(one - beta2 ** e)
        for k, q in enumerate(grads):
            m[k] = beta1 * m[k] + (one - beta1) * q
            v[k] = beta2 * v[k] + (one - beta2) * (q * q)
            prm[k] = prm[k] - step * (m[k] / (np.sqrt(v[k]) / rs2 + eps))
    out = dict(zip(NAMES, prm))
    out["loss"] = np.array(loss)
    return out


def train_groups(U, D, init, transient=0, group_offset=0, in_scale=None, in_shift=None, t_scale=None, t_shift=None,
                 groups=None, **kw):
    """U [G, T_in, n_in], D [G, T, n_out], init six arrays [n_isets, ...]: the stacked results of `groups` (all)."""
    n_isets = len(init[0])
    out = []
    for g in (range(len(U)) if groups is None else groups):
        s = (group_offset + g) % n_isets
        out.append(train(U[g], D[g], [t[s] for t in init], transient,
                         None if in_scale is None else in_scale[g], None if in_shift is None else in_shift[g],
                         None if t_scale is None else t_scale[g], None if t_shift is None else t_shift[g], **kw))
    return {n: np.stack([o[n] for o in out]) for n in NAMES + ("loss",)}


def predict(U, frames_per_group, T, transient, prm, in_scale=None, in_shift=None, t_scale=None, t_shift=None,
            dtype=np.float64):
    """esn_lstm_predict: U [B, T_in, n_in], prm six arrays [G, ...] -> Y [B, T - transient, n_out] in `dtype`."""
    out = []
    for f0 in range(0, len(U), frames_per_group):
        g = f0 // frames_per_group
        x = scaled_inputs(U[f0:f0 + frames_per_group], T, None if in_scale is None else in_scale[g],
                          None if in_shift is None else in_shift[g], dtype)
        ys = forward(x, [np.asarray(t[g], dtype=dtype) for t in prm])["ys"]
        if t_shift is not None:
            ys = ys - np.asarray(t_shift[g], dtype=dtype)
        if t_scale is not None:
            ys = ys / np.asarray(t_scale[g], dtype=dtype)
        out.append(ys[:, transient:])
    return np.concatenate(out)
