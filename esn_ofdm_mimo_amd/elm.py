"""The windowed ELM (extreme learning machine), the reference's pinv-trained comparator of the ESN
(system_model_2_all_comparision.py:51-69 `class ELM`, :115-127 / :147-149 / :551-575 its windowed use): a random tanh
layer over the last `window` received rows, a bias column, and the read-out this project already fits per pilot.

    ElmBank        G ELMs on one GPU, batched like ReservoirBank: features (esn_elm_features) -> solve (the read-out
                   kernels, through ReservoirBank.solve) -> predict (esn_elm_predict, fused) -> detect_count
    ELM            the reference's class surface on already-windowed NumPy matrices
    trainMIMOELM   the reference's trainMIMOModel('ELM', ...) for any antenna count

The definition every layer follows is in include/esn_hip.h; tests/elm_ref.py restates it in NumPy."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import PRECISIONS, check, ptr
from .batched import ReservoirBank, _as_dev


class ElmBank:
    def __init__(self, n_inputs, n_outputs, n_hidden, window, W_in, b, bias_col=True, n_groups=1, device=None):
        """W_in [n_hidden, window n_inputs] or [n_wsets, ...] (window sample 0 the oldest), b [n_hidden] or
        [n_wsets, n_hidden]: group g reads set (group_offset + g) % n_wsets.  n_groups: how many read-outs the bank
        holds after a fit (the G of every [G, ...] argument)."""
        torch = _lib.require_gpu()
        self.torch, self.lib = torch, _lib.load()
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self.n_inputs, self.n_outputs, self.n_hidden = int(n_inputs), int(n_outputs), int(n_hidden)
        self.window, self.bias_col, self.n_groups = int(window), bool(bias_col), int(n_groups)
        self.cols = self.n_hidden + int(self.bias_col)
        # the read-out fit is the ESN's: one dispatch table, one repair rule (a one-unit bank is its carrier)
        self._ro = ReservoirBank(self.n_inputs, self.n_outputs, 1, np.zeros((1, 1)), np.zeros((1, self.n_inputs)),
                                 np.zeros((1, self.n_outputs)), noise=0.0, device=self.device)
        self.set_weights(W_in, b)
        self.in_scale = self.in_shift = self.t_scale = self.t_shift = None
        self.W_out = self.fit_status = None

    def set_weights(self, W_in, b):
        torch, k = self.torch, self.window * self.n_inputs
        with torch.cuda.device(self.device):
            W_in, b = _as_dev(W_in, torch, self.device), _as_dev(b, torch, self.device)
        if W_in.ndim == 2:
            W_in, b = W_in[None], b[None]
        if tuple(W_in.shape[1:]) != (self.n_hidden, k) or tuple(b.shape) != (W_in.shape[0], self.n_hidden):
            raise ValueError(f"W_in must be [n_wsets, {self.n_hidden}, {k}] and b [n_wsets, {self.n_hidden}], not "
                             f"{tuple(W_in.shape)} and {tuple(b.shape)}")
        self.n_wsets, self._W_in, self._b = W_in.shape[0], W_in.contiguous(), b.contiguous()

    def set_scaling(self, in_scale=None, in_shift=None, t_scale=None, t_shift=None):
        """Per-group scalings, each [G, n] (or None = identity), as ReservoirBank.set_scaling."""
        self._ro.set_scaling(in_scale, in_shift, t_scale, t_shift)
        self.in_scale, self.in_shift = self._ro.in_scale, self._ro.in_shift
        self.t_scale, self.t_shift = self._ro.t_scale, self._ro.t_shift

    def set_readout(self, W_out):
        """W_out [G, n_out, e_cols] with n_hidden + bias_col <= e_cols <= n_hidden + 4 (float64)."""
        W_out = _as_dev(W_out, self.torch, self.device)
        self.W_out = (W_out[None] if W_out.ndim == 2 else W_out).contiguous()

    def padded_cols(self, rows, ridge=None, e_dtype="f64"):
        """Columns of E for a fit over `rows` rows: padded with zero columns to the solve kernels' 16-byte row (4
        float32 or 2 float64 columns) only where a zero column changes nothing -- rows < cols (minimum norm) or a ridge
        fit; with rows >= cols and pinv it would make the Gram matrix singular."""
        q = 4 if e_dtype == "f32" else 2
        if rows < self.cols or ridge is not None:
            return (self.cols + q - 1) // q * q
        return self.cols

    def _check_groups(self, g):
        for name in ("in_scale", "in_shift", "t_scale", "t_shift"):
            t = getattr(self, name)
            if t is not None and t.shape[0] < g:
                raise ValueError(f"{name} holds {t.shape[0]} groups, batch has {g}")

    def features(self, U, T=None, e_cols=None, e_dtype="f64", group_offset=0):
        """U [G, T_in, n_in] -> E [G, T, e_cols] (device): zero rows before the first whole window, then
        tanh | 1 | zero pad.  e_dtype "f32": the float64 value rounded."""
        torch = self.torch
        if e_dtype not in ("f64", "f32"):
            raise ValueError("e_dtype must be 'f64' or 'f32'")
        U = _as_dev(U, torch, self.device)
        g, t_in = U.shape[0], U.shape[1]
        T = t_in if T is None else int(T)
        e_cols = self.cols if e_cols is None else int(e_cols)
        self._check_groups(g)
        with torch.cuda.device(self.device):
            E = torch.empty((g, T, e_cols), dtype=torch.float32 if e_dtype == "f32" else torch.float64, device=self.device)
            check(self.lib.esn_elm_features(_lib.F64, self.n_inputs, self.n_hidden, self.window, int(self.bias_col),
                                            self.n_wsets, ptr(self._W_in), ptr(self._b), ptr(self.in_scale),
                                            ptr(self.in_shift), ptr(U), g, t_in, T, int(group_offset), ptr(E),
                                            int(e_dtype == "f32"), e_cols, _lib.stream_handle()), "esn_elm_features")
        return E

    def solve(self, E, D, transient, method="qr", ridge=None, ridge_grid=None):
        """ReservoirBank.solve on the ELM's rows: (W_out, status), the same methods, ridge and ridge_grid."""
        return self._ro.solve(E, D, transient, method=method, ridge=ridge, ridge_grid=ridge_grid)

    def fit(self, U, D, transient=None, method="qr", ridge=None, ridge_grid=None, e_dtype="f64", group_offset=0,
            repair=True):
        """features + solve + set_readout; U [G, T, n_in], D [G, T, n_out].  transient defaults to window - 1 and is
        never below it (the rows before the first whole window are zero and carry no equation).  repair: groups a
        Cholesky solve flagged are re-solved by QR, as ReservoirBank.resolve_failed does (one host read of the status);
        repair=False leaves fit_status for the caller.  Returns E."""
        transient = max(self.window - 1, int(self.window - 1 if transient is None else transient))
        rows = np.shape(U)[1] - transient
        lam = ridge if ridge is not None else ridge_grid
        E = self.features(U, e_cols=self.padded_cols(rows, lam, e_dtype), e_dtype=e_dtype, group_offset=group_offset)
        W_out, status = self.solve(E, D, transient, method=method, ridge=ridge, ridge_grid=ridge_grid)
        if repair and (ridge_grid is not None or method != "qr"):
            self._ro.resolve_failed(E, D, transient, W_out, status, ridge=ridge, ridge_grid=ridge_grid)
        self.set_readout(W_out)
        self.fit_status = status
        return E

    def predict(self, U, frames_per_group, T=None, transient=0, precision="f64", group_offset=0, out=None):
        """U [B, T_in, n_in] (frames ordered by group) -> Y [B, T - transient, n_out] (device, unscaled)."""
        torch = self.torch
        if precision not in ("f64", "f16"):
            raise ValueError(f"precision must be 'f64' or 'f16', not {precision!r}")
        U = _as_dev(U, torch, self.device)
        b, t_in = U.shape[0], U.shape[1]
        T = t_in if T is None else int(T)
        if not (0 <= int(transient) < T and t_in <= T):
            raise ValueError(f"need 0 <= transient < T and T_in <= T (transient={transient}, T_in={t_in}, T={T})")
        g = (b + frames_per_group - 1) // frames_per_group
        self._check_groups(g)
        if self.W_out is None:
            raise AttributeError("W_out: fit (or set_readout) before predict")
        if self.W_out.shape[0] < g:
            raise ValueError(f"readout holds {self.W_out.shape[0]} groups, batch needs {g}")
        with torch.cuda.device(self.device):
            if out is None:
                out = torch.empty((b, T - transient, self.n_outputs), dtype=torch.float64, device=self.device)
            check(self.lib.esn_elm_predict(PRECISIONS[precision], self.n_inputs, self.n_hidden, self.window,
                                           int(self.bias_col), self.n_wsets, self.n_outputs, ptr(self._W_in),
                                           ptr(self._b), ptr(self.W_out), self.W_out.shape[2], ptr(self.in_scale),
                                           ptr(self.in_shift), ptr(self.t_scale), ptr(self.t_shift), ptr(U), b,
                                           int(frames_per_group), t_in, T, int(transient), int(group_offset), ptr(out),
                                           _lib.stream_handle()), "esn_elm_predict")
        return out

    def detect_count(self, Y, tx_bits, p_i, frames_per_group, n_sub, n_t, bits_per_sym, err=None, bits=None,
                     want_xhat=False):
        """ReservoirBank.detect_count: Y [B, N, 2 n_t] -> per-group int64 (errors, bits)."""
        return self._ro.detect_count(Y, tx_bits, p_i, frames_per_group, n_sub, n_t, bits_per_sym, err=err, bits=bits,
                                     want_xhat=want_xhat)


class ELM:
    """The reference's class (system_model_2_all_comparision.py:51-69) on the GPU: inputs are NumPy matrices that are
    already windowed (one row per sample, window = 1 here), float64, QR solve.  random_state None draws from the global
    NumPy RNG in the reference's order: uniform(-1, 1, (hidden, input)), then uniform(-1, 1, hidden)."""

    def __init__(self, input_size, hidden_size=100, output_size=4, random_state=None):
        rng = np.random if random_state is None else np.random.RandomState(random_state)
        self.input_size, self.hidden_size, self.output_size = int(input_size), int(hidden_size), int(output_size)
        self.W_in = rng.uniform(-1, 1, (hidden_size, input_size))
        self.b = rng.uniform(-1, 1, hidden_size)
        self.W_out = None
        self._bank = None

    def _get_bank(self):
        if self._bank is None:
            self._bank = ElmBank(self.input_size, self.output_size, self.hidden_size, 1, self.W_in, self.b)
        else:
            self._bank.set_weights(self.W_in, self.b)
        return self._bank

    def fit(self, inputs, targets):
        bank = self._get_bank()
        bank.fit(np.asarray(inputs, dtype=np.float64)[None], np.asarray(targets, dtype=np.float64)[None], transient=0,
                 method="qr")
        self.W_out = bank.W_out[0, :, :bank.cols].cpu().numpy()        # (without the zero weights of pad columns)

    def predict(self, inputs):
        bank = self._get_bank()
        bank.set_readout(self.W_out)
        return bank.predict(np.asarray(inputs, dtype=np.float64)[None], 1).cpu().numpy()[0]


def mimo_io(y_CP, x_CP, N, N_t, CyclicPrefixLen, delay):
    """ESN_input [N + d + CP, 2 n_r] (received rows, d zero rows appended) and ESN_output [N + d + CP, 2 N_t] (the
    teacher delayed by d), real and imaginary parts interleaved per antenna (:78-89)."""
    y_CP, x_CP = np.asarray(y_CP), np.asarray(x_CP)
    T = N + delay + CyclicPrefixLen
    ESN_input = np.zeros((T, 2 * y_CP.shape[1]))
    ESN_output = np.zeros((T, 2 * N_t))
    ESN_input[:T - delay, 0::2], ESN_input[:T - delay, 1::2] = y_CP.real, y_CP.imag
    ESN_output[delay:, 0::2], ESN_output[delay:, 1::2] = x_CP.real, x_CP.imag
    return ESN_input, ESN_output


def window_rows(ESN_input, window):
    """inputs_window of the reference (:117-120): row j is ESN_input[j:j + window].flatten()."""
    return np.stack([ESN_input[j:j + window].reshape(-1) for j in range(ESN_input.shape[0] - window + 1)])


def trainMIMOELM(y_CP, x_CP, N, N_t, CyclicPrefixLen, IsiDuration, hidden_size=100, window=8, fixed_delay=3,
                 W_in=None, b=None):
    """trainMIMOModel('ELM', ...) of the reference (:72-159) for any antenna count: returns its 9-list
    [ESN_input, ESN_output, model, Delay, fixed_delay, Delay_Min, Delay_Max, nForgetPoints, NMSE].  nForgetPoints
    includes `+= window - 1`; NMSE is computed on the reference's rows [0, N) of the un-cut output (its slice, kept)."""
    Delay = [fixed_delay] * (2 * N_t)
    ESN_input, ESN_output = mimo_io(y_CP, x_CP, N, N_t, CyclicPrefixLen, fixed_delay)
    nForgetPoints = fixed_delay + CyclicPrefixLen
    inputs_window = window_rows(ESN_input, window)
    targets_window = ESN_output[window - 1:, :]
    model = ELM(ESN_input.shape[1] * window, hidden_size, 2 * N_t)
    if W_in is not None:
        model.W_in, model.b = np.asarray(W_in, dtype=np.float64), np.asarray(b, dtype=np.float64)
    model.fit(inputs_window, targets_window)
    x_hat_temp = np.zeros(ESN_output.shape)
    x_hat_temp[window - 1:, :] = model.predict(inputs_window)
    nForgetPoints += window - 1
    x_hat = x_hat_temp[0:N, 0::2] + 1j * x_hat_temp[0:N, 1::2]
    x = np.asarray(x_CP)[IsiDuration - 1:, :]
    NMSE = sum(np.linalg.norm(x_hat[:, i] - x[:, i]) ** 2 / np.linalg.norm(x[:, i]) ** 2 for i in range(N_t))
    return [ESN_input, ESN_output, model, Delay, fixed_delay, fixed_delay, fixed_delay, nForgetPoints, NMSE]
