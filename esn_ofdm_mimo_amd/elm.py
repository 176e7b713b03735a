"""The windowed ELM (extreme learning machine), the reference's pinv-trained comparator of the ESN
(system_model_2_all_comparision.py:51-69 `class ELM`, :115-127 / :147-149 / :551-575 its windowed use): a random tanh
layer over the last `window` received rows, a bias column, and the read-out this project already fits per pilot.

    ElmBank        G ELMs on one GPU, batched like ReservoirBank: features (esn_elm_features) -> solve (the ESN's
                   read-out fit, readout.ReadoutFit, inherited) -> predict (esn_elm_predict, fused) -> detect_count
    ELM            the reference's class surface on already-windowed NumPy matrices
    trainMIMOELM   the reference's trainMIMOModel('ELM', ...) for any antenna count

What the ELM shares with the windowed FNN (fnn.py) is in windowed.py.  The definition every layer follows is in
include/esn_hip.h; tests/elm_ref.py restates it in NumPy."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import PRECISIONS, check, ptr
from .bankbase import _as_dev
from .readout import ReadoutFit
from .windowed import WindowedBank, mimo_io, train_mimo_windowed, window_rows  # noqa: F401  (importable from here)


class ElmBank(WindowedBank, ReadoutFit):
    W_out = fit_status = None

    def __init__(self, n_inputs, n_outputs, n_hidden, window, W_in, b, bias_col=True, n_groups=1, device=None):
        """W_in [n_hidden, window n_inputs] or [n_wsets, ...] (window sample 0 the oldest), b [n_hidden] or
        [n_wsets, n_hidden]: group g reads set (group_offset + g) % n_wsets.  n_groups: how many read-outs the bank
        holds after a fit (the G of every [G, ...] argument)."""
        WindowedBank.__init__(self, n_inputs, n_outputs, n_hidden, window, device)
        self.bias_col, self.n_groups = bool(bias_col), int(n_groups)
        self.cols = self.n_hidden + int(self.bias_col)
        self.set_weights(W_in, b)

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

    def fit(self, U, D, transient=None, method="qr", ridge=None, ridge_grid=None, e_dtype="f64", group_offset=0,
            repair=True):
        """features + solve + set_readout; U [G, T, n_in], D [G, T, n_out]; method, ridge and ridge_grid as in solve
        (ReadoutFit.solve, on the ELM's rows).  transient defaults to window - 1 and is never below it (the rows before
        the first whole window are zero and carry no equation).  repair: groups a Cholesky solve flagged are re-solved
        by QR through resolve_failed (one host read of the status); repair=False leaves fit_status for the caller.
        Returns E."""
        transient = max(self.window - 1, int(self.window - 1 if transient is None else transient))
        rows = np.shape(U)[1] - transient
        lam = ridge if ridge is not None else ridge_grid
        E = self.features(U, e_cols=self.padded_cols(rows, lam, e_dtype), e_dtype=e_dtype, group_offset=group_offset)
        W_out, status = self.solve(E, D, transient, method=method, ridge=ridge, ridge_grid=ridge_grid)
        if repair and (ridge_grid is not None or method != "qr"):
            self.resolve_failed(E, D, transient, W_out, status, ridge=ridge, ridge_grid=ridge_grid)
        self.set_readout(W_out)
        self.fit_status = status
        return E

    def predict(self, U, frames_per_group, T=None, transient=0, precision="f64", group_offset=0, out=None):
        """U [B, T_in, n_in] (frames ordered by group) -> Y [B, T - transient, n_out] (device, unscaled)."""
        U, b, t_in, T, out = self._predict_args(U, frames_per_group, T, transient, precision, out, self.W_out,
                                                "W_out: fit (or set_readout) before predict",
                                                "readout holds {} groups, batch needs {}")
        with self.torch.cuda.device(self.device):
            check(self.lib.esn_elm_predict(PRECISIONS[precision], self.n_inputs, self.n_hidden, self.window,
                                           int(self.bias_col), self.n_wsets, self.n_outputs, ptr(self._W_in),
                                           ptr(self._b), ptr(self.W_out), self.W_out.shape[2], ptr(self.in_scale),
                                           ptr(self.in_shift), ptr(self.t_scale), ptr(self.t_shift), ptr(U), b,
                                           int(frames_per_group), t_in, T, int(transient), int(group_offset), ptr(out),
                                           _lib.stream_handle()), "esn_elm_predict")
        return out


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


def trainMIMOELM(y_CP, x_CP, N, N_t, CyclicPrefixLen, IsiDuration, hidden_size=100, window=8, fixed_delay=3,
                 W_in=None, b=None):
    """trainMIMOModel('ELM', ...) of the reference (:72-159) for any antenna count: returns its 9-list
    [ESN_input, ESN_output, model, Delay, fixed_delay, Delay_Min, Delay_Max, nForgetPoints, NMSE].  nForgetPoints
    includes `+= window - 1`; NMSE is computed on the reference's rows [0, N) of the un-cut output (its slice, kept)."""
    model = ELM(2 * np.shape(y_CP)[1] * window, hidden_size, 2 * N_t)
    if W_in is not None:
        model.W_in, model.b = np.asarray(W_in, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return train_mimo_windowed(model, y_CP, x_CP, N, N_t, CyclicPrefixLen, IsiDuration, window, fixed_delay)
