"""The windowed FNN, the reference's second learned comparator of the ESN (system_model_2_all_comparision.py:40-49
`class FNNModel`, :115-122 / :129-149 its windowed use): the ELM's window of received rows feeding Linear -> ReLU ->
Linear, trained per pilot by 50 full-batch Adam steps (lr 0.01, MSE).

    FnnBank        G FNNs on one GPU, batched like ElmBank: train (esn_fnn_train: one workgroup per group, all epochs in
                   one launch) -> predict (esn_fnn_predict: the ELM's fused kernels with ReLU) -> detect_count
    init_weights   the parameters torch.nn.Linear draws, in the reference's order
    FNN            the reference's model surface on already-windowed NumPy matrices
    trainMIMOFNN   the reference's trainMIMOModel('FNN', ...) for any antenna count

What the FNN shares with the windowed ELM (elm.py) is in windowed.py.  The definition every layer follows is in
include/esn_hip.h; tests/fnn_ref.py restates it in NumPy.  Float64 training only, one pilot per group, no float32 I/O."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import PRECISIONS, check, ptr
from .bankbase import _as_dev
from .windowed import WindowedBank, mimo_io, train_mimo_windowed, window_rows  # noqa: F401  (importable from here)

LDS_BYTES = 160 * 1024


def train_shape_error(n_in, n_hidden, window, n_out, T):
    """None if esn_fnn_train serves the shape, else the limit it misses (the rule of include/esn_hip.h, on the host)."""
    k = window * n_in
    if not (1 <= window <= 16 and n_in >= 1 and k <= 256):
        return f"window = {window}, window * n_in = {k}: served up to window 16 and K = 256"
    if not 1 <= n_out <= 8:
        return f"n_out = {n_out}: served up to 8"
    if not (1 <= n_hidden <= 512 and n_out * n_hidden <= 1024 and -(-n_hidden // 4) * -(-k // 8) <= 512):
        return (f"n_hidden = {n_hidden}, K = {k}, n_out = {n_out}: served up to n_hidden 512, n_out n_hidden 1024 and "
                "ceil(n_hidden / 4) ceil(K / 8) = 512")
    lds = 8 * (n_hidden * (k | 1) + (T * n_in + 1) // 2 * 2 + n_out * n_hidden + n_hidden + n_out + 32 * (n_hidden | 1)
               + 256)
    if lds > LDS_BYTES:
        return f"n_hidden = {n_hidden}, K = {k}, T = {T}: {lds} bytes of LDS, served up to {LDS_BYTES}"
    return None


def init_weights(k, n_hidden, n_out):
    """(W1 [n_hidden, k], b1, W2 [n_out, n_hidden], b2) as float64 NumPy arrays: torch.nn.Linear(k, n_hidden), then
    torch.nn.Linear(n_hidden, n_out), built on the CPU -- under torch.manual_seed(s) exactly what the reference's
    FNNModel(k) draws."""
    import torch
    fc1 = torch.nn.Linear(k, n_hidden)
    fc2 = torch.nn.Linear(n_hidden, n_out)
    return tuple(t.detach().numpy().astype(np.float64) for t in (fc1.weight, fc1.bias, fc2.weight, fc2.bias))


class FnnBank(WindowedBank):
    W1 = b1 = W2 = b2 = loss = None
    _work = None

    def __init__(self, n_inputs, n_outputs, n_hidden, window, n_groups=1, device=None):
        WindowedBank.__init__(self, n_inputs, n_outputs, n_hidden, window, device)
        self.n_groups = int(n_groups)

    def _sets(self, params):
        """(W1, b1, W2, b2), one set or [n_sets, ...] -> four contiguous device tensors [n_sets, ...]."""
        torch, k, nh, no = self.torch, self.window * self.n_inputs, self.n_hidden, self.n_outputs
        with torch.cuda.device(self.device):
            W1, b1, W2, b2 = (_as_dev(t, torch, self.device) for t in params)
        if W1.ndim == 2:
            W1, b1, W2, b2 = W1[None], b1[None], W2[None], b2[None]
        n = W1.shape[0]
        want = ((n, nh, k), (n, nh), (n, no, nh), (n, no))
        got = tuple(tuple(t.shape) for t in (W1, b1, W2, b2))
        if got != want:
            raise ValueError(f"(W1, b1, W2, b2) must have shapes {want}, not {got}")
        return W1.contiguous(), b1.contiguous(), W2.contiguous(), b2.contiguous()

    def set_weights(self, W1, b1, W2, b2):
        """Trained parameters, [G, ...] (or one set): what predict reads."""
        self.W1, self.b1, self.W2, self.b2 = self._sets((W1, b1, W2, b2))

    def train(self, U, D, init, transient=None, epochs=50, lr=0.01, betas=(0.9, 0.999), eps=1e-8, group_offset=0,
              want_loss=False):
        """U [G, T_in, n_in], D [G, T, n_out] (T_in <= T: zero rows are appended before scaling); init = (W1, b1, W2, b2),
        one set or [n_isets, ...]: group g starts from set (group_offset + g) % n_isets.  transient defaults to
        window - 1 and is never below it.  Sets W1, b1, W2, b2 [G, ...] (and loss [G, epochs], the loss before each
        step, if want_loss); returns self."""
        torch = self.torch
        U, D = _as_dev(U, torch, self.device), _as_dev(D, torch, self.device)
        g, t_in, T = U.shape[0], U.shape[1], D.shape[1]
        if D.shape[0] != g or U.shape[2] != self.n_inputs or D.shape[2] != self.n_outputs or t_in > T:
            raise ValueError(f"U {tuple(U.shape)} and D {tuple(D.shape)} must be [G, T_in, {self.n_inputs}] and "
                             f"[G, T, {self.n_outputs}] with T_in <= T")
        transient = max(self.window - 1, int(self.window - 1 if transient is None else transient))
        why = train_shape_error(self.n_inputs, self.n_hidden, self.window, self.n_outputs, T)
        if why:
            raise ValueError("esn_fnn_train does not serve this shape: " + why)
        W1_0, b1_0, W2_0, b2_0 = self._sets(init)
        self._check_groups(g)
        k = self.window * self.n_inputs
        with torch.cuda.device(self.device):
            kw = dict(dtype=torch.float64, device=self.device)
            W1, b1 = torch.empty((g, self.n_hidden, k), **kw), torch.empty((g, self.n_hidden), **kw)
            W2, b2 = torch.empty((g, self.n_outputs, self.n_hidden), **kw), torch.empty((g, self.n_outputs), **kw)
            loss = torch.empty((g, int(epochs)), **kw) if want_loss else None
            need = int(self.lib.esn_fnn_workspace_bytes(self.n_inputs, self.n_hidden, self.window, self.n_outputs, g, T))
            if self._work is None or self._work.numel() * 8 < need:
                self._work = torch.empty(max(1, (need + 7) // 8), **kw)
            check(self.lib.esn_fnn_train(_lib.F64, self.n_inputs, self.n_hidden, self.window, self.n_outputs,
                                         W1_0.shape[0], ptr(W1_0), ptr(b1_0), ptr(W2_0), ptr(b2_0), ptr(self.in_scale),
                                         ptr(self.in_shift), ptr(self.t_scale), ptr(self.t_shift), ptr(U), ptr(D), g, t_in,
                                         T, transient, int(group_offset), int(epochs), float(lr), float(betas[0]),
                                         float(betas[1]), float(eps), ptr(W1), ptr(b1), ptr(W2), ptr(b2), ptr(loss),
                                         ptr(self._work), self._work.numel() * 8, _lib.stream_handle()), "esn_fnn_train")
        self.W1, self.b1, self.W2, self.b2, self.loss = W1, b1, W2, b2, loss
        return self

    def predict(self, U, frames_per_group, T=None, transient=0, precision="f64", out=None):
        """U [B, T_in, n_in] (frames ordered by group) -> Y [B, T - transient, n_out] (device, unscaled); group g reads
        its own trained set."""
        U, b, t_in, T, out = self._predict_args(U, frames_per_group, T, transient, precision, out, self.W1,
                                                "W1: train (or set_weights) before predict",
                                                "the bank holds {} trained sets, batch needs {}")
        with self.torch.cuda.device(self.device):
            check(self.lib.esn_fnn_predict(PRECISIONS[precision], self.n_inputs, self.n_hidden, self.window,
                                           self.n_outputs, ptr(self.W1), ptr(self.b1), ptr(self.W2), ptr(self.b2),
                                           ptr(self.in_scale), ptr(self.in_shift), ptr(self.t_scale), ptr(self.t_shift),
                                           ptr(U), b, int(frames_per_group), t_in, T, int(transient), ptr(out),
                                           _lib.stream_handle()), "esn_fnn_predict")
        return out


class FNN:
    """The reference's FNNModel with its training loop (system_model_2_all_comparision.py:40-49, :133-145) on the GPU:
    inputs are NumPy matrices that are already windowed (one row per sample, window = 1 here), float64.  init None
    draws init_weights(input_size, hidden_size, output_size) from torch's global generator, as the reference does."""

    def __init__(self, input_size, hidden_size=100, output_size=4, init=None, epochs=50, lr=0.01):
        self.input_size, self.hidden_size, self.output_size = int(input_size), int(hidden_size), int(output_size)
        self.epochs, self.lr = int(epochs), float(lr)
        init = init_weights(input_size, hidden_size, output_size) if init is None else init
        self.W1, self.b1, self.W2, self.b2 = (np.asarray(t, dtype=np.float64) for t in init)
        self.loss = None
        self._bank = None

    def _get_bank(self):
        if self._bank is None:
            self._bank = FnnBank(self.input_size, self.output_size, self.hidden_size, 1)
        return self._bank

    def fit(self, inputs, targets):
        bank = self._get_bank()
        bank.train(np.asarray(inputs, dtype=np.float64)[None], np.asarray(targets, dtype=np.float64)[None],
                   (self.W1, self.b1, self.W2, self.b2), transient=0, epochs=self.epochs, lr=self.lr, want_loss=True)
        self.W1, self.b1, self.W2, self.b2 = (t[0].cpu().numpy() for t in (bank.W1, bank.b1, bank.W2, bank.b2))
        self.loss = bank.loss[0].cpu().numpy()

    def predict(self, inputs):
        bank = self._get_bank()
        bank.set_weights(self.W1, self.b1, self.W2, self.b2)
        return bank.predict(np.asarray(inputs, dtype=np.float64)[None], 1).cpu().numpy()[0]


def trainMIMOFNN(y_CP, x_CP, N, N_t, CyclicPrefixLen, IsiDuration, hidden_size=100, window=8, fixed_delay=3, init=None):
    """trainMIMOModel('FNN', ...) of the reference (:72-159) for any antenna count: returns its 9-list
    [ESN_input, ESN_output, model, Delay, fixed_delay, Delay_Min, Delay_Max, nForgetPoints, NMSE].  Training uses all
    windowed rows, unscaled, as the reference does; nForgetPoints includes `+= window - 1`; NMSE is computed on the
    reference's rows [0, N) of the un-cut output (its slice, kept, as trainMIMOELM does)."""
    model = FNN(2 * np.shape(y_CP)[1] * window, hidden_size, 2 * N_t, init=init)
    return train_mimo_windowed(model, y_CP, x_CP, N, N_t, CyclicPrefixLen, IsiDuration, window, fixed_delay)
