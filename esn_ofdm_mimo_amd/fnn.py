"""The windowed FNN, the reference's second learned comparator of the ESN (system_model_2_all_comparision.py:40-49
`class FNNModel`, :115-122 / :129-149 its windowed use): the ELM's window of received rows feeding Linear -> ReLU ->
Linear, trained per pilot by 50 full-batch Adam steps (lr 0.01, MSE).

    FnnBank        G FNNs on one GPU, batched like ElmBank: train (esn_fnn_train: one workgroup per group, all epochs in
                   one launch) -> predict (esn_fnn_predict: the ELM's fused kernels with ReLU) -> detect_count
    init_weights   the parameters torch.nn.Linear draws, in the reference's order
    FNN            the reference's model surface on already-windowed NumPy matrices
    trainMIMOFNN   the reference's trainMIMOModel('FNN', ...) for any antenna count

What the FNN shares with the windowed ELM (elm.py) is in windowed.py, what it shares with the CNN and the LSTM (the bank's
host side, the model surface) in trained.py.  The definition every layer follows is in
include/esn_hip.h; tests/fnn_ref.py restates it in NumPy.  Float64 training only, one pilot per group, no float32 I/O."""
from __future__ import annotations

import numpy as np

from .trained import TrainedBank, TrainedModel
from .windowed import mimo_io, train_mimo_windowed, window_rows  # noqa: F401  (importable from here)

NAMES = ("W1", "b1", "W2", "b2")
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


class FnnBank(TrainedBank):
    NAMES, ENTRY, train_shape_error = NAMES, "fnn", staticmethod(train_shape_error)
    F16 = True                  # predict runs the ELM's fused kernels with ReLU, both of their precisions

    def _sizes(self):
        return self.n_inputs, self.n_hidden, self.window, self.n_outputs

    def _shapes(self, n):
        k, nh, no = self.window * self.n_inputs, self.n_hidden, self.n_outputs
        return ((n, nh, k), (n, nh), (n, no, nh), (n, no))

    def _workspace_bytes(self, n_groups, n_frames, T):          # the query takes no n_frames ...
        return self.lib.esn_fnn_workspace_bytes(*self._sizes(), n_groups, T)

    def _workspace(self, n_groups, n_frames, T):                # ... and esn_fnn_predict no workspace
        return TrainedBank._workspace(self, n_groups, 0, T) if n_groups else []

    def _shape_check(self, T, who):     # train_shape_error is the training kernel's; the ELM's kernels have wider limits
        if who == "esn_fnn_train":
            TrainedBank._shape_check(self, T, who)

    def train(self, U, D, init, transient=None, **kw):
        """TrainedBank.train, except that transient defaults to window - 1 and is never below it (the rows before the
        first whole window carry no equation)."""
        transient = max(self.window - 1, int(self.window - 1 if transient is None else transient))
        return TrainedBank.train(self, U, D, init, transient, **kw)


class FNN(TrainedModel):
    """The reference's FNNModel with its training loop (system_model_2_all_comparision.py:40-49, :133-145) on the GPU
    (trained.TrainedModel): inputs are NumPy matrices that are already windowed (one row per sample, window = 1 here).
    init None draws init_weights(input_size, hidden_size, output_size) from torch's global generator, as the reference
    does."""
    NAMES = NAMES

    def __init__(self, input_size, hidden_size=100, output_size=4, init=None, epochs=50, lr=0.01):
        self.input_size, self.hidden_size, self.output_size = int(input_size), int(hidden_size), int(output_size)
        TrainedModel.__init__(self, init_weights(input_size, hidden_size, output_size) if init is None else init, epochs,
                              lr)

    def _make_bank(self):
        return FnnBank(self.input_size, self.output_size, self.hidden_size, 1)


def trainMIMOFNN(y_CP, x_CP, N, N_t, CyclicPrefixLen, IsiDuration, hidden_size=100, window=8, fixed_delay=3, init=None):
    """trainMIMOModel('FNN', ...) of the reference (:72-159) for any antenna count: returns its 9-list
    [ESN_input, ESN_output, model, Delay, fixed_delay, Delay_Min, Delay_Max, nForgetPoints, NMSE].  Training uses all
    windowed rows, unscaled, as the reference does; nForgetPoints includes `+= window - 1`; NMSE is computed on the
    reference's rows [0, N) of the un-cut output (its slice, kept, as trainMIMOELM does)."""
    model = FNN(2 * np.shape(y_CP)[1] * window, hidden_size, 2 * N_t, init=init)
    return train_mimo_windowed(model, y_CP, x_CP, N, N_t, CyclicPrefixLen, IsiDuration, window, fixed_delay)
