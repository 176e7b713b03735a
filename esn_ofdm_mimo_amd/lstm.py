"""The LSTM, the reference's fourth learned comparator of the ESN and the only recurrent one -- the reference calls the
model RNNModel and its curve BER_RNN (system_model_2_all_comparision.py:29-38 `class RNNModel`, :93-113 its use):
nn.LSTM(n_in, 100, batch_first=True) -> nn.Linear(100, n_out) over the whole received sequence, trained per pilot by 50
full-batch Adam steps (lr 0.01, MSE).

    LstmBank       G LSTMs on one GPU, batched like CnnBank: train (esn_lstm_train: one workgroup per group, all epochs
                   in one launch, backpropagation through time against a resident W_hh) -> predict (esn_lstm_predict:
                   16 frames of a group per workgroup, each step a product on the float64 matrix pipe) -> detect_count
    init_weights   the parameters torch.nn.LSTM and torch.nn.Linear draw, in the reference's order
    LSTM           the reference's model surface on NumPy sequences
    trainMIMOLSTM  the reference's trainMIMOModel('RNN', ...) for any antenna count

The bank is a trained.TrainedBank whose `window` is 1 (a row of the output sees every earlier row through the state,
none through a window).  The definition is in include/esn_hip.h; tests/lstm_ref.py restates it in NumPy.  Float64 only
(no fp16 prediction), one pilot per group, one layer, no float32 I/O."""
from __future__ import annotations

import numpy as np

from .trained import TrainedBank, TrainedModel
from .windowed import train_mimo_sequence

NAMES = ("W_ih", "W_hh", "b_ih", "b_hh", "W_fc", "b_fc")


def train_shape_error(n_in, n_hidden, n_out, T):
    """None if esn_lstm_train / esn_lstm_predict serve the shape, else the limit it misses (the rule of
    include/esn_hip.h and lstm_shape_limit in csrc/esn_lstm.hip, on the host)."""
    if not 1 <= n_in <= 64:
        return f"n_in = {n_in}: served from 1 to 64"
    if not 1 <= n_hidden <= 128:
        return f"n_hidden = {n_hidden}: served from 1 to 128"
    if not 1 <= n_out <= 8:
        return f"n_out = {n_out}: served up to 8"
    if not 1 <= T <= 4096:
        return f"T = {T}: served from 1 to 4096"
    return None


def init_weights(n_in=4, n_out=4, n_hidden=100):
    """(W_ih [4H, n_in], W_hh [4H, H], b_ih [4H], b_hh [4H], W_fc [n_out, H], b_fc [n_out]) as float64 NumPy arrays:
    torch.nn.LSTM, then torch.nn.Linear, built in that order on the CPU -- under torch.manual_seed(s) exactly what the
    reference's RNNModel() draws."""
    import torch
    lstm = torch.nn.LSTM(int(n_in), int(n_hidden), batch_first=True)
    fc = torch.nn.Linear(int(n_hidden), int(n_out))
    prm = (lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0, fc.weight, fc.bias)
    return tuple(t.detach().numpy().astype(np.float64) for t in prm)


class LstmBank(TrainedBank):
    NAMES, ENTRY, train_shape_error = NAMES, "lstm", staticmethod(train_shape_error)

    def __init__(self, n_inputs, n_outputs, n_hidden=100, n_groups=1, device=None):
        TrainedBank.__init__(self, n_inputs, n_outputs, n_hidden, 1, n_groups, device)

    def _sizes(self):
        return self.n_inputs, self.n_hidden, self.n_outputs

    def _shapes(self, n):
        i, h, o = self.n_inputs, self.n_hidden, self.n_outputs
        return ((n, 4 * h, i), (n, 4 * h, h), (n, 4 * h), (n, 4 * h), (n, o, h), (n, o))


class LSTM(TrainedModel):
    """The reference's RNNModel with its training loop (system_model_2_all_comparision.py:29-38, :102-113) on the GPU
    (trained.TrainedModel); every frame starts from h = c = 0.  init None draws init_weights(n_in, n_out, n_hidden) from
    torch's global generator, as the reference does."""
    NAMES = NAMES

    def __init__(self, n_in=4, n_out=4, n_hidden=100, init=None, epochs=50, lr=0.01):
        self.n_in, self.n_out, self.n_hidden = int(n_in), int(n_out), int(n_hidden)
        TrainedModel.__init__(self, init_weights(n_in, n_out, n_hidden) if init is None else init, epochs, lr)

    def _make_bank(self):
        return LstmBank(self.n_in, self.n_out, self.n_hidden)


def trainMIMOLSTM(y_CP, x_CP, N, N_t, CyclicPrefixLen, IsiDuration, fixed_delay=3, n_hidden=100, init=None):
    """trainMIMOModel('RNN', ...) of the reference (:72-113, :151-159) for any antenna count: returns its 9-list
    [ESN_input, ESN_output, model, Delay, fixed_delay, Delay_Min, Delay_Max, nForgetPoints, NMSE].  Training uses every
    row, unscaled, as the reference does; nForgetPoints = delay + CP, with no window term (:91); NMSE is computed on the
    reference's rows [0, N) of the output (its slice, kept, as trainMIMOCNN does)."""
    model = LSTM(2 * np.shape(y_CP)[1], 2 * N_t, n_hidden, init=init)
    return train_mimo_sequence(model, y_CP, x_CP, N, N_t, CyclicPrefixLen, IsiDuration, fixed_delay)
