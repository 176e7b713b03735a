"""The windowed CNN, the reference's third learned comparator of the ESN (system_model_2_all_comparision.py:14-27
`class CNNModel`, :93-113 its use): Conv1d -> ReLU -> Conv1d -> ReLU -> Conv1d (n_in -> 32 -> 64 -> n_out, kernel 5, zero
padding 2) over the whole received sequence, trained per pilot by 50 full-batch Adam steps (lr 0.01, MSE).

    CnnBank        G CNNs on one GPU, batched like FnnBank: train (esn_cnn_train: one workgroup per group, all epochs in
                   one launch, every product on the float64 matrix pipe) -> predict (esn_cnn_predict) -> detect_count
    init_weights   the parameters three torch.nn.Conv1d draw, in the reference's order
    CNN            the reference's model surface on NumPy sequences
    trainMIMOCNN   the reference's trainMIMOModel('CNN', ...) for any antenna count

The bank is a trained.TrainedBank whose `window` is the kernel size (a row of the output sees 3 (k - 1) + 1 input rows
centred on it) and whose n_hidden is the last hidden channel count.  The definition every layer follows is in
include/esn_hip.h; tests/cnn_ref.py restates it in NumPy.  Float64 only (no fp16 prediction), one pilot per group, no
float32 I/O."""
from __future__ import annotations

import numpy as np

from .trained import TrainedBank, TrainedModel
from .windowed import train_mimo_sequence

NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")


def train_shape_error(n_in, c1, c2, n_out, kernel, T):
    """None if esn_cnn_train / esn_cnn_predict serve the shape, else the limit it misses (the rule of
    include/esn_hip.h and cnn_shape_limit in csrc/esn_cnn.hip, on the host)."""
    if not 1 <= n_in <= 64:
        return f"n_in = {n_in}: served from 1 to 64"
    if not (1 <= c1 <= 128 and 1 <= c2 <= 128):
        return f"channels = ({c1}, {c2}): each served from 1 to 128"
    if not 1 <= n_out <= 8:
        return f"n_out = {n_out}: served up to 8"
    if kernel not in (1, 3, 5, 7):
        return f"kernel = {kernel}: served are the odd sizes 1, 3, 5 and 7"
    if not 1 <= T <= 4096:
        return f"T = {T}: served from 1 to 4096"
    return None


def init_weights(n_in=4, n_out=4, channels=(32, 64), kernel=5):
    """(W1 [c1, n_in, k], b1, W2 [c2, c1, k], b2, W3 [n_out, c2, k], b3) as float64 NumPy arrays: three torch.nn.Conv1d
    built in that order on the CPU -- under torch.manual_seed(s) exactly what the reference's CNNModel() draws."""
    import torch
    c = (int(n_in), int(channels[0]), int(channels[1]), int(n_out))
    convs = [torch.nn.Conv1d(c[l], c[l + 1], kernel_size=kernel, padding=(kernel - 1) // 2) for l in range(3)]
    return tuple(t.detach().numpy().astype(np.float64) for conv in convs for t in (conv.weight, conv.bias))


class CnnBank(TrainedBank):
    NAMES, ENTRY, train_shape_error = NAMES, "cnn", staticmethod(train_shape_error)

    def __init__(self, n_inputs, n_outputs, channels=(32, 64), kernel=5, n_groups=1, device=None):
        channels = tuple(int(c) for c in channels)
        if len(channels) != 2:
            raise ValueError(f"channels must be (c1, c2), not {channels!r}")
        self.channels, self.kernel = channels, int(kernel)
        TrainedBank.__init__(self, n_inputs, n_outputs, channels[1], kernel, n_groups, device)

    def _sizes(self):
        return (self.n_inputs,) + self.channels + (self.n_outputs, self.kernel)

    def _shapes(self, n):
        c, k = (self.n_inputs,) + self.channels + (self.n_outputs,), self.kernel
        return tuple(s for l in range(3) for s in ((n, c[l + 1], c[l], k), (n, c[l + 1])))


class CNN(TrainedModel):
    """The reference's CNNModel with its training loop (system_model_2_all_comparision.py:14-27, :102-113) on the GPU
    (trained.TrainedModel).  init None draws init_weights(n_in, n_out, channels, kernel) from torch's global generator,
    as the reference does."""
    NAMES = NAMES

    def __init__(self, n_in=4, n_out=4, channels=(32, 64), kernel=5, init=None, epochs=50, lr=0.01):
        self.n_in, self.n_out, self.channels, self.kernel = int(n_in), int(n_out), tuple(channels), int(kernel)
        TrainedModel.__init__(self, init_weights(n_in, n_out, channels, kernel) if init is None else init, epochs, lr)

    def _make_bank(self):
        return CnnBank(self.n_in, self.n_out, self.channels, self.kernel)


def trainMIMOCNN(y_CP, x_CP, N, N_t, CyclicPrefixLen, IsiDuration, fixed_delay=3, init=None):
    """trainMIMOModel('CNN', ...) of the reference (:72-113, :151-159) for any antenna count: returns its 9-list
    [ESN_input, ESN_output, model, Delay, fixed_delay, Delay_Min, Delay_Max, nForgetPoints, NMSE].  Training uses every
    row, unscaled, as the reference does; nForgetPoints = delay + CP, with no window term (:91); NMSE is computed on the
    reference's rows [0, N) of the output (its slice, kept, as trainMIMOFNN does)."""
    model = CNN(2 * np.shape(y_CP)[1], 2 * N_t, init=init)
    return train_mimo_sequence(model, y_CP, x_CP, N, N_t, CyclicPrefixLen, IsiDuration, fixed_delay)
