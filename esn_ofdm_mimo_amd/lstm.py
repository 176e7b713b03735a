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

The bank is a windowed.WindowedBank whose `window` is 1 (a row of the output sees every earlier row through the state,
none through a window).  The definition is in include/esn_hip.h; tests/lstm_ref.py restates it in NumPy.  Float64 only
(no fp16 prediction), one pilot per group, one layer, no float32 I/O."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import check, ptr
from .bankbase import _as_dev
from .windowed import WindowedBank, mimo_io

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


class LstmBank(WindowedBank):
    W_ih = W_hh = b_ih = b_hh = W_fc = b_fc = loss = None
    _work = None

    def __init__(self, n_inputs, n_outputs, n_hidden=100, n_groups=1, device=None):
        WindowedBank.__init__(self, n_inputs, n_outputs, n_hidden, 1, device)
        self.n_groups = int(n_groups)

    def _shapes(self, n):
        i, h, o = self.n_inputs, self.n_hidden, self.n_outputs
        return ((n, 4 * h, i), (n, 4 * h, h), (n, 4 * h), (n, 4 * h), (n, o, h), (n, o))

    def _sets(self, params):
        """The six arrays of NAMES, one set or [n_sets, ...] -> six contiguous device tensors [n_sets, ...]."""
        torch = self.torch
        with torch.cuda.device(self.device):
            prm = [_as_dev(t, torch, self.device) for t in params]
        if len(prm) != 6:
            raise ValueError(f"need the six arrays {NAMES}, got {len(prm)}")
        if prm[0].ndim == 2:
            prm = [t[None] for t in prm]
        want = self._shapes(prm[0].shape[0])
        got = tuple(tuple(t.shape) for t in prm)
        if got != want:
            raise ValueError(f"{NAMES} must have shapes {want}, not {got}")
        return [t.contiguous() for t in prm]

    def set_weights(self, W_ih, W_hh, b_ih, b_hh, W_fc, b_fc):
        """Trained parameters, [G, ...] (or one set): what predict reads."""
        self.W_ih, self.W_hh, self.b_ih, self.b_hh, self.W_fc, self.b_fc = self._sets((W_ih, W_hh, b_ih, b_hh, W_fc, b_fc))

    def _workspace(self, n_groups, n_frames, T):
        """The device workspace of a training of n_groups or a prediction of n_frames (under the device guard)."""
        need = int(self.lib.esn_lstm_workspace_bytes(self.n_inputs, self.n_hidden, self.n_outputs, n_groups, n_frames, T))
        if self._work is None or self._work.numel() * 8 < need:
            self._work = None                                  # (release before growing)
            self._work = self.torch.empty(max(1, (need + 7) // 8), dtype=self.torch.float64, device=self.device)
        return self._work

    def _shape_check(self, T, who):
        why = train_shape_error(self.n_inputs, self.n_hidden, self.n_outputs, T)
        if why:
            raise ValueError(f"{who} does not serve this shape: " + why)

    def train(self, U, D, init, transient=0, epochs=50, lr=0.01, betas=(0.9, 0.999), eps=1e-8, group_offset=0,
              want_loss=False):
        """U [G, T_in, n_in], D [G, T, n_out] (T_in <= T: zero rows are appended before scaling); init = the six arrays
        of init_weights, one set or [n_isets, ...]: group g starts from set (group_offset + g) % n_isets.  The loss runs
        over rows [transient, T).  Sets W_ih .. b_fc [G, ...] (and loss [G, epochs], the loss before each step, if
        want_loss); returns self."""
        torch = self.torch
        U, D = _as_dev(U, torch, self.device), _as_dev(D, torch, self.device)
        g, t_in, T = U.shape[0], U.shape[1], D.shape[1]
        if D.shape[0] != g or U.shape[2] != self.n_inputs or D.shape[2] != self.n_outputs or t_in > T:
            raise ValueError(f"U {tuple(U.shape)} and D {tuple(D.shape)} must be [G, T_in, {self.n_inputs}] and "
                             f"[G, T, {self.n_outputs}] with T_in <= T")
        self._shape_check(T, "esn_lstm_train")
        init = self._sets(init)
        self._check_groups(g)
        with torch.cuda.device(self.device):
            kw = dict(dtype=torch.float64, device=self.device)
            out = [torch.empty(s, **kw) for s in self._shapes(g)]
            loss = torch.empty((g, int(epochs)), **kw) if want_loss else None
            work = self._workspace(g, 0, T)
            check(self.lib.esn_lstm_train(_lib.F64, self.n_inputs, self.n_hidden, self.n_outputs, init[0].shape[0],
                                          *[ptr(t) for t in init], ptr(self.in_scale), ptr(self.in_shift),
                                          ptr(self.t_scale), ptr(self.t_shift), ptr(U), ptr(D), g, t_in, T, int(transient),
                                          int(group_offset), int(epochs), float(lr), float(betas[0]), float(betas[1]),
                                          float(eps), *[ptr(t) for t in out], ptr(loss), ptr(work), work.numel() * 8,
                                          _lib.stream_handle()), "esn_lstm_train")
        self.W_ih, self.W_hh, self.b_ih, self.b_hh, self.W_fc, self.b_fc = out
        self.loss = loss
        return self

    def predict(self, U, frames_per_group, T=None, transient=0, precision="f64", out=None):
        """U [B, T_in, n_in] (frames ordered by group) -> Y [B, T - transient, n_out] (device, unscaled); group g reads
        its own trained set, every frame starts from h = c = 0.  precision "f64" only: there is no fp16 instance of the
        LSTM."""
        if precision != "f64":
            raise ValueError(f"precision must be 'f64' (the LSTM has no fp16 prediction), not {precision!r}")
        U, b, t_in, T, out = self._predict_args(U, frames_per_group, T, transient, precision, out, self.W_ih,
                                                "W_ih: train (or set_weights) before predict",
                                                "the bank holds {} trained sets, batch needs {}")
        self._shape_check(T, "esn_lstm_predict")
        with self.torch.cuda.device(self.device):
            work = self._workspace(0, b, T)
            check(self.lib.esn_lstm_predict(_lib.F64, self.n_inputs, self.n_hidden, self.n_outputs,
                                            *[ptr(getattr(self, n)) for n in NAMES], ptr(self.in_scale),
                                            ptr(self.in_shift), ptr(self.t_scale), ptr(self.t_shift), ptr(U), b,
                                            int(frames_per_group), t_in, T, int(transient), ptr(out), ptr(work),
                                            work.numel() * 8, _lib.stream_handle()), "esn_lstm_predict")
        return out


class LSTM:
    """The reference's RNNModel with its training loop (system_model_2_all_comparision.py:29-38, :102-113) on the GPU:
    inputs [T, n_in] and targets [T, n_out] are NumPy sequences, float64.  init None draws
    init_weights(n_in, n_out, n_hidden) from torch's global generator, as the reference does."""

    def __init__(self, n_in=4, n_out=4, n_hidden=100, init=None, epochs=50, lr=0.01):
        self.n_in, self.n_out, self.n_hidden = int(n_in), int(n_out), int(n_hidden)
        self.epochs, self.lr = int(epochs), float(lr)
        init = init_weights(n_in, n_out, n_hidden) if init is None else init
        for n, t in zip(NAMES, init):
            setattr(self, n, np.asarray(t, dtype=np.float64))
        self.loss = None
        self._bank = None

    def _get_bank(self):
        if self._bank is None:
            self._bank = LstmBank(self.n_in, self.n_out, self.n_hidden)
        return self._bank

    def _params(self):
        return tuple(getattr(self, n) for n in NAMES)

    def fit(self, inputs, targets):
        bank = self._get_bank()
        bank.train(np.asarray(inputs, dtype=np.float64)[None], np.asarray(targets, dtype=np.float64)[None],
                   self._params(), transient=0, epochs=self.epochs, lr=self.lr, want_loss=True)
        for n in NAMES:
            setattr(self, n, getattr(bank, n)[0].cpu().numpy())
        self.loss = bank.loss[0].cpu().numpy()

    def predict(self, inputs):
        bank = self._get_bank()
        bank.set_weights(*self._params())
        return bank.predict(np.asarray(inputs, dtype=np.float64)[None], 1).cpu().numpy()[0]


def trainMIMOLSTM(y_CP, x_CP, N, N_t, CyclicPrefixLen, IsiDuration, fixed_delay=3, n_hidden=100, init=None):
    """trainMIMOModel('RNN', ...) of the reference (:72-113, :151-159) for any antenna count: returns its 9-list
    [ESN_input, ESN_output, model, Delay, fixed_delay, Delay_Min, Delay_Max, nForgetPoints, NMSE].  Training uses every
    row, unscaled, as the reference does; nForgetPoints = delay + CP, with no window term (:91); NMSE is computed on the
    reference's rows [0, N) of the output (its slice, kept, as trainMIMOCNN does)."""
    Delay = [fixed_delay] * (2 * N_t)
    ESN_input, ESN_output = mimo_io(y_CP, x_CP, N, N_t, CyclicPrefixLen, fixed_delay)
    model = LSTM(ESN_input.shape[1], 2 * N_t, n_hidden, init=init)
    model.fit(ESN_input, ESN_output)
    x_hat_temp = model.predict(ESN_input)
    x_hat = x_hat_temp[0:N, 0::2] + 1j * x_hat_temp[0:N, 1::2]
    x = np.asarray(x_CP)[IsiDuration - 1:, :]
    NMSE = sum(np.linalg.norm(x_hat[:, i] - x[:, i]) ** 2 / np.linalg.norm(x[:, i]) ** 2 for i in range(N_t))
    return [ESN_input, ESN_output, model, Delay, fixed_delay, fixed_delay, fixed_delay, fixed_delay + CyclicPrefixLen,
            NMSE]
