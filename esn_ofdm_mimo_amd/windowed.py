"""What the reference's learned comparators (elm.py, and through trained.py fnn.py, cnn.py, lstm.py) share: a model over
the last `window` received rows, trained per pilot, with the ESN's scalings and detector tail.

    WindowedBank        the device bank all build on: sizes, scalings, the checks of predict, detect_count
    mimo_io             the reference's ESN_input / ESN_output of one pilot
    window_rows         its inputs_window
    train_mimo_windowed its trainMIMOModel(...) around a constructed model on windowed rows, for any antenna count
    train_mimo_sequence the same around a model that reads the whole sequence (CNN, LSTM)"""
from __future__ import annotations

import numpy as np

from .bankbase import DetectorTail, DeviceBank, _as_dev


class WindowedBank(DeviceBank, DetectorTail):
    def __init__(self, n_inputs, n_outputs, n_hidden, window, device=None):
        DeviceBank.__init__(self, device)
        self.n_inputs, self.n_outputs, self.n_hidden = int(n_inputs), int(n_outputs), int(n_hidden)
        self.window = int(window)

    def _predict_args(self, U, frames_per_group, T, transient, precision, out, held, unfitted, too_few):
        """The checks of predict, before its kernel call: U [B, T_in, n_in] on the device, 0 <= transient < T and
        T_in <= T, scalings and trained sets (`held`: their tensor, or None before a fit; `unfitted` / `too_few`: what to
        say then) for every group of the batch, and `out` [B, T - transient, n_out].  Returns (U, B, T_in, T, out)."""
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
        if held is None:
            raise AttributeError(unfitted)
        if held.shape[0] < g:
            raise ValueError(too_few.format(held.shape[0], g))
        if out is None:
            with torch.cuda.device(self.device):
                out = torch.empty((b, T - transient, self.n_outputs), dtype=torch.float64, device=self.device)
        return U, b, t_in, T, out


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


def train_mimo_windowed(model, y_CP, x_CP, N, N_t, CyclicPrefixLen, IsiDuration, window, fixed_delay):
    """trainMIMOModel(...) of the reference (:72-159) around `model`, which has the reference's fit / predict on
    windowed rows of 2 n_r window inputs and 2 N_t outputs: returns its 9-list
    [ESN_input, ESN_output, model, Delay, fixed_delay, Delay_Min, Delay_Max, nForgetPoints, NMSE].  Training uses all
    windowed rows, unscaled, as the reference does; nForgetPoints includes `+= window - 1`; NMSE is computed on the
    reference's rows [0, N) of the un-cut output (its slice, kept)."""
    Delay = [fixed_delay] * (2 * N_t)
    ESN_input, ESN_output = mimo_io(y_CP, x_CP, N, N_t, CyclicPrefixLen, fixed_delay)
    nForgetPoints = fixed_delay + CyclicPrefixLen
    inputs_window = window_rows(ESN_input, window)
    targets_window = ESN_output[window - 1:, :]
    model.fit(inputs_window, targets_window)
    x_hat_temp = np.zeros(ESN_output.shape)
    x_hat_temp[window - 1:, :] = model.predict(inputs_window)
    nForgetPoints += window - 1
    x_hat = x_hat_temp[0:N, 0::2] + 1j * x_hat_temp[0:N, 1::2]
    x = np.asarray(x_CP)[IsiDuration - 1:, :]
    NMSE = sum(np.linalg.norm(x_hat[:, i] - x[:, i]) ** 2 / np.linalg.norm(x[:, i]) ** 2 for i in range(N_t))
    return [ESN_input, ESN_output, model, Delay, fixed_delay, fixed_delay, fixed_delay, nForgetPoints, NMSE]


def train_mimo_sequence(model, y_CP, x_CP, N, N_t, CyclicPrefixLen, IsiDuration, fixed_delay):
    """trainMIMOModel(...) of the reference (:72-113, :151-159) around `model`, which has the reference's fit / predict
    on whole sequences of 2 n_r inputs and 2 N_t outputs: returns its 9-list as train_mimo_windowed does.  Training uses
    every row, unscaled, as the reference does; nForgetPoints = delay + CP, with no window term (:91); NMSE is computed
    on the reference's rows [0, N) of the output (its slice, kept)."""
    Delay = [fixed_delay] * (2 * N_t)
    ESN_input, ESN_output = mimo_io(y_CP, x_CP, N, N_t, CyclicPrefixLen, fixed_delay)
    model.fit(ESN_input, ESN_output)
    x_hat_temp = model.predict(ESN_input)
    x_hat = x_hat_temp[0:N, 0::2] + 1j * x_hat_temp[0:N, 1::2]
    x = np.asarray(x_CP)[IsiDuration - 1:, :]
    NMSE = sum(np.linalg.norm(x_hat[:, i] - x[:, i]) ** 2 / np.linalg.norm(x[:, i]) ** 2 for i in range(N_t))
    return [ESN_input, ESN_output, model, Delay, fixed_delay, fixed_delay, fixed_delay, fixed_delay + CyclicPrefixLen,
            NMSE]
