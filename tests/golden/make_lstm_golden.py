#!/usr/bin/env python
"""Generate tests/golden/lstm.npz by RUNNING THE REFERENCE's LSTM code (its RNNModel).

Runs only where the reference's checkout exists (make_fnn_golden.REF), like make_cnn_golden.py:
    python tests/golden/make_lstm_golden.py

The reference defines its model inside a driver script that runs a whole simulation at import, so the generator parses
the script and compiles only `class RNNModel` and `def trainMIMOModel` into a namespace that holds np, torch, nn and
optim.  No reference text is copied; lstm.npz holds arrays only.

The frames are those of the ELM's case A (make_elm_golden.py: 2x2, N = 64, isi 8, 16-QAM, exponential PDP at 12 dB; one
pilot and two data frames, T = 74).  Under torch.manual_seed(77): trainMIMOModel('RNN', ...) on the pilot -- its 9-list,
the trained parameters as float32 -- and the model's output x_hat_temp [T, 4] on all three frames (:112-113, :543).  The
initial parameters are what RNNModel() draws after the same re-seeding (the model is the first thing trainMIMOModel draws
from torch's generator).

W_hh [400, 100] alone would be 160 KB twice over, so of it the file keeps rows [::8] of the initial and of the trained
matrix and the SHA-256 of the initial float32 bytes; every output depends on all of W_hh, so x_hat_temp covers the rows
that are left out.  The pilot's ESN_input / ESN_output and the three frames' inputs are those of elm.npz (asserted here)
and are read from there."""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_fnn_golden import REF, SEED, definitions  # noqa: E402

NAMES = ("W_ih", "W_hh", "b_ih", "b_hh", "W_fc", "b_fc")
ROWS = slice(None, None, 8)


def params(model):
    t = (model.lstm.weight_ih_l0, model.lstm.weight_hh_l0, model.lstm.bias_ih_l0, model.lstm.bias_hh_l0, model.fc.weight,
         model.fc.bias)
    return [a.detach().numpy().copy() for a in t]


def main():
    torch.set_num_threads(1)
    elm = np.load(os.path.join(HERE, "elm.npz"))
    N, cp, d, isi, n_t = 64, 7, 3, 8, 2
    out = dict(seed=SEED)

    ns = definitions(REF, ["RNNModel", "trainMIMOModel"])
    torch.manual_seed(SEED)
    init = params(ns["RNNModel"]())
    torch.manual_seed(SEED)
    res = ns["trainMIMOModel"]("RNN", elm["y_cp"][0], elm["x_cp"][0], N, n_t, cp, isi)
    ESN_input, ESN_output, model, Delay, idx, dmin, dmax, n_forget, nmse = res
    assert (idx, dmin, dmax) == (3, d, d) and Delay == [d] * 4 and n_forget == d + cp
    assert np.array_equal(ESN_input, elm["a_ESN_input"]) and np.array_equal(ESN_output, elm["a_ESN_output"])
    inputs = elm["a_inputs"]
    assert np.array_equal(inputs[0], ESN_input)
    with torch.no_grad():
        x_hat = np.stack([model(torch.from_numpy(u).float().unsqueeze(0)).squeeze(0).numpy() for u in inputs])
    trained = params(model)
    for name, t0, t1 in zip(NAMES, init, trained):
        assert t0.dtype == t1.dtype == np.float32
        if name == "W_hh":
            out["W_hh_0_sha256"] = hashlib.sha256(np.ascontiguousarray(t0).tobytes()).hexdigest()
            t0, t1 = t0[ROWS], t1[ROWS]
        out[name + "_0"], out[name] = t0, t1
    out.update(x_hat_temp=x_hat.astype(np.float32), Delay=np.array(Delay), nForgetPoints=n_forget, NMSE=nmse)
    path = os.path.join(HERE, "lstm.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; NMSE", float(nmse), "max |W_hh - W_hh_0|",
          float(np.abs(trained[1] - init[1]).max()))


if __name__ == "__main__":
    main()
