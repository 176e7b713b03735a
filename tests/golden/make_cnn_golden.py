#!/usr/bin/env python
"""Generate tests/golden/cnn.npz by RUNNING THE REFERENCE's CNN code.

Runs only where the reference's checkout exists (make_fnn_golden.REF), like make_fnn_golden.py:
    python tests/golden/make_cnn_golden.py

The reference defines its CNN inside a driver script that runs a whole simulation at import, so the generator parses the
script and compiles only `class CNNModel` and `def trainMIMOModel` into a namespace that holds np, torch, nn and optim.
No reference text is copied; cnn.npz holds arrays only.

The frames are those of the ELM's case A (make_elm_golden.py: 2x2, N = 64, isi 8, 16-QAM, exponential PDP at 12 dB; one
pilot and two data frames, T = 74).  Under torch.manual_seed(77): trainMIMOModel('CNN', ...) on the pilot -- its 9-list,
the trained parameters as float32 -- and the model's output x_hat_temp [T, 4] on all three frames (:112-113, :535).  The
initial parameters are what CNNModel() draws after the same re-seeding (the model is the first thing trainMIMOModel draws
from torch's generator)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_fnn_golden import REF, SEED, definitions  # noqa: E402

NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")


def params(model):
    return [t.detach().numpy().copy() for conv in (model.conv1, model.conv2, model.conv3) for t in (conv.weight, conv.bias)]


def main():
    torch.set_num_threads(1)
    elm = np.load(os.path.join(HERE, "elm.npz"))
    N, cp, d, isi, n_t = 64, 7, 3, 8, 2
    out = dict(ebno=12.0, y_cp=elm["y_cp"], x_cp=elm["x_cp"], seed=SEED)

    ns = definitions(REF, ["CNNModel", "trainMIMOModel"])
    torch.manual_seed(SEED)
    init = params(ns["CNNModel"]())
    torch.manual_seed(SEED)
    res = ns["trainMIMOModel"]("CNN", elm["y_cp"][0], elm["x_cp"][0], N, n_t, cp, isi)
    ESN_input, ESN_output, model, Delay, idx, dmin, dmax, n_forget, nmse = res
    assert (idx, dmin, dmax) == (3, d, d) and Delay == [d] * 4 and n_forget == d + cp
    assert np.array_equal(ESN_input, elm["a_ESN_input"]) and np.array_equal(ESN_output, elm["a_ESN_output"])
    inputs = elm["a_inputs"]
    assert np.array_equal(inputs[0], ESN_input)
    with torch.no_grad():
        x_hat = np.stack([model(torch.from_numpy(u).float().unsqueeze(0)).squeeze(0).numpy().astype(np.float64)
                          for u in inputs])                                                 # :112-113, a frame at a time
    trained = params(model)
    for name, t0, t1 in zip(NAMES, init, trained):
        assert t0.dtype == t1.dtype == np.float32
        out[name + "_0"], out[name] = t0, t1
    out.update(ESN_input=ESN_input, ESN_output=ESN_output, inputs=inputs, x_hat_temp=x_hat, Delay=np.array(Delay),
               nForgetPoints=n_forget, NMSE=nmse)
    path = os.path.join(HERE, "cnn.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; NMSE", float(nmse), "max |W2 - W2_0|", float(np.abs(trained[2] - init[2]).max()))


if __name__ == "__main__":
    main()
