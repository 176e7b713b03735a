#!/usr/bin/env python
"""Generate tests/golden/fnn.npz by RUNNING THE REFERENCE's FNN code.

Runs only in the build container (where /root/reference exists), like make_elm_golden.py:
    python tests/golden/make_fnn_golden.py

The reference defines its FNN inside a driver script that runs a whole simulation at import, so the generator parses the
script and compiles only `class FNNModel` and `def trainMIMOModel` into a namespace that holds np, torch, nn and optim.
No reference text is copied; fnn.npz holds arrays only.

The frames are those of the ELM's case A (make_elm_golden.py: 2x2, N = 64, isi 8, 16-QAM, exponential PDP at 12 dB; one
pilot and two data frames).  Under torch.manual_seed(77): trainMIMOModel('FNN', ...) on the pilot -- its 9-list, the
trained parameters -- and the model's un-cut output x_hat_temp [T, 4] on all three frames (:144-148, :551-569).  The
initial parameters are what FNNModel(32) draws after the same re-seeding (the model is the first thing trainMIMOModel
draws from torch's generator)."""
import ast
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.optim as optim

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle.ofdm_frames import LinkConfig, exp_pdp_taps, make_frame  # noqa: E402

REF = "/root/reference/system_model_2/system_model_2_all_comparision.py"
SEED = 77


def definitions(path, names):
    tree = ast.parse(open(path).read(), path)
    body = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names]
    assert sorted(n.name for n in body) == sorted(names), [n.name for n in body]
    ns = {"np": np, "torch": torch, "nn": nn, "optim": optim}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


def params(model):
    return [t.detach().numpy().copy() for t in (model.fc1.weight, model.fc1.bias, model.fc2.weight, model.fc2.bias)]


def main():
    torch.set_num_threads(1)
    cfg = LinkConfig(n_t=2, n_r=2, n_sub=64, m=4, isi=8)
    ebno, N, cp, d, window = 12.0, cfg.n_sub, cfg.cp, 3, 8
    rs = np.random.RandomState(20260)
    taps = exp_pdp_taps(cfg, rs)
    frames = [make_frame(cfg, ebno, taps, rs) for _ in range(3)]          # pilot, data, data: the ELM's case A
    elm = np.load(os.path.join(HERE, "elm.npz"))
    assert np.array_equal(np.stack([f["y_cp"] for f in frames]), elm["y_cp"])
    out = dict(ebno=ebno, p_i=cfg.p_i(ebno), y_cp=elm["y_cp"], x_cp=elm["x_cp"], seed=SEED)

    ns = definitions(REF, ["FNNModel", "trainMIMOModel"])
    torch.manual_seed(SEED)
    init = params(ns["FNNModel"](4 * window))
    torch.manual_seed(SEED)
    res = ns["trainMIMOModel"]("FNN", frames[0]["y_cp"], frames[0]["x_cp"], N, cfg.n_t, cp, cfg.isi)
    ESN_input, ESN_output, model, Delay, idx, dmin, dmax, n_forget, nmse = res
    assert (idx, dmin, dmax) == (3, d, d) and Delay == [d] * 4 and n_forget == d + cp + window - 1
    assert np.array_equal(ESN_input, elm["a_ESN_input"]) and np.array_equal(ESN_output, elm["a_ESN_output"])
    inputs = elm["a_inputs"]

    def win(x):         # :117-120
        return np.stack([x[i - window + 1:i + 1].flatten() for i in range(window - 1, x.shape[0])])
    x_hat = np.zeros((3, N + d + cp, 4))
    with torch.no_grad():
        for k in range(3):
            x_hat[k, window - 1:] = model(torch.from_numpy(win(inputs[k])).float()).numpy()     # :144-148
    trained = params(model)
    for name, t0, t1 in zip(("W1", "b1", "W2", "b2"), init, trained):
        out[name + "_0"], out[name] = t0, t1
    out.update(ESN_input=ESN_input, ESN_output=ESN_output, inputs=inputs, x_hat_temp=x_hat, Delay=np.array(Delay),
               nForgetPoints=n_forget, NMSE=nmse)
    path = os.path.join(HERE, "fnn.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; NMSE", float(nmse), "max |W1 - W1_0|", float(np.abs(trained[0] - init[0]).max()))


if __name__ == "__main__":
    main()
