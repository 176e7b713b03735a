#!/usr/bin/env python
"""Generate tests/golden/elm.npz by RUNNING THE REFERENCE's ELM code.

Runs only in the build container (where /root/reference exists), like make_golden.py:
    python tests/golden/make_elm_golden.py

The reference defines its ELMs inside driver scripts that run a whole simulation at import, so the generator parses the
scripts and compiles only the definitions it needs (`class ELM`, `def trainMIMOModel`; `class ELM` and the two
standardize functions of the Demo-2x2 variant) into a namespace that holds NumPy -- the torch branches of trainMIMOModel
are never reached.  No reference text is copied; elm.npz holds arrays only.

Case A  system_model_2_all_comparision.py: 2x2, N = 64, isi 8, 16-QAM, exponential PDP at 12 dB; one pilot and two data
        frames from oracle/ofdm_frames.py.  Under a seeded global RNG: trainMIMOModel('ELM', ...) on the pilot (its
        9-list, the model's W_in / b / W_out, the windowed inputs and targets) and the model's un-cut output
        x_hat_temp [T, 4] on all three frames (:551-569).
Case B  Demo_MIMO_2x2_all_DL_model_comparion.py: no window, 200 normal-weight hidden units, no bias column, ridge
        alpha = 1e-3 on standardised inputs and targets (:19-52, :314-327, :420-437), the same three frames, rows from
        nForgetPoints = delay + CP on."""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle.ofdm_frames import LinkConfig, exp_pdp_taps, make_frame  # noqa: E402

REF_A = "/root/reference/system_model_2/system_model_2_all_comparision.py"
REF_B = "/root/reference/system_model_2/Demo_MIMO_2x2_all_DL_model_comparion.py"


def definitions(path, names):
    """The top-level classes / functions `names` of a script, compiled into a namespace with NumPy only."""
    tree = ast.parse(open(path).read(), path)
    body = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names]
    assert sorted(n.name for n in body) == sorted(names), [n.name for n in body]
    ns = {"np": np}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


def main():
    cfg = LinkConfig(n_t=2, n_r=2, n_sub=64, m=4, isi=8)
    ebno, N, cp, d, window = 12.0, cfg.n_sub, cfg.cp, 3, 8
    rs = np.random.RandomState(20260)
    taps = exp_pdp_taps(cfg, rs)
    frames = [make_frame(cfg, ebno, taps, rs) for _ in range(3)]          # pilot, data, data
    out = dict(ebno=ebno, p_i=cfg.p_i(ebno), taps=taps,
               y_cp=np.stack([f["y_cp"] for f in frames]), x_cp=np.stack([f["x_cp"] for f in frames]),
               bits=np.stack([f["bits"] for f in frames]).astype(np.uint8))

    a = definitions(REF_A, ["ELM", "trainMIMOModel"])
    np.random.seed(77)
    res = a["trainMIMOModel"]("ELM", frames[0]["y_cp"], frames[0]["x_cp"], N, cfg.n_t, cp, cfg.isi)
    ESN_input, ESN_output, model, Delay, idx, dmin, dmax, n_forget, nmse = res
    assert (idx, dmin, dmax) == (3, d, d) and Delay == [d] * 4 and n_forget == d + cp + window - 1

    def io(f):          # ESN_input of any frame as trainMIMOModel builds it (:78-84)
        z = np.zeros((N + d + cp, 4))
        z[:N + cp, 0::2], z[:N + cp, 1::2] = f["y_cp"].real, f["y_cp"].imag
        return z

    def win(x):         # :117-120
        return np.stack([x[i - window + 1:i + 1].flatten() for i in range(window - 1, x.shape[0])])
    assert np.array_equal(io(frames[0]), ESN_input)
    inputs = np.stack([io(f) for f in frames])
    x_hat = np.zeros((3, N + d + cp, 4))
    for k in range(3):
        x_hat[k, window - 1:] = model.predict(win(inputs[k]))            # :567-569
    out.update(a_W_in=model.W_in, a_b=model.b, a_W_out=model.W_out, a_inputs_window=win(ESN_input),
               a_targets_window=ESN_output[window - 1:], a_ESN_input=ESN_input, a_ESN_output=ESN_output,
               a_Delay=np.array(Delay), a_nForgetPoints=n_forget, a_NMSE=nmse, a_inputs=inputs, a_x_hat_temp=x_hat,
               a_cond=np.linalg.cond(np.hstack([np.tanh(win(ESN_input) @ model.W_in.T + model.b),
                                                np.ones((N + d + cp - window + 1, 1))])))

    b = definitions(REF_B, ["ELM", "standardize_fit", "standardize_apply"])
    forget = d + cp                                                        # the ESN trainer's nForgetPoints (:307-316)
    X_tr, Y_tr = ESN_input[forget:], ESN_output[forget:]
    X_mu, X_sigma = b["standardize_fit"](X_tr)
    Y_mu, Y_sigma = b["standardize_fit"](Y_tr)
    elm = b["ELM"](n_hidden=200, activation="tanh", alpha=1e-3, seed=42)
    elm.fit(b["standardize_apply"](X_tr, X_mu, X_sigma), b["standardize_apply"](Y_tr, Y_mu, Y_sigma))
    y_pred = np.stack([elm.predict(b["standardize_apply"](inputs[k][forget:], X_mu, X_sigma)) * Y_sigma + Y_mu
                       for k in range(3)])                                 # :424-437
    out.update(b_W=elm.W, b_b=elm.b, b_W_out=elm.W_out, b_X_mu=X_mu, b_X_sigma=X_sigma, b_Y_mu=Y_mu, b_Y_sigma=Y_sigma,
               b_forget=forget, b_alpha=1e-3, b_Y_pred=y_pred)
    path = os.path.join(HERE, "elm.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; cond(E) of case A", float(out["a_cond"]))


if __name__ == "__main__":
    main()
