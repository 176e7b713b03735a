"""The windowed FNN's definition (include/esn_hip.h, restated in tests/fnn_ref.py) against the reference's own numbers
(tests/golden/fnn.npz, written by tests/golden/make_fnn_golden.py from the reference's FNNModel and trainMIMOModel under
torch.manual_seed(77)).  No GPU.

The reference trains in float32; the restatement in float64 cannot meet it closer than float32 rounding carried through
50 Adam steps.  That figure is measured here, not committed: the bound is 4 x the largest difference between the
restatement run in float32 and in float64 on the same inputs (seen for seed 77: reference 3.3e-7, float32 restatement
6.5e-7 from the float64 one, so about 8 x room).  The ratios are printed."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elm_ref  # noqa: E402
import fnn_ref  # noqa: E402
from esn_ofdm_mimo_amd import fnn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "fnn.npz"))
NAMES = ("W1", "b1", "W2", "b2")
WINDOW = 8


def x_hat_temp(prm, dtype):
    """The un-cut output of the three golden frames in `dtype` arithmetic (:144-148)."""
    W1, b1, W2, b2 = (np.asarray(prm[k], dtype=dtype) for k in NAMES)
    out = np.zeros(GOLD["x_hat_temp"].shape)
    for k in range(3):
        x = elm_ref.windows(GOLD["inputs"][k], WINDOW).astype(dtype)
        out[k, WINDOW - 1:] = np.maximum(x @ W1.T + b1, dtype(0)) @ W2.T + b2
    return out


def float32_bound():
    """(restatement in float64, 4 x max |float32 - float64| over the parameters, the same over x_hat_temp)."""
    init = [GOLD[k + "_0"] for k in NAMES]
    r64 = fnn_ref.train(GOLD["ESN_input"], GOLD["ESN_output"], init, WINDOW, 0)
    r32 = fnn_ref.train(GOLD["ESN_input"], GOLD["ESN_output"], init, WINDOW, 0, dtype=np.float32)
    d_prm = max(np.abs(r32[k].astype(np.float64) - r64[k]).max() for k in NAMES)
    d_out = np.abs(x_hat_temp(r32, np.float32) - x_hat_temp(r64, np.float64)).max()
    return r64, 4.0 * d_prm, 4.0 * d_out


def test_float64_restatement_meets_the_reference_float32_training():
    r64, b_prm, b_out = float32_bound()
    assert r64["min_pre"] > 1e-9, r64["min_pre"]                  # no ReLU on its kink
    for k in NAMES:
        err = np.abs(r64[k] - GOLD[k]).max()
        print(k, "reference vs float64 restatement", err, "bound", b_prm, "ratio", err / b_prm)
        assert err <= b_prm
    err = np.abs(x_hat_temp(r64, np.float64) - GOLD["x_hat_temp"]).max()
    print("x_hat_temp", err, "bound", b_out, "ratio", err / b_out)
    assert err <= b_out
    assert not GOLD["x_hat_temp"][:, :WINDOW - 1].any()
    assert r64["loss"][-1] < 0.05 * r64["loss"][0]                # it did train
    # the restated prediction is the same function
    Y = fnn_ref.predict(GOLD["inputs"][:, :71], 3, 74, 0, *(r64[k][None] for k in NAMES), WINDOW)
    assert np.abs(Y - x_hat_temp(r64, np.float64)).max() <= 1e-13


def test_init_weights_draws_what_the_reference_model_draws():
    import torch
    torch.manual_seed(int(GOLD["seed"]))
    got = fnn.init_weights(4 * WINDOW, 100, 4)
    for k, t in zip(NAMES, got):
        assert t.dtype == np.float64
        np.testing.assert_array_equal(t, GOLD[k + "_0"].astype(np.float64))


def test_a_unit_that_is_never_active_keeps_its_parameters_bitwise():
    init = [GOLD[k + "_0"].astype(np.float64) for k in NAMES]
    dead = 17
    init[1][dead] = -100.0
    for dtype in (np.float64, np.float32):
        r = fnn_ref.train(GOLD["ESN_input"], GOLD["ESN_output"], init, WINDOW, 0, dtype=dtype)
        want = [np.asarray(t, dtype=dtype) for t in init]
        np.testing.assert_array_equal(r["W1"][dead], want[0][dead])
        assert r["b1"][dead] == want[1][dead]
        np.testing.assert_array_equal(r["W2"][:, dead], want[2][:, dead])
        assert all(np.isfinite(r[k]).all() for k in NAMES)
        assert np.abs(r["W1"][dead - 1] - want[0][dead - 1]).max() > 1e-3       # its neighbour moved


def test_the_served_shape_rule_holds_the_reference_shapes():
    assert fnn.train_shape_error(4, 100, 8, 4, 74) is None                     # K = 32
    assert fnn.train_shape_error(16, 100, 8, 8, 138) is None                   # K = 128
    assert fnn.train_shape_error(16, 64, 16, 2, 40) is None                    # n_hidden K = 16384
    assert "LDS" in fnn.train_shape_error(16, 128, 8, 8, 138)
    assert "n_hidden" in fnn.train_shape_error(4, 600, 1, 1, 20)
    assert "window" in fnn.train_shape_error(32, 10, 16, 1, 20)
