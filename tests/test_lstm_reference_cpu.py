"""The LSTM comparator's definition (include/esn_hip.h, restated in tests/lstm_ref.py) against the reference's own numbers
(tests/golden/lstm.npz, written by tests/golden/make_lstm_golden.py from the reference's RNNModel and trainMIMOModel under
torch.manual_seed(77)), against torch's own LSTM and autograd, the served-shape rule and the C ABI of the three entry
points.  No GPU.

The reference trains in float32; the restatement in float64 cannot meet it closer than float32 rounding carried through
50 Adam steps.  That figure is measured here, not committed: the bound is 4 x the largest difference between the
restatement run in float32 and in float64 on the same inputs, over the parameters and over the outputs.  The ratios are
printed.  lstm.npz keeps W_hh on rows [::8] only (and the SHA-256 of the initial matrix): the initial set of every test
here is what init_weights draws under the golden seed, which the SHA pins."""
import functools
import hashlib
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import c_abi  # noqa: E402
import lstm_ref  # noqa: E402
from lstm_ref import NAMES  # noqa: E402
from esn_ofdm_mimo_amd import _lib, build, lstm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "lstm.npz"))
ELM = np.load(os.path.join(ROOT, "tests", "golden", "elm.npz"))       # the frames: the ELM's case A
ESN_INPUT, ESN_OUTPUT, INPUTS = ELM["a_ESN_input"], ELM["a_ESN_output"], ELM["a_inputs"]
ROWS = slice(None, None, 8)                                           # the rows of W_hh the golden file keeps


def stored(name, a):
    """`a` as lstm.npz stores the parameter `name`."""
    return a[ROWS] if name == "W_hh" else a


@functools.lru_cache(maxsize=None)
def golden_init():
    """What RNNModel() draws under the golden seed, float64 (the float32 values, widened)."""
    import torch
    torch.manual_seed(int(GOLD["seed"]))
    init = lstm.init_weights(4, 4, 100)
    for t in init:
        t.setflags(write=False)
    return init


def x_hat_temp(prm, dtype):
    """The output of the three golden frames in `dtype` arithmetic (:112-113)."""
    return lstm_ref.predict(INPUTS, 3, INPUTS.shape[1], 0, [prm[n][None] for n in NAMES], dtype=dtype).astype(np.float64)


@functools.lru_cache(maxsize=None)
def float32_bound():
    """(restatement in float64, 4 x max |float32 - float64| over the parameters, the same over x_hat_temp)."""
    init = golden_init()
    r64 = lstm_ref.train(ESN_INPUT, ESN_OUTPUT, init)
    r32 = lstm_ref.train(ESN_INPUT, ESN_OUTPUT, init, dtype=np.float32)
    d_prm = max(np.abs(r32[n].astype(np.float64) - r64[n]).max() for n in NAMES)
    d_out = np.abs(x_hat_temp(r32, np.float32) - x_hat_temp(r64, np.float64)).max()
    return r64, 4.0 * d_prm, 4.0 * d_out


def test_init_weights_draws_what_the_reference_model_draws():
    got = golden_init()
    assert [t.shape for t in got] == [(400, 4), (400, 100), (400,), (400,), (4, 100), (4,)]
    for n, t in zip(NAMES, got):
        assert t.dtype == np.float64
        np.testing.assert_array_equal(stored(n, t), GOLD[n + "_0"].astype(np.float64))
    sha = hashlib.sha256(np.ascontiguousarray(got[1].astype(np.float32)).tobytes()).hexdigest()
    assert sha == str(GOLD["W_hh_0_sha256"])


def test_float64_restatement_meets_the_reference_float32_training():
    r64, b_prm, b_out = float32_bound()
    for n in NAMES:
        assert GOLD[n].dtype == np.float32 and stored(n, r64[n]).shape == GOLD[n].shape
        err = np.abs(stored(n, r64[n]) - GOLD[n]).max()
        print(n, "reference vs float64 restatement", err, "bound", b_prm, "ratio", err / b_prm)
        assert err <= b_prm
    err = np.abs(x_hat_temp(r64, np.float64) - GOLD["x_hat_temp"]).max()
    print("x_hat_temp", err, "bound", b_out, "ratio", err / b_out, "loss first / last", r64["loss"][0], r64["loss"][-1])
    assert err <= b_out
    assert r64["loss"][-1] < r64["loss"][0]                       # un-scaled pilot: the loss only halves in 50 epochs
    assert int(GOLD["nForgetPoints"]) == 3 + 7                    # no window term (:91)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "lstm.npz")) < 200 * 1024


def test_one_adam_step_of_the_restatement_is_torch_lstm_autograd_and_adam():
    """float64, T_in < T, transient 2, non-trivial scalings: the parameters after one step within 1e-12, the loss within
    1e-14 relative."""
    import torch
    rs = np.random.RandomState(5)
    n_in, H, n_out, t_in, T, transient = 3, 5, 2, 6, 8, 2
    torch.manual_seed(3)
    prm = lstm.init_weights(n_in, n_out, H)
    U, D = rs.randn(t_in, n_in), rs.randn(T, n_out)
    sc, sh = rs.uniform(0.5, 2, n_in), rs.uniform(-0.2, 0.2, n_in)
    tsc, tsh = rs.uniform(0.5, 2, n_out), rs.uniform(-0.2, 0.2, n_out)
    r = lstm_ref.train(U, D, prm, transient=transient, in_scale=sc, in_shift=sh, t_scale=tsc, t_shift=tsh, epochs=1, lr=0.01)
    net = torch.nn.LSTM(n_in, H, batch_first=True).double()
    fc = torch.nn.Linear(H, n_out).double()
    tp = [net.weight_ih_l0, net.weight_hh_l0, net.bias_ih_l0, net.bias_hh_l0, fc.weight, fc.bias]
    with torch.no_grad():
        for t, a in zip(tp, prm):
            t.copy_(torch.tensor(a))
    x = torch.tensor(lstm_ref.scaled_inputs(U, T, sc, sh))[None]
    ys = fc(net(x)[0])[0]
    loss = ((ys - torch.tensor(D * tsc + tsh))[transient:] ** 2).mean()
    assert abs(float(loss.detach()) - r["loss"][0]) <= 1e-14 * abs(float(loss.detach()))
    opt = torch.optim.Adam(tp, lr=0.01)
    loss.backward()
    opt.step()
    for n, t in zip(NAMES, tp):
        err = np.abs(t.detach().numpy() - r[n]).max()
        print(n, "torch vs restatement after one step", err)
        assert err <= 1e-12, n
    # and the forward pass alone, un-scaled into Y
    Y = lstm_ref.predict(U[None], 1, T, transient, [np.asarray(a)[None] for a in prm], sc[None], sh[None], tsc[None],
                         tsh[None])
    want = ((ys.detach().numpy() - tsh) / tsc)[transient:]
    assert np.abs(Y[0] - want).max() <= 1e-13


def test_with_one_row_the_recurrent_and_forget_gate_parameters_stay_bitwise():
    rs = np.random.RandomState(9)
    n_in, H, n_out = 2, 3, 1
    a = 1.0 / np.sqrt(H)
    init = [rs.uniform(-a, a, s) for s in ((4 * H, n_in), (4 * H, H), (4 * H,), (4 * H,), (n_out, H), (n_out,))]
    U, D = rs.randn(1, n_in), rs.randn(1, n_out)
    fgt = slice(H, 2 * H)
    for dtype in (np.float64, np.float32):
        r = lstm_ref.train(U, D, init, epochs=3, dtype=dtype)
        want = [np.asarray(t, dtype=dtype) for t in init]
        np.testing.assert_array_equal(r["W_hh"], want[1])
        for k in (0, 2, 3):
            np.testing.assert_array_equal(r[NAMES[k]][fgt], want[k][fgt])
            for gate in (0, 2, 3):                                 # every other gate's rows moved
                rows = slice(gate * H, (gate + 1) * H)
                assert np.abs(r[NAMES[k]][rows] - want[k][rows]).min() > 1e-4, (NAMES[k], gate)
        assert np.abs(r["W_fc"] - want[4]).min() > 1e-4 and np.abs(r["b_fc"] - want[5]).min() > 1e-4
        assert all(np.isfinite(r[n]).all() for n in NAMES)


def test_the_served_shape_rule_holds_the_reference_shapes():
    for T in (74, 138, 522):
        assert lstm.train_shape_error(4, 100, 4, T) is None
        assert lstm.train_shape_error(16, 100, 8, T) is None
    assert lstm.train_shape_error(1, 1, 1, 1) is None
    assert lstm.train_shape_error(64, 128, 8, 4096) is None
    assert "n_hidden" in lstm.train_shape_error(4, 129, 4, 74)        # what the header says it refuses
    assert "n_hidden" in lstm.train_shape_error(4, 0, 4, 74)
    assert "n_out" in lstm.train_shape_error(4, 100, 9, 74)
    assert "n_out" in lstm.train_shape_error(4, 100, 0, 74)
    assert "n_in" in lstm.train_shape_error(65, 100, 4, 74)
    assert "n_in" in lstm.train_shape_error(0, 100, 4, 74)
    assert "T" in lstm.train_shape_error(4, 100, 4, 4097)
    assert "T" in lstm.train_shape_error(4, 100, 4, 0)


def test_the_three_entry_points_are_declared_bound_and_built():
    src = open(os.path.join(ROOT, "include", "esn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, n_args in (("esn_lstm_workspace_bytes", 6), ("esn_lstm_train", 37), ("esn_lstm_predict", 24)):
        decl = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args, name
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
    assert "esn_lstm.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "esn_lstm.hip"))
    assert _lib.ABI_VERSION == 10
    lib = _lib.load()
    assert lib.esn_abi_version() == 10
    for name in ("esn_lstm_workspace_bytes", "esn_lstm_train", "esn_lstm_predict"):
        assert hasattr(lib, name)
    # training: per group the three packed layers three times, the scaled input, gates and dz, c, tanh c and h, dys
    n_in, H, n_out, T = 16, 100, 8, 138
    per_group = 3 * (4 * H * (n_in + 1) + 4 * H * (H + 1) + n_out * (H + 1)) + T * n_in + 8 * H * T + (3 * T + 2) * H + T * n_out
    assert lib.esn_lstm_workspace_bytes(n_in, H, n_out, 3, 0, T) == 8 * 3 * per_group
    # prediction: per workgroup (at most 1024) the streamed k-steps; at H = 100 those of [W_ih | b] alone
    assert lib.esn_lstm_workspace_bytes(n_in, H, n_out, 0, 5, T) == 5 * 2048 * 7 * 5
    assert lib.esn_lstm_workspace_bytes(n_in, H, n_out, 0, 5000, T) == 1024 * 2048 * 7 * 5
    assert lib.esn_lstm_workspace_bytes(4, 128, 4, 0, 2, T) == 2 * 2048 * 8 * (2 + (32 - 16 - 8))
    for bad in ((n_in, 129, n_out, 3, 0, T), (65, H, n_out, 3, 0, T), (n_in, H, 9, 3, 0, T), (n_in, H, n_out, 3, 0, 4097)):
        assert lib.esn_lstm_workspace_bytes(*bad) == 0


def test_refusals_need_no_device():
    """Unserved shapes, precisions and a short workspace are refused before any HIP call."""
    import ctypes as C
    lib = _lib.load()
    buf = (C.c_double * 16)()
    a = C.cast(buf, C.c_void_p).value

    def train(precision, n_hidden=100, work_bytes=1 << 30, T=74, n_in=4, n_out=4, transient=0, epochs=3):
        rc = lib.esn_lstm_train(precision, n_in, n_hidden, n_out, 1, *[a] * 6, None, None, None, None, a, a, 1, T, T,
                                transient, 0, epochs, 0.01, 0.9, 0.999, 1e-8, *[a] * 6, None, a, work_bytes, None)
        return rc, lib.esn_last_error().decode()

    rc, msg = train(_lib.F64, n_hidden=129)
    assert rc == -1 and "n_hidden" in msg and "128" in msg, (rc, msg)
    rc, msg = train(_lib.F64, T=5000)
    assert rc == -1 and "4096" in msg, (rc, msg)
    rc, msg = train(_lib.F64, n_in=65)
    assert rc == -1 and "n_in" in msg, (rc, msg)
    rc, msg = train(_lib.F64, n_out=9)
    assert rc == -1 and "n_out" in msg, (rc, msg)
    rc, msg = train(_lib.F64, transient=74)
    assert rc == -1 and "transient" in msg, (rc, msg)
    rc, msg = train(_lib.F64, epochs=0)
    assert rc == -1 and "epochs" in msg, (rc, msg)
    rc, msg = train(_lib.F64, work_bytes=8)
    assert rc == -1 and "workspace" in msg, (rc, msg)
    for precision in (_lib.F32, _lib.F16, _lib.BF16):
        rc, msg = train(precision)
        assert rc == -2 and msg, (precision, rc, msg)

    def predict(precision, n_hidden=100, work_bytes=1 << 30):
        rc = lib.esn_lstm_predict(precision, 4, n_hidden, 4, *[a] * 6, None, None, None, None, a, 1, 1, 74, 74, 0, a, a,
                                  work_bytes, None)
        return rc, lib.esn_last_error().decode()

    rc, msg = predict(_lib.F16)
    assert rc == -2 and msg
    rc, msg = predict(_lib.F64, n_hidden=0)
    assert rc == -1 and "n_hidden" in msg, (rc, msg)
    rc, msg = predict(_lib.F64, work_bytes=8)
    assert rc == -1 and "workspace" in msg, (rc, msg)


def test_c99_program_includes_the_header_and_links(tmp_path):
    prog = ('#include "esn_hip.h"\n#include <stdio.h>\n'
            "int main(void) {\n"
            "    size_t n = esn_lstm_workspace_bytes(4, 100, 4, 1, 0, 74);\n"
            "    size_t z = esn_lstm_workspace_bytes(4, 129, 4, 1, 0, 74);\n"
            "    int rc = esn_lstm_train(ESN_F64, 4, 129, 4, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 74, 74, 0, 0, 50,\n"
            "                            0.01, 0.9, 0.999, 1e-8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0);\n"
            "    int rp = esn_lstm_predict(ESN_F64, 4, 129, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 74, 74, 0, 0, 0, 0, 0);\n"
            '    printf("%d %zu %zu %d %d\\n", esn_abi_version(), n, z, rc, rp);\n'
            "    return 0;\n}\n")
    out = c_abi.compile_and_run(tmp_path, "t", prog).stdout.split()
    assert out[0] == "10" and int(out[1]) > 0 and out[2] == "0" and out[3] == "-1" and out[4] == "-1", out
