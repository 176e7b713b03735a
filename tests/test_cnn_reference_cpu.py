"""The windowed CNN's definition (include/esn_hip.h, restated in tests/cnn_ref.py) against the reference's own numbers
(tests/golden/cnn.npz, written by tests/golden/make_cnn_golden.py from the reference's CNNModel and trainMIMOModel under
torch.manual_seed(77)), the served-shape rule and the C ABI of the three entry points.  No GPU.

The reference trains in float32; the restatement in float64 cannot meet it closer than float32 rounding carried through
50 Adam steps.  That figure is measured here, not committed: the bound is 4 x the largest difference between the
restatement run in float32 and in float64 on the same inputs, over the parameters and over the outputs.  The ratios are
printed."""
import functools
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import c_abi  # noqa: E402
import cnn_ref  # noqa: E402
from cnn_ref import NAMES  # noqa: E402
from esn_ofdm_mimo_amd import _lib, build, cnn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "cnn.npz"))
KERNEL = 5


def x_hat_temp(prm, dtype):
    """The output of the three golden frames in `dtype` arithmetic (:112-113)."""
    return cnn_ref.predict(GOLD["inputs"], 3, GOLD["inputs"].shape[1], 0, [prm[n][None] for n in NAMES], KERNEL,
                           dtype=dtype).astype(np.float64)


@functools.lru_cache(maxsize=None)
def float32_bound():
    """(restatement in float64, 4 x max |float32 - float64| over the parameters, the same over x_hat_temp)."""
    init = [GOLD[n + "_0"] for n in NAMES]
    r64 = cnn_ref.train(GOLD["ESN_input"], GOLD["ESN_output"], init, KERNEL)
    r32 = cnn_ref.train(GOLD["ESN_input"], GOLD["ESN_output"], init, KERNEL, dtype=np.float32)
    d_prm = max(np.abs(r32[n].astype(np.float64) - r64[n]).max() for n in NAMES)
    d_out = np.abs(x_hat_temp(r32, np.float32) - x_hat_temp(r64, np.float64)).max()
    return r64, 4.0 * d_prm, 4.0 * d_out


def test_float64_restatement_meets_the_reference_float32_training():
    r64, b_prm, b_out = float32_bound()
    assert r64["min_pre"] > 1e-9, r64["min_pre"]                  # no ReLU on its kink
    for n in NAMES:
        assert GOLD[n].dtype == np.float32 and r64[n].shape == GOLD[n].shape
        err = np.abs(r64[n] - GOLD[n]).max()
        print(n, "reference vs float64 restatement", err, "bound", b_prm, "ratio", err / b_prm)
        assert err <= b_prm
    err = np.abs(x_hat_temp(r64, np.float64) - GOLD["x_hat_temp"]).max()
    print("x_hat_temp", err, "bound", b_out, "ratio", err / b_out, "min |pre|", r64["min_pre"])
    assert err <= b_out
    assert r64["loss"][-1] < 0.5 * r64["loss"][0]                 # it did train
    assert int(GOLD["nForgetPoints"]) == 3 + 7                    # no window term (:91)


def test_init_weights_draws_what_the_reference_model_draws():
    import torch
    torch.manual_seed(int(GOLD["seed"]))
    got = cnn.init_weights(4, 4, (32, 64), 5)
    for n, t in zip(NAMES, got):
        assert t.dtype == np.float64
        np.testing.assert_array_equal(t, GOLD[n + "_0"].astype(np.float64))


def test_a_channel_that_is_never_active_keeps_its_parameters_bitwise():
    init = [GOLD[n + "_0"].astype(np.float64) for n in NAMES]
    dead = 17
    init[1][dead] = -100.0
    for dtype in (np.float64, np.float32):
        r = cnn_ref.train(GOLD["ESN_input"], GOLD["ESN_output"], init, KERNEL, dtype=dtype)
        want = [np.asarray(t, dtype=dtype) for t in init]
        np.testing.assert_array_equal(r["W1"][dead], want[0][dead])
        assert r["b1"][dead] == want[1][dead]
        np.testing.assert_array_equal(r["W2"][:, dead], want[2][:, dead])      # the next layer's weights that read it
        assert all(np.isfinite(r[n]).all() for n in NAMES)
        assert np.abs(r["W1"][dead - 1] - want[0][dead - 1]).max() > 1e-3       # its neighbour moved
        assert np.abs(r["W2"][:, dead - 1] - want[2][:, dead - 1]).max() > 1e-3


def test_the_restatement_is_torch_conv1d():
    """rows / wmat / fold against torch.nn.functional.conv1d and its autograd, float64, a shape with T below the
    receptive field and scalings that make a scaled zero row differ from zero padding."""
    import torch
    rs = np.random.RandomState(5)
    n_in, c1, c2, n_out, k, t_in, T = 3, 5, 4, 2, 3, 6, 7
    prm = cnn.init_weights(n_in, n_out, (c1, c2), k)
    U, D = rs.randn(t_in, n_in), rs.randn(T, n_out)
    sc, sh = rs.uniform(0.5, 2, n_in), rs.uniform(-0.2, 0.2, n_in)
    r = cnn_ref.train(U, D, prm, k, transient=2, in_scale=sc, in_shift=sh, epochs=1, lr=0.01)
    tp = [torch.tensor(t, requires_grad=True) for t in prm]
    x = torch.tensor(cnn_ref.scaled_inputs(U, T, sc, sh)).T[None]
    h = torch.relu(torch.nn.functional.conv1d(x, tp[0], tp[1], padding=1))
    h = torch.relu(torch.nn.functional.conv1d(h, tp[2], tp[3], padding=1))
    ys = torch.nn.functional.conv1d(h, tp[4], tp[5], padding=1)[0].T
    loss = ((ys - torch.tensor(D))[2:] ** 2).mean()
    assert abs(float(loss.detach()) - r["loss"][0]) <= 1e-14 * abs(float(loss.detach()))
    opt = torch.optim.Adam(tp, lr=0.01)
    loss.backward()
    opt.step()
    for n, t in zip(NAMES, tp):
        assert np.abs(t.detach().numpy() - r[n]).max() <= 1e-12, n


def test_the_served_shape_rule_holds_the_reference_shapes():
    for T in (74, 138, 522):
        assert cnn.train_shape_error(4, 32, 64, 4, 5, T) is None
        assert cnn.train_shape_error(16, 32, 64, 8, 5, T) is None
    assert cnn.train_shape_error(4, 7, 19, 3, 3, 23) is None                  # channels that are no multiple of 16
    assert cnn.train_shape_error(6, 64, 64, 2, 7, 13) is None
    assert cnn.train_shape_error(2, 3, 2, 1, 1, 1) is None
    assert cnn.train_shape_error(4, 32, 64, 4, 5, 1024) is None
    assert "kernel" in cnn.train_shape_error(4, 32, 64, 4, 4, 74)             # what the header says it refuses
    assert "kernel" in cnn.train_shape_error(4, 32, 64, 4, 9, 74)
    assert "channels" in cnn.train_shape_error(4, 129, 64, 4, 5, 74)
    assert "channels" in cnn.train_shape_error(4, 32, 0, 4, 5, 74)
    assert "n_out" in cnn.train_shape_error(4, 32, 64, 9, 5, 74)
    assert "n_in" in cnn.train_shape_error(65, 32, 64, 4, 5, 74)
    assert "T" in cnn.train_shape_error(4, 32, 64, 4, 5, 4097)


def test_the_three_entry_points_are_declared_bound_and_built():
    src = open(os.path.join(ROOT, "include", "esn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, n_args in (("esn_cnn_workspace_bytes", 8), ("esn_cnn_train", 39), ("esn_cnn_predict", 26)):
        decl = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args, name
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
    assert "esn_cnn.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "esn_cnn.hip"))
    assert _lib.ABI_VERSION == 10
    lib = _lib.load()
    assert lib.esn_abi_version() == 10
    for name in ("esn_cnn_workspace_bytes", "esn_cnn_train", "esn_cnn_predict"):
        assert hasattr(lib, name)
    # the workspace: per group the parameters with their bias column three times, the padded activations and gradients
    n = 32 * 81 + 64 * 161 + 8 * 321
    assert lib.esn_cnn_workspace_bytes(16, 32, 64, 8, 5, 3, 0, 138) == 8 * 3 * (3 * n + 142 * (16 + 32 + 64) + 142 * (32 + 64 + 8))
    assert lib.esn_cnn_workspace_bytes(16, 32, 64, 8, 5, 0, 2, 138) == 8 * 2 * (n + 142 * (16 + 32 + 64))
    assert lib.esn_cnn_workspace_bytes(16, 32, 64, 8, 4, 3, 0, 138) == 0


def test_refusals_need_no_device():
    """Unserved shapes, precisions and a short workspace are refused before any HIP call."""
    import ctypes as C
    lib = _lib.load()
    buf = (C.c_double * 16)()
    a = C.cast(buf, C.c_void_p).value

    def train(precision, kernel=5, work_bytes=1 << 30, T=74):
        rc = lib.esn_cnn_train(precision, 4, 32, 64, 4, kernel, 1, *[a] * 6, None, None, None, None, a, a, 1, T, T, 0, 0, 3,
                               0.01, 0.9, 0.999, 1e-8, *[a] * 6, None, a, work_bytes, None)
        return rc, lib.esn_last_error().decode()

    rc, msg = train(_lib.F64, kernel=4)
    assert rc == -1 and "kernel" in msg, (rc, msg)
    rc, msg = train(_lib.F64, T=5000)
    assert rc == -1 and "4096" in msg, (rc, msg)
    rc, msg = train(_lib.F64, work_bytes=8)
    assert rc == -1 and "workspace" in msg, (rc, msg)
    for precision in (_lib.F32, _lib.F16, _lib.BF16):
        rc, msg = train(precision)
        assert rc == -2 and msg, (precision, rc, msg)
    rc = lib.esn_cnn_predict(_lib.F16, 4, 32, 64, 4, 5, *[a] * 6, None, None, None, None, a, 1, 1, 74, 74, 0, a, a, 1 << 30,
                             None)
    assert rc == -2 and lib.esn_last_error()


def test_c99_program_includes_the_header_and_links(tmp_path):
    prog = ('#include "esn_hip.h"\n#include <stdio.h>\n'
            "int main(void) {\n"
            "    size_t n = esn_cnn_workspace_bytes(4, 32, 64, 4, 5, 1, 0, 74);\n"
            "    int rc = esn_cnn_train(ESN_F64, 4, 32, 64, 4, 4, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 74, 74, 0, 0, 50,\n"
            "                           0.01, 0.9, 0.999, 1e-8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0);\n"
            "    int rp = esn_cnn_predict(ESN_F64, 4, 32, 64, 4, 5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 74, 74, 0, 0, 0, 0, 0);\n"
            '    printf("%d %zu %d %d\\n", esn_abi_version(), n, rc, rp);\n'
            "    return 0;\n}\n")
    out = c_abi.compile_and_run(tmp_path, "t", prog).stdout.split()
    assert out[0] == "10" and int(out[1]) > 0 and out[2] == "-1" and out[3] == "-1", out
