"""CPU-only checks around the windowed ELM (include/esn_hip.h: esn_elm_features / esn_elm_predict).

tests/elm_ref.py, the NumPy restatement of the definition, reproduces what the reference's own ELM code computed
(tests/golden/elm.npz, made by tests/golden/make_elm_golden.py): case A, the windowed pinv ELM of
system_model_2_all_comparision.py, and case B, the ridge / standardised variant of the Demo-2x2 script expressed through
in_scale / in_shift / t_scale / t_shift.  Features and predictions within 1e-12 of max; W_out within 1e-9 relative
(cond(E) of case A is 7.5e2, stored in the golden; pinv and lstsq agree to 1e-13 there).  The reference's slice of its own
ELM output (rows [0, N) of the un-cut output) decodes at chance, the aligned slice (rows [delay + cp, + N)) below it.
Both entry points are plain C, typed by the binding, and return every unserved shape and null pointer before a device is
touched; the ABI number stays; elm_point refuses its arguments before it touches its FrameSource."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import c_abi  # noqa: E402
import elm_ref  # noqa: E402
from oracle import esn_oracle as eo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "elm.npz"))
N, N_T, CP, D, WINDOW = 64, 2, 7, 3, 8


def test_golden_is_small_and_holds_arrays_only():
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "elm.npz")) < 200 * 1024
    assert all(G[k].dtype.kind in "fciu" for k in G.files)
    assert float(G["a_cond"]) <= 1e4


def test_restatement_reproduces_golden_a():
    W_in, b = G["a_W_in"], G["a_b"]
    us = elm_ref.scaled_inputs(G["a_ESN_input"], N + D + CP)
    np.testing.assert_array_equal(elm_ref.windows(us, WINDOW), G["a_inputs_window"])
    E = elm_ref.rows(G["a_ESN_input"], N + D + CP, W_in, b, WINDOW)
    hidden = np.tanh(G["a_inputs_window"] @ W_in.T + b)
    assert np.abs(E[WINDOW - 1:, :100] - hidden).max() <= 1e-12
    assert not E[:WINDOW - 1].any() and (E[WINDOW - 1:, 100] == 1.0).all()
    W_out = elm_ref.fit(E, G["a_ESN_output"], WINDOW - 1)
    assert np.abs(W_out - G["a_W_out"]).max() <= 1e-9 * np.abs(G["a_W_out"]).max()
    Y = elm_ref.predict(G["a_inputs"], 3, N + D + CP, 0, W_in[None], b[None], G["a_W_out"][None], WINDOW)
    assert np.abs(Y - G["a_x_hat_temp"]).max() <= 1e-12 * np.abs(G["a_x_hat_temp"]).max()
    assert not Y[:, :WINDOW - 1].any()


def _b_args():
    sx, sy = G["b_X_sigma"], G["b_Y_sigma"]
    return dict(in_scale=(1.0 / sx)[None], in_shift=(-G["b_X_mu"] / sx)[None], t_scale=(1.0 / sy)[None],
                t_shift=(-G["b_Y_mu"] / sy)[None])


def test_restatement_reproduces_golden_b_through_the_four_scalings():
    kw, forget = _b_args(), int(G["b_forget"])
    W_in, b = G["b_W"].T.copy(), G["b_b"]
    E = elm_ref.rows(G["a_ESN_input"], N + D + CP, W_in, b, 1, bias_col=False, in_scale=kw["in_scale"][0],
                     in_shift=kw["in_shift"][0])
    W_out = elm_ref.fit(E, G["a_ESN_output"], forget, kw["t_scale"][0], kw["t_shift"][0], ridge=float(G["b_alpha"]))
    assert np.abs(W_out - G["b_W_out"].T).max() <= 1e-9 * np.abs(G["b_W_out"]).max()
    Y = elm_ref.predict(G["a_inputs"], 3, N + D + CP, forget, W_in[None], b[None], G["b_W_out"].T[None], 1,
                        bias_col=False, **kw)
    assert np.abs(Y - G["b_Y_pred"]).max() <= 1e-12 * np.abs(G["b_Y_pred"]).max()


def slice_ber(x_hat_temp, bits, first_row, p_i, m=4):
    """BER of rows [first_row, + N) of un-cut outputs [F, T, 2 n_t] through the oracle's tail."""
    const, err, n = eo.unit_qam(m), 0, 0
    for y, tx in zip(x_hat_temp, bits):
        x = eo.outputs_to_time_signals(y[first_row:first_row + N], np.full(2 * N_T, D), D, N, N_T)
        err += eo.count_bit_errors(tx, eo.hard_bits(eo.time_to_freq(x, N, p_i), const, m))
        n += tx.size
    return err / n


def test_reference_slice_decodes_at_chance_and_the_aligned_slice_below_it():
    data, bits = G["a_x_hat_temp"][1:], G["bits"][1:]
    ref = slice_ber(data, bits, 0, float(G["p_i"]))
    aligned = slice_ber(data, bits, D + CP, float(G["p_i"]))
    assert 0.45 <= ref <= 0.55, ref
    assert aligned < ref, (aligned, ref)


def test_binding_types_both_entry_points_and_the_abi_number_stays():
    import ctypes as C
    from esn_ofdm_mimo_amd import _lib
    assert _lib.ABI_VERSION == 10
    lib = _lib.load()
    assert lib.esn_abi_version() == 10
    for name, n_args in (("esn_elm_features", 19), ("esn_elm_predict", 24)):
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args
        assert getattr(lib, name).argtypes == args
    assert _lib.SIGNATURES["esn_elm_features"][1][14] is C.c_uint64
    assert _lib.SIGNATURES["esn_elm_predict"][1][21] is C.c_uint64


# esn_elm_predict: (precision, n_in, n_hidden, window, bias_col, n_wsets, n_out, e_cols, n_frames, frames_per_group, T_in,
# T, transient), the code and the word the message must hold; GOOD is served as far as the checks go
GOOD = (0, 16, 512, 8, 1, 1, 8, 513, 40, 20, 135, 138, 10)
BAD = [
    ((1,) + GOOD[1:], -2, "precision"), ((3,) + GOOD[1:], -2, "precision"), ((7,) + GOOD[1:], -1, "precision"),
    ((0, 0) + GOOD[2:], -1, "n_in"), ((0, 16, 512, 0) + GOOD[4:], -1, "window"), ((0, 16, 512, 17) + GOOD[4:], -1, "window"),
    ((0, 33, 512, 8) + GOOD[4:], -1, "K = 256"), ((0, 257, 512, 1) + GOOD[4:], -1, "K = 256"),
    ((0, 16, 0) + GOOD[3:], -1, "n_hidden"), ((0, 16, 1025, 8, 1, 1, 8, 1026) + GOOD[8:], -1, "n_hidden"),
    ((0, 16, 512, 8, 2) + GOOD[5:], -1, "bias_col"), ((0, 16, 512, 8, 1, 0) + GOOD[6:], -1, "n_wsets"),
    ((0, 16, 512, 8, 1, 1, 0) + GOOD[7:], -1, "n_out"), ((0, 16, 512, 8, 1, 1, 9) + GOOD[7:], -1, "n_out"),
    (GOOD[:7] + (512,) + GOOD[8:], -1, "e_cols"), (GOOD[:7] + (517,) + GOOD[8:], -1, "e_cols"),
    (GOOD[:8] + (0,) + GOOD[9:], -1, "invalid sizes"), (GOOD[:9] + (0,) + GOOD[10:], -1, "invalid sizes"),
    (GOOD[:10] + (0, 138, 10), -1, "T_in"), (GOOD[:10] + (139, 138, 10), -1, "T_in"),
    (GOOD[:10] + (135, (1 << 20) + 1, 10), -1, "T_in"), (GOOD[:10] + (5, 7, 0), -1, "exceeds T"),
    (GOOD[:10] + (135, 138, -1), -1, "transient"), (GOOD[:10] + (135, 138, 138), -1, "transient"),
    (GOOD[:8] + (40000, 20, 1 << 20, 1 << 20, 10), -1, "tiles"),
]
# esn_elm_features: (precision, n_in, n_hidden, window, bias_col, n_wsets, n_groups, T_in, T, e_f32, e_cols)
F_GOOD = (0, 16, 512, 8, 1, 1, 5, 135, 138, 0, 516)
F_BAD = [
    ((2,) + F_GOOD[1:], -2, "ESN_F64"), ((1,) + F_GOOD[1:], -2, "precision"), ((0, 32, 512, 9) + F_GOOD[4:], -1, "K = 256"),
    (F_GOOD[:6] + (0,) + F_GOOD[7:], -1, "invalid sizes"), (F_GOOD[:10] + (518,), -1, "e_cols"),
    (F_GOOD[:7] + (139, 138) + F_GOOD[9:], -1, "T_in"), ((0, 16, 2000) + F_GOOD[3:], -1, "n_hidden"),
]


def _predict(lib, row, W_in=64, b=64, W_out=64, U=64, Y=64):
    prec, n_in, nh, w, bias, ns, n_out, e_cols, n_f, fpg, t_in, T, tr = row
    return lib.esn_elm_predict(prec, n_in, nh, w, bias, ns, n_out, W_in or None, b or None, W_out or None, e_cols, None,
                               None, None, None, U or None, n_f, fpg, t_in, T, tr, 0, Y or None, None)


def _features(lib, row, W_in=64, b=64, U=64, E=64):
    prec, n_in, nh, w, bias, ns, n_g, t_in, T, e32, e_cols = row
    return lib.esn_elm_features(prec, n_in, nh, w, bias, ns, W_in or None, b or None, None, None, U or None, n_g, t_in,
                                T, 0, E or None, e32, e_cols, None)


def test_every_unserved_shape_and_null_pointer_is_refused_from_ctypes_without_a_device():
    from esn_ofdm_mimo_amd import _lib
    lib = _lib.load()
    for row, code, word in BAD:
        assert _predict(lib, row) == code, row
        msg = lib.esn_last_error().decode()
        assert "esn_elm_predict" in msg and word in msg, (row, msg)
    for row, code, word in F_BAD:
        assert _features(lib, row) == code, row
        msg = lib.esn_last_error().decode()
        assert "esn_elm_features" in msg and word in msg, (row, msg)
    for kw in (dict(W_in=0), dict(b=0), dict(W_out=0), dict(U=0), dict(Y=0)):
        assert _predict(lib, GOOD, **kw) == -1 and "null" in lib.esn_last_error().decode(), kw
    for kw in (dict(W_in=0), dict(b=0), dict(U=0), dict(E=0)):
        assert _features(lib, F_GOOD, **kw) == -1 and "null" in lib.esn_last_error().decode(), kw
    assert _predict(lib, GOOD, Y=72) == -1 and "aligned" in lib.esn_last_error().decode()
    assert _features(lib, F_GOOD, E=72) == -1 and "aligned" in lib.esn_last_error().decode()


C_SRC = r'''
#include <stdio.h>
#include <string.h>
#include "esn_hip.h"
static int said(const char* who, const char* word) {
    return strstr(esn_last_error(), who) != 0 && strstr(esn_last_error(), word) != 0;
}
/* pointers are never dereferenced: the checks run first */
static int predict(int prec, int n_in, int nh, int w, int bias, int ns, int n_out, int e_cols, int n_f, int fpg, int t_in,
                   int T, int tr) {
    return esn_elm_predict(prec, n_in, nh, w, bias, ns, n_out, (const double*)64, (const double*)64, (const double*)64,
                           e_cols, 0, 0, 0, 0, (const double*)64, n_f, fpg, t_in, T, tr, 0, (double*)64, 0);
}
static int features(int prec, int n_in, int nh, int w, int bias, int ns, int n_g, int t_in, int T, int e32, int e_cols) {
    return esn_elm_features(prec, n_in, nh, w, bias, ns, (const double*)64, (const double*)64, 0, 0, (const double*)64,
                            n_g, t_in, T, 0, (void*)64, e32, e_cols, 0);
}
int main(void) {
    if (esn_abi_version() != 10) return 1;
%s
    printf("elm abi ok\n");
    return 0;
}
'''


def test_entry_points_link_from_c99_and_validate_without_a_device(tmp_path):
    rows = ['    if (predict(%s) != %d || !said("esn_elm_predict", "%s")) return %d;'
            % (", ".join(str(v) for v in row), code, word, 2 + i) for i, (row, code, word) in enumerate(BAD)]
    rows += ['    if (features(%s) != %d || !said("esn_elm_features", "%s")) return %d;'
             % (", ".join(str(v) for v in row), code, word, 100 + i) for i, (row, code, word) in enumerate(F_BAD)]
    r = c_abi.compile_and_run(tmp_path, "elm", C_SRC % "\n".join(rows))
    assert "elm abi ok" in r.stdout


def test_elm_point_refuses_its_arguments_before_the_device():
    from esn_ofdm_mimo_amd import montecarlo, points
    assert montecarlo.elm_point is points.elm_point

    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError("the FrameSource was touched: " + name)

    for kw, word in ((dict(slice="early"), "slice must be"), (dict(weights="fresh"), "weights must be"),
                     (dict(precision="bf16"), "precision must be"), (dict(method="pinv"), "method must be"),
                     (dict(window=0), "window"), (dict(window=17), "window"), (dict(window=2.5), "window"),
                     (dict(n_hidden=0), "n_hidden"), (dict(n_hidden=2048), "n_hidden"), (dict(gain=0.0), "gain"),
                     (dict(ridge=-1.0), "ridge"), (dict(n_blocks=0), "n_blocks"), (dict(first_block=-1), "first_block"),
                     (dict(chunk_blocks=0), "chunk_blocks"), (dict(frames_per_block=0), "frames_per_block")):
        args = dict(dict(ebno_db=12.0, snr_idx=0, n_blocks=2), **kw)
        with pytest.raises(ValueError, match=word):
            points.elm_point(NoDevice(), **args)
