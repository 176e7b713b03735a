"""The windowed ELM on the device (csrc/esn_elm.hip, esn_ofdm_mimo_amd/elm.py, points.elm_point) against the NumPy
restatement tests/elm_ref.py and the reference's own numbers (tests/golden/elm.npz).

Inputs have unit variance, |W_in| <= 1, b in (-1, 1); scalings differ per group.  Bounds:
  features, float64   1e-11 absolute: K <= 256 products of magnitude <= ~10 give 3e-13 of re-ordering, plus a few ulp of
                      tanh.  Rows < window - 1 and pad columns are exactly 0.0; a float32 E is the float64 E rounded.
  predict, float64    |Y - Y_ref| t_scale <= 1e-11 (1 + sum_c |W_out[o][c]|) per output: the feature bound carried through
                      the read-out product.  Rows in [transient, window - 1) are exactly zero; the fused result is within
                      the same bound of features -> matmul on the device; a frame alone is bitwise itself in the batch.
  fit                 W_out within 1e-7 relative of the reference's pinv / ridge solution (the project's pinv-parity
                      figure), predictions within 1e-9 of max, the 9-list of trainMIMOELM equal with NMSE to 1e-9.
  predict, fp16       against elm_ref(fp16_operands=True); the bound is 4 x the largest difference between that and the
                      float64 restatement on the same inputs, normalised by max |Y| -- computed here, not committed;
                      the factor covers float32 accumulation order and the device tanh.  The ratios are printed.
  elm_point           per-block error counts equal to the same loop in NumPy on the device's own frames, for a seed at
                      which no X_hat of the restatement lies within 1e-8 of a slicer boundary (asserted)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elm_ref  # noqa: E402
import remod_ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# n_in, window, n_hidden, bias_col, T_in, T, n_groups, n_wsets, group_offset, e_cols, n_out
SHAPES = [
    (2, 1, 33, 0, 21, 21, 1, 1, 0, 33, 1),
    (4, 8, 100, 1, 71, 74, 3, 1, 0, 101, 4),
    (4, 8, 100, 1, 71, 74, 3, 1, 0, 104, 4),
    (16, 8, 512, 1, 135, 138, 5, 3, 7, 516, 8),
    (4, 3, 17, 1, 19, 23, 2, 2, 1, 18, 3),
    (32, 1, 100, 1, 67, 67, 1, 1, 0, 101, 4),
    (16, 16, 1024, 0, 40, 40, 2, 1, 0, 1024, 2),
]
IDS = ["in%d-w%d-h%d-b%d-T%d_%d-G%d-S%d-off%d-e%d-o%d" % s for s in SHAPES]
F16_SHAPES = [SHAPES[1], SHAPES[3], SHAPES[4], SHAPES[6]]     # rows 2 and 3 of the table; an odd n_out; W_in beyond LDS
DELAY_CP = 10


@functools.lru_cache(maxsize=None)
def make_case(shape, fpg=1):
    """Host arrays of one shape: weights, per-group scalings, one training sequence per group with the restatement's
    features and its own pinv fit, and B = n_groups fpg - (fpg > 1) frames (a ragged last group)."""
    n_in, w, nh, bias, t_in, T, G, S, off, e_cols, n_out = shape
    rs = np.random.RandomState(1000 * nh + 10 * n_in + w)
    c = dict(W_in=rs.uniform(-1, 1, (S, nh, w * n_in)), b=rs.uniform(-1, 1, (S, nh)),
             in_scale=rs.uniform(0.5, 2.0, (G, n_in)), in_shift=rs.uniform(-0.2, 0.2, (G, n_in)),
             t_scale=rs.uniform(0.5, 2.0, (G, n_out)), t_shift=rs.uniform(-0.2, 0.2, (G, n_out)))
    c["U_fit"] = rs.randn(G, t_in, n_in) / c["in_scale"][:, None, :]          # unit variance after scaling
    c["D_fit"] = rs.randn(G, T, n_out)
    c["E"] = elm_ref.features(c["U_fit"], T, c["W_in"], c["b"], w, bias, e_cols, c["in_scale"], c["in_shift"], off)
    c["W_out"] = np.stack([elm_ref.fit(c["E"][g], c["D_fit"][g], w - 1, c["t_scale"][g], c["t_shift"][g])
                           for g in range(G)])
    B = G * fpg - (1 if fpg > 1 else 0)
    c["U"] = rs.randn(B, t_in, n_in) / c["in_scale"][np.arange(B) // fpg][:, None, :]
    return c


def make_bank(shape, c):
    from esn_ofdm_mimo_amd.elm import ElmBank
    n_in, w, nh, bias, _, _, G, _, _, _, n_out = shape
    bank = ElmBank(n_in, n_out, nh, w, c["W_in"], c["b"], bias_col=bool(bias), n_groups=G)
    bank.set_scaling(c["in_scale"], c["in_shift"], c["t_scale"], c["t_shift"])
    return bank


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_features_f64_match_the_restatement(shape):
    n_in, w, nh, bias, t_in, T, G, S, off, e_cols, n_out = shape
    c = make_case(shape)
    bank = make_bank(shape, c)
    E = bank.features(c["U_fit"], T=T, e_cols=e_cols, group_offset=off)
    E32 = bank.features(c["U_fit"], T=T, e_cols=e_cols, e_dtype="f32", group_offset=off)
    got = E.cpu().numpy()
    err = np.abs(got - c["E"]).max()
    print("features", IDS[SHAPES.index(shape)], "max abs err", err)
    assert got.shape == (G, T, e_cols) and np.isfinite(got).all()
    assert err <= 1e-11
    assert not got[:, :w - 1].any() and not got[:, :, nh + bias:].any()
    if bias:
        assert (got[:, w - 1:, nh] == 1.0).all()
    if T > t_in:      # rows from T_in on see in_shift alone: the same bytes as zero rows given explicitly
        padded = np.concatenate([c["U_fit"], np.zeros((G, T - t_in, n_in))], axis=1)
        np.testing.assert_array_equal(bank.features(padded, e_cols=e_cols, group_offset=off).cpu().numpy(), got)
    np.testing.assert_array_equal(E32.cpu().numpy(), got.astype(np.float32))


@pytest.mark.parametrize("fpg", [1, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_predict_f64_matches_the_restatement(shape, fpg):
    import torch
    n_in, w, nh, bias, t_in, T, G, S, off, e_cols, n_out = shape
    c = make_case(shape, fpg)
    bank = make_bank(shape, c)
    bank.set_readout(c["W_out"])
    B = c["U"].shape[0]
    grp = np.arange(B) // fpg
    bound = 1e-11 * (1.0 + np.abs(c["W_out"]).sum(axis=2))                   # [G, n_out]
    for transient in [t for t in (0, w - 1) if t != DELAY_CP] + [DELAY_CP]:
        ref = elm_ref.predict(c["U"], fpg, T, transient, c["W_in"], c["b"], c["W_out"], w, bias, c["in_scale"],
                              c["in_shift"], c["t_scale"], c["t_shift"], off)
        Y = bank.predict(c["U"], fpg, T=T, transient=transient, group_offset=off)
        got = Y.cpu().numpy()
        assert got.shape == ref.shape and np.isfinite(got).all()
        excess = (np.abs(got - ref) * c["t_scale"][grp][:, None, :] / bound[grp][:, None, :]).max()
        print("predict", IDS[SHAPES.index(shape)], "fpg", fpg, "transient", transient, "err / bound", excess)
        assert excess <= 1.0
        if transient < w - 1:
            assert not got[:, :w - 1 - transient].any()
    # one frame alone is bitwise itself inside the batch (transient DELAY_CP, the last of the loop)
    k = B - 1
    g = int(grp[k])
    alone = make_bank(shape, dict(c, in_scale=c["in_scale"][g:g + 1], in_shift=c["in_shift"][g:g + 1],
                                  t_scale=c["t_scale"][g:g + 1], t_shift=c["t_shift"][g:g + 1]))
    alone.set_readout(c["W_out"][g:g + 1])
    one = alone.predict(c["U"][k:k + 1], fpg, T=T, transient=DELAY_CP, group_offset=off + g)
    assert torch.equal(one[0], Y[k])
    if S > 1:         # the weight set follows (group_offset + g) % n_wsets
        other = bank.predict(c["U"], fpg, T=T, transient=DELAY_CP, group_offset=off + 1).cpu().numpy()
        ref1 = elm_ref.predict(c["U"], fpg, T, DELAY_CP, c["W_in"], c["b"], c["W_out"], w, bias, c["in_scale"],
                               c["in_shift"], c["t_scale"], c["t_shift"], off + 1)
        assert (np.abs(other - ref1) * c["t_scale"][grp][:, None, :] / bound[grp][:, None, :]).max() <= 1.0
        assert np.abs(other - got).max() > 1e-3
    if fpg == 1:      # fused against features -> matmul on the device
        E = bank.features(c["U"], T=T, e_cols=e_cols, group_offset=off)
        ys = torch.einsum("gtc,goc->gto", E, bank.W_out)
        two = ((ys - bank.t_shift[:, None, :]) / bank.t_scale[:, None, :])[:, max(DELAY_CP, w - 1):].cpu().numpy()
        fused = got[:, max(DELAY_CP, w - 1) - DELAY_CP:]
        assert (np.abs(fused - two) * c["t_scale"][:, None, :] / bound[:, None, :]).max() <= 1.0


GOLD = np.load(os.path.join(ROOT, "tests", "golden", "elm.npz"))


@pytest.mark.parametrize("method", ["qr", "chol"])
def test_bank_fit_reproduces_golden_a(method):
    from esn_ofdm_mimo_amd.elm import ElmBank
    bank = ElmBank(4, 4, 100, 8, GOLD["a_W_in"], GOLD["a_b"])
    E = bank.fit(GOLD["a_ESN_input"][None], GOLD["a_ESN_output"][None], method=method)
    W_out = bank.W_out.cpu().numpy()[0]
    assert E.shape[2] == 102 and W_out.shape == (4, 102)                    # 67 rows < 101 columns: padded to 16 bytes
    assert int(bank.fit_status.abs().sum()) == 0
    rel = np.abs(W_out[:, :101] - GOLD["a_W_out"]).max() / np.abs(GOLD["a_W_out"]).max()
    print("golden A", method, "W_out rel err", rel, "pad", np.abs(W_out[:, 101:]).max())
    assert rel <= 1e-7
    assert np.abs(W_out[:, 101:]).max() <= 1e-14 * np.abs(W_out).max()
    Y = bank.predict(GOLD["a_inputs"], 3).cpu().numpy()
    assert np.abs(Y - GOLD["a_x_hat_temp"]).max() <= 1e-9 * np.abs(GOLD["a_x_hat_temp"]).max()
    # an unpadded read-out gives the same predictions
    bank.set_readout(W_out[None, :, :101].copy())
    assert np.abs(bank.predict(GOLD["a_inputs"], 3).cpu().numpy() - Y).max() <= 1e-12 * np.abs(Y).max()


def test_elm_class_and_train_mimo_elm_reproduce_golden_a():
    from esn_ofdm_mimo_amd.elm import ELM, trainMIMOELM
    np.random.seed(77)                                                       # the generator's seed: same draws
    res = trainMIMOELM(GOLD["y_cp"][0], GOLD["x_cp"][0], 64, 2, 7, 8)
    ESN_input, ESN_output, model, Delay, idx, dmin, dmax, n_forget, nmse = res
    np.testing.assert_array_equal(ESN_input, GOLD["a_ESN_input"])
    np.testing.assert_array_equal(ESN_output, GOLD["a_ESN_output"])
    np.testing.assert_array_equal(model.W_in, GOLD["a_W_in"])
    np.testing.assert_array_equal(model.b, GOLD["a_b"])
    assert (Delay, idx, dmin, dmax, n_forget) == ([3] * 4, 3, 3, 3, int(GOLD["a_nForgetPoints"]))
    print("trainMIMOELM NMSE", nmse, "golden", float(GOLD["a_NMSE"]))
    assert abs(nmse - float(GOLD["a_NMSE"])) <= 1e-9 * float(GOLD["a_NMSE"])
    assert np.abs(model.W_out - GOLD["a_W_out"]).max() <= 1e-7 * np.abs(GOLD["a_W_out"]).max()
    elm = ELM(32, random_state=5)
    elm.W_in, elm.b = GOLD["a_W_in"], GOLD["a_b"]
    elm.fit(GOLD["a_inputs_window"], GOLD["a_targets_window"])
    assert np.abs(elm.W_out - GOLD["a_W_out"]).max() <= 1e-7 * np.abs(GOLD["a_W_out"]).max()
    want = GOLD["a_x_hat_temp"][1, 7:]
    from esn_ofdm_mimo_amd.elm import window_rows
    assert np.abs(elm.predict(window_rows(GOLD["a_inputs"][1], 8)) - want).max() <= 1e-9 * np.abs(want).max()


def test_bank_fit_reproduces_golden_b_through_ridge_and_the_four_scalings():
    from esn_ofdm_mimo_amd.elm import ElmBank
    sx, sy, forget = GOLD["b_X_sigma"], GOLD["b_Y_sigma"], int(GOLD["b_forget"])
    bank = ElmBank(4, 4, 200, 1, GOLD["b_W"].T.copy(), GOLD["b_b"], bias_col=False)
    bank.set_scaling((1.0 / sx)[None], (-GOLD["b_X_mu"] / sx)[None], (1.0 / sy)[None], (-GOLD["b_Y_mu"] / sy)[None])
    for method in ("qr", "chol"):
        bank.fit(GOLD["a_ESN_input"][None], GOLD["a_ESN_output"][None], transient=forget, method=method,
                 ridge=float(GOLD["b_alpha"]))
        W_out = bank.W_out.cpu().numpy()[0]
        rel = np.abs(W_out - GOLD["b_W_out"].T).max() / np.abs(GOLD["b_W_out"]).max()
        print("golden B", method, "W_out rel err", rel)
        assert rel <= 1e-7
        Y = bank.predict(GOLD["a_inputs"], 3, transient=forget).cpu().numpy()
        assert np.abs(Y - GOLD["b_Y_pred"]).max() <= 1e-9 * np.abs(GOLD["b_Y_pred"]).max()


def test_padded_columns_take_zero_weight_and_leave_the_predictions():
    from esn_ofdm_mimo_amd.elm import ElmBank
    bank = ElmBank(4, 4, 100, 8, GOLD["a_W_in"], GOLD["a_b"])
    U, D = GOLD["a_ESN_input"][None], GOLD["a_ESN_output"][None]
    outs = []
    for e_cols in (101, 104):
        W_out, status = bank.solve(bank.features(U, e_cols=e_cols), D, 7, method="qr")
        assert int(status.abs().sum()) == 0
        bank.set_readout(W_out)
        outs.append((W_out.cpu().numpy()[0], bank.predict(GOLD["a_inputs"], 3).cpu().numpy()))
    (w0, y0), (w1, y1) = outs
    assert np.abs(w1[:, 101:]).max() <= 1e-14 * np.abs(w1).max()
    assert np.abs(w1[:, :101] - w0).max() <= 1e-7 * np.abs(w0).max()
    assert np.abs(y1 - y0).max() <= 1e-9 * np.abs(y0).max()


@pytest.mark.parametrize("shape", F16_SHAPES, ids=[IDS[SHAPES.index(s)] for s in F16_SHAPES])
def test_predict_f16_is_within_four_times_the_fp16_operand_error(shape):
    n_in, w, nh, bias, t_in, T, G, S, off, e_cols, n_out = shape
    fpg = 5
    c = make_case(shape, fpg)
    bank = make_bank(shape, c)
    bank.set_readout(c["W_out"])
    args = (c["U"], fpg, T, w - 1, c["W_in"], c["b"], c["W_out"], w, bias, c["in_scale"], c["in_shift"], c["t_scale"],
            c["t_shift"], off)
    ref64 = elm_ref.predict(*args)
    ref16 = elm_ref.predict(*args, fp16_operands=True)
    bound = 4.0 * np.abs(ref16 - ref64).max() / np.abs(ref64).max()
    got = bank.predict(c["U"], fpg, T=T, transient=w - 1, precision="f16", group_offset=off).cpu().numpy()
    assert got.shape == ref16.shape and np.isfinite(got).all()
    err = np.abs(got - ref16).max() / np.abs(ref64).max()
    print("f16", IDS[SHAPES.index(shape)], "err", err, "bound", bound, "ratio err / (bound / 4)", 4.0 * err / bound)
    assert err <= bound
    zero = bank.predict(c["U"], fpg, T=T, transient=0, precision="f16", group_offset=off).cpu().numpy()
    assert not zero[:, :w - 1].any()
    np.testing.assert_array_equal(zero[:, w - 1:], got)


def numpy_elm_point(src, ebno, si, n_blocks, F, n_hidden, window, gain, seed, rows, first_block=0):
    """The loop of elm_point in NumPy on the device's own frames: per-block errors, bits and the smallest distance of
    an X_hat coordinate from a slicer boundary."""
    from esn_ofdm_mimo_amd.points import elm_weights
    from esn_ofdm_mimo_amd.frames import _view_real
    p = src.p
    d, T, n_in = p.delay, p.t_frame + p.delay, 2 * p.n_r
    data = src.blocks_fast(ebno, si, first_block, n_blocks, F)
    py, px = _view_real(data["pilot_y"]).cpu().numpy(), _view_real(data["pilot_x"]).cpu().numpy()
    dy, bits = _view_real(data["data_y"]).cpu().numpy(), data["data_bits"].cpu().numpy()
    W_in, b = elm_weights(n_hidden, window * n_in, gain, seed)
    scale = 1.0 / np.sqrt(p.var_x(ebno))
    transient = max(p.forget, window - 1)
    side, norm = remod_ref.slicer_constants(p.m)
    errs, margin = [], np.inf
    for g in range(n_blocks):
        U = np.zeros((T, n_in))
        D = np.zeros((T, 2 * p.n_t))
        U[:p.t_frame], D[d:] = py[g], px[g]
        E = elm_ref.rows(U, T, W_in, b, window, True, in_scale=scale)
        W_out = elm_ref.fit(E, D, transient, t_scale=scale)
        Y = elm_ref.predict(dy[g * F:(g + 1) * F], F, T, 0, W_in[None], b[None], W_out[None], window, True,
                            in_scale=np.full((1, n_in), scale), t_scale=np.full((1, 2 * p.n_t), scale))
        r = remod_ref.detect_remod(Y[:, rows:rows + p.n_sub], F, p.n_sub, p.cp, d, p.n_t, p.m, [p.p_i(ebno)],
                                   tx_bits=bits[g * F:(g + 1) * F])
        errs.append(int(r["err"][0]))
        xy = np.stack([r["X_hat"].real, r["X_hat"].imag]) * norm             # boundaries at the even integers
        inner = np.abs(xy) < side - 2 + 1.0
        margin = min(margin, np.abs(xy - 2.0 * np.rint(xy / 2.0))[inner].min() / norm if inner.any() else np.inf)
    return np.array(errs), F * p.n_sub * p.m * p.n_t, margin


POINT_CASES = [("2x2-N64-qpsk", dict(n_t=2, n_r=2, n_sub=64, m=2, channel="exp"), 100, 15.0),
               ("4x8-N128-16qam", dict(), 512, 21.0)]


@pytest.mark.parametrize("name,link,n_hidden,ebno", POINT_CASES, ids=[c[0] for c in POINT_CASES])
def test_elm_point_counts_what_the_numpy_loop_counts(name, link, n_hidden, ebno):
    from esn_ofdm_mimo_amd import montecarlo as mc
    p = mc.LinkParams(**link)
    src = mc.FrameSource(p, seed=11)
    G, F, kw = 6, 4, dict(n_hidden=n_hidden, window=8, gain=0.05, seed=3, frames_per_block=4)
    ber = {}
    for sl, rows in (("aligned", p.forget), ("reference", 0)):
        want, nb, margin = numpy_elm_point(src, ebno, 2, G, F, n_hidden, 8, 0.05, 3, rows)
        assert margin > 1e-8, margin                  # precondition on the NumPy side: nothing sits on a boundary
        err, bits = mc.elm_point(src, ebno, 2, G, slice=sl, **kw)
        print("elm_point", name, sl, "errors", err.cpu().numpy(), "numpy", want, "margin", margin)
        np.testing.assert_array_equal(err.cpu().numpy(), want)
        assert (bits.cpu().numpy() == nb).all()
        ber[sl] = want.sum() / (G * nb)
    assert 0.45 <= ber["reference"] <= 0.55 and ber["aligned"] < ber["reference"], ber


def test_elm_point_is_the_same_in_one_call_and_in_two():
    import torch
    from esn_ofdm_mimo_amd import montecarlo as mc
    src = mc.FrameSource(mc.LinkParams(n_t=2, n_r=2, n_sub=64, m=2, channel="exp"), seed=11)
    kw = dict(n_hidden=100, window=8, seed=3, frames_per_block=4)
    for weights in ("shared", "per_block"):
        e8, b8 = mc.elm_point(src, 15.0, 1, 8, weights=weights, **kw)
        e3, b3 = mc.elm_point(src, 15.0, 1, 3, weights=weights, chunk_blocks=2, **kw)
        e5, b5 = mc.elm_point(src, 15.0, 1, 5, weights=weights, first_block=3, **kw)
        assert torch.equal(e8, torch.cat([e3, e5])) and torch.equal(b8, torch.cat([b3, b5]))
        assert int(b8.sum()) == 8 * 4 * 64 * 2 * 2 and int(e8.sum()) < int(b8.sum()) // 2
