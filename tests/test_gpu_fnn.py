"""The windowed FNN on the device (csrc/esn_fnn.hip, the ReLU instantiations of csrc/esn_elm.hip, esn_ofdm_mimo_amd/fnn.py,
points.fnn_point) against the NumPy restatement tests/fnn_ref.py and the reference's own numbers (tests/golden/fnn.npz).

Inputs have unit variance after scaling, the initial parameters are U(+-1 / sqrt(fan_in)); scalings differ per group.
  training            every parameter within max(16 epochs lr (|R| + K + n_hidden) 2^-53, 64 s) of the float64
                      restatement: the first term is the rounding of one gradient sum carried through `epochs` steps of
                      size at most lr; s is the largest difference between the float64 restatement and itself in
                      longdouble (first group; not at the 4x8 shape, where it would take 10 s of host time and the
                      first term decides anyway) and with the rows in reversed order (every group), computed here.
                      loss[g][e] within the same figure, relative.  Precondition, asserted: the smallest |pre-activation|
                      the restatement met exceeds 1e-9 (no ReLU on its kink).  A group alone and any chunking of the
                      groups are bitwise the batch; a unit that is never active is bitwise untouched.
  predict, float64    |Y - Y_ref| t_scale <= 1e-11 (1 + sum |[W2 | b2][o]|) per output, the ELM test's bound; rows in
                      [transient, window - 1) exactly zero; a frame alone bitwise itself in the batch; the fused result
                      within the same bound of hidden rows -> matmul done with torch on the device.
  predict, fp16       against fnn_ref.predict(fp16_operands=True); bound 4 x the largest difference between that and the
                      float64 restatement, normalised by max |Y|, computed here.
  golden              FnnBank, FNN and trainMIMOFNN meet the reference's float32 training at the float32 bound of
                      tests/test_fnn_reference_cpu.py; the NMSE at that bound carried through its formula.
  fnn_point           per-block error counts equal to the same loop in NumPy on the device's own frames, for a seed at
                      which no X_hat of the restatement lies within 1e-8 of a slicer boundary (asserted).
The ratios are printed."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fnn_ref  # noqa: E402
import remod_ref  # noqa: E402
from test_fnn_reference_cpu import GOLD, NAMES, float32_bound, x_hat_temp  # noqa: E402
from esn_ofdm_mimo_amd import fnn as fnn_mod  # noqa: E402

pytestmark = pytest.mark.gpu

# n_in, window, n_hidden, n_out, T_in, T, n_groups, n_isets, group_offset, transient, epochs
SHAPES = [
    (2, 1, 5, 1, 21, 21, 1, 1, 0, 0, 3),
    (4, 8, 100, 4, 71, 74, 3, 1, 0, 7, 50),          # the reference's shape: K = 32, 100 is no multiple of 16
    (16, 8, 100, 8, 135, 138, 5, 3, 7, 10, 50),      # the 4x8 shape: K = 128, transient above window - 1
    (4, 3, 17, 3, 19, 23, 2, 2, 1, 2, 10),           # everything odd
    (16, 16, 64, 2, 40, 40, 1, 1, 0, 15, 5),         # the largest served n_hidden K = 16384
]
IDS = ["in%d-w%d-h%d-o%d-T%d_%d-G%d-S%d-off%d-tr%d-ep%d" % s for s in SHAPES]
F16_SHAPES = SHAPES[1:]
LR = 0.01
LONGDOUBLE_MACS = 500000      # NumPy's longdouble products run at ~1e7 multiply-adds a second: above this size of one
                              # product s comes from the reversed order alone, which can only make the bound smaller


@functools.lru_cache(maxsize=None)
def make_case(shape):
    """Host arrays of one shape, the float64 restatement of every group's training and the sensitivity s."""
    n_in, w, nh, n_out, t_in, T, G, S, off, transient, epochs = shape
    k = w * n_in
    rs = np.random.RandomState(1000 * nh + 10 * n_in + w)
    a1, a2 = 1.0 / np.sqrt(k), 1.0 / np.sqrt(nh)
    c = dict(init=(rs.uniform(-a1, a1, (S, nh, k)), rs.uniform(-a1, a1, (S, nh)), rs.uniform(-a2, a2, (S, n_out, nh)),
                   rs.uniform(-a2, a2, (S, n_out))),
             in_scale=rs.uniform(0.5, 2.0, (G, n_in)), in_shift=rs.uniform(-0.2, 0.2, (G, n_in)),
             t_scale=rs.uniform(0.5, 2.0, (G, n_out)), t_shift=rs.uniform(-0.2, 0.2, (G, n_out)))
    c["U"] = rs.randn(G, t_in, n_in) / c["in_scale"][:, None, :]              # unit variance after scaling
    c["D"] = rs.randn(G, T, n_out)
    kw = dict(group_offset=off, in_scale=c["in_scale"], in_shift=c["in_shift"], t_scale=c["t_scale"],
              t_shift=c["t_shift"], epochs=epochs, lr=LR)
    ref = fnn_ref.train_groups(c["U"], c["D"], c["init"], w, transient, **kw)
    rev = fnn_ref.train_groups(c["U"], c["D"], c["init"], w, transient, reverse=True, **kw)
    s = max(np.abs(rev[n] - ref[n]).max() for n in NAMES)
    n_rows = T - max(transient, w - 1)
    if nh * k * n_rows <= LONGDOUBLE_MACS:
        ld = fnn_ref.train_groups(c["U"], c["D"], c["init"], w, transient, groups=[0], dtype=np.longdouble, **kw)
        s = max(s, max(float(np.abs(ld[n][0] - ref[n][0]).max()) for n in NAMES))
    c.update(ref=ref, s=s, bound=max(16.0 * epochs * LR * (n_rows + k + nh) * 2.0 ** -53, 64.0 * s))
    for v in list(c.values()) + list(ref.values()) + list(c["init"]):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def make_bank(shape, c, groups=slice(None)):
    n_in, w, nh, n_out = shape[:4]
    bank = fnn_mod.FnnBank(n_in, n_out, nh, w, n_groups=shape[6])
    bank.set_scaling(c["in_scale"][groups], c["in_shift"][groups], c["t_scale"][groups], c["t_shift"][groups])
    return bank


def train(shape, c, groups=slice(None), first=0, init=None, want_loss=False):
    n_in, w, nh, n_out, t_in, T, G, S, off, transient, epochs = shape
    bank = make_bank(shape, c, groups)
    bank.train(c["U"][groups], c["D"][groups], c["init"] if init is None else init, transient=transient, epochs=epochs,
               lr=LR, group_offset=off + first, want_loss=want_loss)
    return bank


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_training_matches_the_float64_restatement(shape):
    c = make_case(shape)
    ref = c["ref"]
    assert ref["min_pre"] > 1e-9, ref["min_pre"]                  # precondition on the host side
    bank = train(shape, c, want_loss=True)
    for n in NAMES:
        got = getattr(bank, n).cpu().numpy()
        assert got.shape == ref[n].shape and np.isfinite(got).all()
        err = np.abs(got - ref[n]).max()
        print("train", IDS[SHAPES.index(shape)], n, "err", err, "bound", c["bound"], "ratio", err / c["bound"], "s", c["s"])
        assert err <= c["bound"]
    loss = bank.loss.cpu().numpy()
    rel = (np.abs(loss - ref["loss"]) / np.abs(ref["loss"])).max()
    print("train", IDS[SHAPES.index(shape)], "loss rel err", rel, "ratio", rel / c["bound"], "first / last",
          ref["loss"][0, 0], ref["loss"][0, -1], "min |pre|", ref["min_pre"])
    assert loss.shape == ref["loss"].shape and rel <= c["bound"]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_a_group_alone_and_any_chunking_are_bitwise_the_batch(shape):
    import torch
    G = shape[6]
    c = make_case(shape)
    whole = train(shape, c, want_loss=True)
    g = G - 1
    alone = train(shape, c, groups=slice(g, g + 1), first=g, want_loss=True)
    for n in NAMES + ("loss",):
        assert torch.equal(getattr(alone, n)[0], getattr(whole, n)[g]), n
    without = train(shape, c)                                      # and the loss output changes nothing
    for n in NAMES:
        assert torch.equal(getattr(without, n), getattr(whole, n)), n
    if G > 1:
        cut = (G + 1) // 2
        a = train(shape, c, groups=slice(0, cut))
        b = train(shape, c, groups=slice(cut, G), first=cut)
        for n in NAMES:
            assert torch.equal(torch.cat([getattr(a, n), getattr(b, n)]), getattr(whole, n)), n


def test_a_unit_that_is_never_active_is_bitwise_untouched():
    shape = SHAPES[1]
    c = make_case(shape)
    init = [t.copy() for t in c["init"]]
    dead = 17
    init[1][:, dead] = -100.0
    bank = train(shape, c, init=init)
    W1, b1, W2 = bank.W1.cpu().numpy(), bank.b1.cpu().numpy(), bank.W2.cpu().numpy()
    for g in range(shape[6]):
        np.testing.assert_array_equal(W1[g, dead], init[0][0, dead])
        assert b1[g, dead] == -100.0
        np.testing.assert_array_equal(W2[g, :, dead], init[2][0, :, dead])
        assert np.abs(W1[g, dead - 1] - init[0][0, dead - 1]).max() > 1e-3
    assert all(np.isfinite(getattr(bank, n).cpu().numpy()).all() for n in NAMES)


def test_unserved_shapes_and_precisions_are_refused_with_a_message():
    import torch
    from esn_ofdm_mimo_amd import _lib
    lib = _lib.load()

    def raw(precision, n_in, nh, w, n_out, T, work_bytes=None):
        k = w * n_in
        z = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device="cuda")   # noqa: E731
        U, D = torch.zeros((1, T, n_in), dtype=torch.float64, device="cuda"), z(1, T, n_out)
        init = [z(1, nh, k), z(1, nh), z(1, n_out, nh), z(1, n_out)]
        out = [z(1, nh, k), z(1, nh), z(1, n_out, nh), z(1, n_out)]
        need = int(lib.esn_fnn_workspace_bytes(n_in, nh, w, n_out, 1, T))
        work = torch.empty(max(1, need // 8), dtype=torch.float64, device="cuda")
        rc = lib.esn_fnn_train(precision, n_in, nh, w, n_out, 1, *[t.data_ptr() for t in init], None, None, None, None,
                               U.data_ptr(), D.data_ptr(), 1, T, T, w - 1, 0, 3, 0.01, 0.9, 0.999, 1e-8,
                               *[t.data_ptr() for t in out], None, work.data_ptr(),
                               need if work_bytes is None else work_bytes, _lib.stream_handle())
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in out)                 # nothing ran
        return rc, lib.esn_last_error().decode()

    rc, msg = raw(_lib.F64, 16, 128, 8, 8, 138)
    assert rc == -1 and "LDS" in msg, (rc, msg)
    rc, msg = raw(_lib.F64, 4, 600, 1, 1, 20)
    assert rc == -1 and "512" in msg, (rc, msg)
    rc, msg = raw(_lib.F64, 32, 10, 16, 1, 20)
    assert rc == -1 and "256" in msg, (rc, msg)
    rc, msg = raw(_lib.F64, 4, 100, 8, 9, 74)
    assert rc == -1 and "n_out" in msg, (rc, msg)
    rc, msg = raw(_lib.F64, 4, 100, 8, 4, 74, work_bytes=8)
    assert rc == -1 and "workspace" in msg, (rc, msg)
    for precision in (_lib.F32, _lib.F16, _lib.BF16):
        rc, msg = raw(precision, 4, 100, 8, 4, 74)
        assert rc == -2 and msg, (precision, rc, msg)
    bank = fnn_mod.FnnBank(16, 8, 128, 8)
    with pytest.raises(ValueError, match="LDS"):
        bank.train(np.zeros((1, 138, 16)), np.zeros((1, 138, 8)), fnn_mod.init_weights(128, 128, 8))
    bank = fnn_mod.FnnBank(4, 4, 100, 8)
    bank.set_weights(*fnn_mod.init_weights(32, 100, 4))
    with pytest.raises(ValueError, match="precision"):
        bank.predict(np.zeros((1, 74, 4)), 1, precision="f32")
    Y = torch.empty((1, 74, 4), dtype=torch.float64, device="cuda")
    args = [4, 100, 8, 4, bank.W1.data_ptr(), bank.b1.data_ptr(), bank.W2.data_ptr(), bank.b2.data_ptr(), None, None, None,
            None, Y.data_ptr(), 1, 1, 74, 74, 0, Y.data_ptr(), _lib.stream_handle()]
    assert lib.esn_fnn_predict(_lib.F32, *args) == -2 and lib.esn_last_error()
    args[2] = 17
    assert lib.esn_fnn_predict(_lib.F64, *args) == -1 and b"window" in lib.esn_last_error()


def predict_case(shape, fpg):
    """Frames of a ragged last group (fpg > 1) and the parameters the restatement trained."""
    n_in, w, nh, n_out, t_in, T, G = shape[:7]
    c = make_case(shape)
    rs = np.random.RandomState(7 + fpg)
    B = G * fpg - (1 if fpg > 1 else 0)
    U = rs.randn(B, t_in, n_in) / c["in_scale"][np.arange(B) // fpg][:, None, :]
    prm = [c["ref"][n] for n in NAMES]
    return c, U, prm


@pytest.mark.parametrize("fpg", [1, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_predict_f64_matches_the_restatement(shape, fpg):
    import torch
    n_in, w, nh, n_out, t_in, T, G = shape[:7]
    delay_cp = shape[9]
    c, U, prm = predict_case(shape, fpg)
    bank = make_bank(shape, c)
    bank.set_weights(*prm)
    B = U.shape[0]
    grp = np.arange(B) // fpg
    bound = 1e-11 * (1.0 + np.abs(prm[2]).sum(axis=2) + np.abs(prm[3]))       # [G, n_out]
    sc = (c["in_scale"], c["in_shift"], c["t_scale"], c["t_shift"])
    for transient in sorted({0, w - 1, delay_cp}):
        ref = fnn_ref.predict(U, fpg, T, transient, *prm, w, *sc)
        Y = bank.predict(U, fpg, T=T, transient=transient)
        got = Y.cpu().numpy()
        assert got.shape == ref.shape and np.isfinite(got).all()
        excess = (np.abs(got - ref) * c["t_scale"][grp][:, None, :] / bound[grp][:, None, :]).max()
        print("predict", IDS[SHAPES.index(shape)], "fpg", fpg, "transient", transient, "err / bound", excess)
        assert excess <= 1.0
        if transient < w - 1:
            assert not got[:, :w - 1 - transient].any()
    # one frame alone is bitwise itself inside the batch (the last transient of the loop)
    k = B - 1
    g = int(grp[k])
    alone = make_bank(shape, c, slice(g, g + 1))
    alone.set_weights(*[t[g:g + 1] for t in prm])
    one = alone.predict(U[k:k + 1], fpg, T=T, transient=transient)
    assert torch.equal(one[0], Y[k])
    if fpg == 1:      # fused against hidden rows -> matmul with torch on the device
        dev = bank.W1.device
        us = torch.zeros((B, T, n_in), dtype=torch.float64, device=dev)
        us[:, :t_in] = torch.as_tensor(U, device=dev)
        us = us * bank.in_scale[:, None, :] + bank.in_shift[:, None, :]
        x = us.unfold(1, w, 1).permute(0, 1, 3, 2).reshape(B, T - w + 1, w * n_in)      # oldest sample first
        hid = torch.relu(torch.einsum("gtk,ghk->gth", x, bank.W1) + bank.b1[:, None, :])
        ys = torch.einsum("gth,goh->gto", hid, bank.W2) + bank.b2[:, None, :]
        two = ((ys - bank.t_shift[:, None, :]) / bank.t_scale[:, None, :]).cpu().numpy()[:, max(transient, w - 1) - (w - 1):]
        fused = got[:, max(transient, w - 1) - transient:]
        assert (np.abs(fused - two) * c["t_scale"][:, None, :] / bound[:, None, :]).max() <= 1.0


@pytest.mark.parametrize("shape", F16_SHAPES, ids=[IDS[SHAPES.index(s)] for s in F16_SHAPES])
def test_predict_f16_is_within_four_times_the_fp16_operand_error(shape):
    n_in, w, nh, n_out, t_in, T, G = shape[:7]
    fpg = 5
    c, U, prm = predict_case(shape, fpg)
    bank = make_bank(shape, c)
    bank.set_weights(*prm)
    args = (U, fpg, T, w - 1, *prm, w, c["in_scale"], c["in_shift"], c["t_scale"], c["t_shift"])
    ref64 = fnn_ref.predict(*args)
    ref16 = fnn_ref.predict(*args, fp16_operands=True)
    bound = 4.0 * np.abs(ref16 - ref64).max() / np.abs(ref64).max()
    got = bank.predict(U, fpg, T=T, transient=w - 1, precision="f16").cpu().numpy()
    assert got.shape == ref16.shape and np.isfinite(got).all()
    err = np.abs(got - ref16).max() / np.abs(ref64).max()
    print("f16", IDS[SHAPES.index(shape)], "err", err, "bound", bound, "ratio err / (bound / 4)", 4.0 * err / bound)
    assert err <= bound
    zero = bank.predict(U, fpg, T=T, transient=0, precision="f16").cpu().numpy()
    assert not zero[:, :w - 1].any()
    np.testing.assert_array_equal(zero[:, w - 1:], got)


def nmse_bound(x_hat_pilot, b_out, N=64, isi=8):
    """What an error of at most b_out in every entry of x_hat_temp can change the NMSE by: per stream the error vector e
    moves by at most delta = sqrt(2 N) b_out in norm, so |e|^2 by at most 2 |e| delta + delta^2."""
    x_hat = x_hat_pilot[0:N, 0::2] + 1j * x_hat_pilot[0:N, 1::2]
    x = GOLD["x_cp"][0][isi - 1:, :]
    delta = np.sqrt(2.0 * N) * b_out
    return sum((2.0 * np.linalg.norm(x_hat[:, i] - x[:, i]) * delta + delta ** 2) / np.linalg.norm(x[:, i]) ** 2
               for i in range(2))


def test_bank_class_and_train_mimo_fnn_reproduce_the_golden_training():
    r64, b_prm, b_out = float32_bound()
    init = [GOLD[n + "_0"] for n in NAMES]
    b_nmse = nmse_bound(x_hat_temp(r64, np.float64)[0], b_out)
    bank = fnn_mod.FnnBank(4, 4, 100, 8)
    bank.train(GOLD["ESN_input"][None], GOLD["ESN_output"][None], init)
    for n in NAMES:
        err = np.abs(getattr(bank, n).cpu().numpy()[0] - GOLD[n]).max()
        print("golden", n, "err", err, "bound", b_prm, "ratio", err / b_prm)
        assert err <= b_prm
    Y = bank.predict(np.ascontiguousarray(GOLD["inputs"]), 3).cpu().numpy()
    err = np.abs(Y - GOLD["x_hat_temp"]).max()
    print("golden x_hat_temp err", err, "bound", b_out, "ratio", err / b_out)
    assert err <= b_out and not Y[:, :7].any()

    res = fnn_mod.trainMIMOFNN(GOLD["y_cp"][0], GOLD["x_cp"][0], 64, 2, 7, 8, init=init)
    ESN_input, ESN_output, model, Delay, idx, dmin, dmax, n_forget, nmse = res
    np.testing.assert_array_equal(ESN_input, GOLD["ESN_input"])
    np.testing.assert_array_equal(ESN_output, GOLD["ESN_output"])
    assert (Delay, idx, dmin, dmax, n_forget) == ([3] * 4, 3, 3, 3, int(GOLD["nForgetPoints"]))
    print("trainMIMOFNN NMSE", nmse, "golden", float(GOLD["NMSE"]), "bound", b_nmse)
    assert abs(nmse - float(GOLD["NMSE"])) <= b_nmse
    for n in NAMES:
        assert np.abs(getattr(model, n) - GOLD[n]).max() <= b_prm
    # the class surface on windowed matrices, its parameters drawn as the reference's model draws them
    import torch
    torch.manual_seed(int(GOLD["seed"]))
    net = fnn_mod.FNN(32)
    np.testing.assert_array_equal(net.W1, GOLD["W1_0"].astype(np.float64))
    net.fit(fnn_mod.window_rows(GOLD["ESN_input"], 8), GOLD["ESN_output"][7:])
    for n in NAMES:
        assert np.abs(getattr(net, n) - GOLD[n]).max() <= b_prm
    want = GOLD["x_hat_temp"][1, 7:]
    assert np.abs(net.predict(fnn_mod.window_rows(GOLD["inputs"][1], 8)) - want).max() <= b_out
    assert net.loss.shape == (50,) and net.loss[-1] < 0.05 * net.loss[0]


def numpy_fnn_point(src, ebno, si, n_blocks, F, n_hidden, window, seed, rows, first_block=0):
    """The loop of fnn_point in NumPy on the device's own frames: per-block errors, bits, the smallest distance of an
    X_hat coordinate from a slicer boundary and the smallest |pre-activation| of the trainings."""
    from esn_ofdm_mimo_amd.points import fnn_weights
    from esn_ofdm_mimo_amd.frames import _view_real
    p = src.p
    d, T, n_in, n_out = p.delay, p.t_frame + p.delay, 2 * p.n_r, 2 * p.n_t
    data = src.blocks_fast(ebno, si, first_block, n_blocks, F)
    py, px = _view_real(data["pilot_y"]).cpu().numpy(), _view_real(data["pilot_x"]).cpu().numpy()
    dy, bits = _view_real(data["data_y"]).cpu().numpy(), data["data_bits"].cpu().numpy()
    init = fnn_weights(n_hidden, window * n_in, n_out, seed)
    scale = 1.0 / np.sqrt(p.var_x(ebno))
    transient = max(p.forget, window - 1)
    side, norm = remod_ref.slicer_constants(p.m)
    errs, margin, min_pre = [], np.inf, np.inf
    for g in range(n_blocks):
        U = np.zeros((T, n_in))
        D = np.zeros((T, n_out))
        U[:p.t_frame], D[d:] = py[g], px[g]
        r = fnn_ref.train(U, D, init, window, transient, in_scale=scale, t_scale=scale)
        min_pre = min(min_pre, r["min_pre"])
        Y = fnn_ref.predict(dy[g * F:(g + 1) * F], F, T, 0, *(r[n][None] for n in NAMES), window,
                            in_scale=np.full((1, n_in), scale), t_scale=np.full((1, n_out), scale))
        r = remod_ref.detect_remod(Y[:, rows:rows + p.n_sub], F, p.n_sub, p.cp, d, p.n_t, p.m, [p.p_i(ebno)],
                                   tx_bits=bits[g * F:(g + 1) * F])
        errs.append(int(r["err"][0]))
        xy = np.stack([r["X_hat"].real, r["X_hat"].imag]) * norm             # boundaries at the even integers
        inner = np.abs(xy) < side - 2 + 1.0
        margin = min(margin, np.abs(xy - 2.0 * np.rint(xy / 2.0))[inner].min() / norm if inner.any() else np.inf)
    return np.array(errs), F * p.n_sub * p.m * p.n_t, margin, min_pre


POINT_CASES = [("2x2-N64-qpsk", dict(n_t=2, n_r=2, n_sub=64, m=2, channel="exp"), 15.0),
               ("4x8-N128-16qam", dict(), 21.0)]
POINT_SEED = 3


@pytest.mark.parametrize("name,link,ebno", POINT_CASES, ids=[c[0] for c in POINT_CASES])
def test_fnn_point_counts_what_the_numpy_loop_counts(name, link, ebno):
    from esn_ofdm_mimo_amd import montecarlo as mc
    p = mc.LinkParams(**link)
    src = mc.FrameSource(p, seed=11)
    G, F, kw = 6, 4, dict(n_hidden=100, window=8, seed=POINT_SEED, frames_per_block=4)
    ber = {}
    for sl, rows in (("aligned", p.forget), ("reference", 0)):
        want, nb, margin, min_pre = numpy_fnn_point(src, ebno, 2, G, F, 100, 8, POINT_SEED, rows)
        assert margin > 1e-8, margin                  # preconditions on the NumPy side: nothing sits on a boundary
        assert min_pre > 1e-9, min_pre                # and no ReLU on its kink
        err, bits = mc.fnn_point(src, ebno, 2, G, slice=sl, **kw)
        print("fnn_point", name, sl, "errors", err.cpu().numpy(), "numpy", want, "margin", margin, "min |pre|", min_pre)
        np.testing.assert_array_equal(err.cpu().numpy(), want)
        assert (bits.cpu().numpy() == nb).all()
        ber[sl] = want.sum() / (G * nb)
    print("fnn_point", name, "BER", ber)
    assert 0.45 <= ber["reference"] <= 0.55 and ber["aligned"] < ber["reference"], ber


def test_fnn_point_is_the_same_in_one_call_and_in_two():
    import torch
    from esn_ofdm_mimo_amd import montecarlo as mc
    src = mc.FrameSource(mc.LinkParams(n_t=2, n_r=2, n_sub=64, m=2, channel="exp"), seed=11)
    kw = dict(n_hidden=100, window=8, seed=POINT_SEED, frames_per_block=4)
    for weights in ("shared", "per_block"):
        e8, b8 = mc.fnn_point(src, 15.0, 1, 8, weights=weights, **kw)
        e3, b3 = mc.fnn_point(src, 15.0, 1, 3, weights=weights, chunk_blocks=2, **kw)
        e5, b5 = mc.fnn_point(src, 15.0, 1, 5, weights=weights, first_block=3, **kw)
        assert torch.equal(e8, torch.cat([e3, e5])) and torch.equal(b8, torch.cat([b3, b5]))
        assert int(b8.sum()) == 8 * 4 * 64 * 2 * 2 and int(e8.sum()) < int(b8.sum()) // 2


def test_fnn_point_refuses_bad_arguments_before_any_device_work():
    from esn_ofdm_mimo_amd import montecarlo as mc
    src = mc.FrameSource(mc.LinkParams(n_t=2, n_r=2, n_sub=64, m=2, channel="exp"), seed=11)
    for bad in (dict(slice="early"), dict(weights="fresh"), dict(precision="f32"), dict(window=0), dict(epochs=0),
                dict(n_hidden=600), dict(chunk_blocks=0), dict(frames_per_block=0)):
        with pytest.raises(ValueError):
            mc.fnn_point(src, 15.0, 0, 2, **bad)
    big = mc.FrameSource(mc.LinkParams(), seed=11)
    with pytest.raises(ValueError, match="LDS"):
        mc.fnn_point(big, 21.0, 0, 2, n_hidden=128)
