"""The LSTM comparator on the device (csrc/esn_lstm.hip, esn_ofdm_mimo_amd/lstm.py, points.lstm_point) against the NumPy
restatement tests/lstm_ref.py and the reference's own numbers (tests/golden/lstm.npz).

Inputs have unit variance after scaling, the initial parameters are U(+-1 / sqrt(H)); scalings and shifts differ per
group and are non-zero.
  training            every parameter and the relative loss[g][e] within max(16 epochs lr T (H + n_in + 1) 2^-53, 64 s) of
                      the float64 restatement: the first term is the rounding of one pre-activation's sum carried through
                      `epochs` steps of size at most lr over T rows; s is the largest difference between the float64
                      restatement and itself with every sum's terms in reversed order, with every tanh and sigma moved
                      one ulp up (every group) and, where the training has at most LONGDOUBLE_MACS multiply-adds, in
                      longdouble (first group) -- computed here from the restatement, never from the device.  A group
                      alone and any two-way chunking are bitwise the batch; want_loss changes nothing; at T = 1 W_hh and
                      the forget-gate rows are bitwise the initial set's.
  predict             within max(64 d, 1e-13 max |Y|), d the largest difference between the restatement in float64 and
                      in longdouble on the first two frames; the last frame alone bitwise itself in the batch;
                      frames_per_group 19 crosses a 16-frame tile, the last group is ragged.
  golden              LstmBank, LSTM and trainMIMOLSTM meet the reference's float32 training at the float32 bounds of
                      tests/test_lstm_reference_cpu.py; the NMSE at that bound carried through its formula.
  lstm_point          per-block error counts equal to the same loop in NumPy on the device's own frames, for a seed at
                      which no X_hat of the restatement lies within 1e-8 of a slicer boundary (asserted).
The ratios are printed."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_ref  # noqa: E402
import remod_ref  # noqa: E402
from lstm_ref import NAMES  # noqa: E402
from test_lstm_reference_cpu import ELM, ESN_INPUT, ESN_OUTPUT, GOLD, INPUTS, float32_bound, golden_init, stored, x_hat_temp  # noqa: E402
from esn_ofdm_mimo_amd import lstm as lstm_mod  # noqa: E402

pytestmark = pytest.mark.gpu

# n_in, H, n_out, T_in, T, n_groups, n_isets, group_offset, transient, epochs
SHAPES = [
    (2, 3, 1, 1, 1, 1, 1, 0, 0, 3),                       # T = 1: no recurrent step
    (2, 5, 1, 2, 2, 2, 1, 0, 0, 3),                       # exactly one recurrent step
    (4, 100, 4, 71, 74, 3, 1, 0, 0, 50),                  # the reference's shape
    (16, 100, 8, 135, 138, 5, 3, 7, 10, 50),              # the 4x8 shape, rotating initial sets
    (4, 7, 3, 19, 23, 2, 2, 1, 2, 10),                    # everything odd, H below one MFMA tile
    (6, 128, 2, 13, 17, 1, 1, 0, 0, 5),                   # the largest H (columns 96 .. 127 of W_hh streamed)
    (64, 16, 8, 9, 9, 1, 1, 0, 0, 3),                     # the largest n_in and n_out
]
IDS = ["in%d-H%d-o%d-T%d_%d-G%d-S%d-off%d-tr%d-ep%d" % s for s in SHAPES]
LR = 0.01
LONGDOUBLE_MACS = 2e7         # 12 H (H + n_in + 1) T epochs above this: s comes from the reversed order and the nudge
                              # alone, which can only make the bound smaller
PREDICT_LD_FRAMES = 2         # frames of a prediction restated in longdouble


def train_macs(shape):
    n_in, H, n_out, t_in, T = shape[:5]
    return 12 * H * (H + n_in + 1) * T * shape[9]


@functools.lru_cache(maxsize=None)
def make_case(shape):
    """Host arrays of one shape, the float64 restatement of every group's training and the sensitivity s."""
    n_in, H, n_out, t_in, T, G, S, off, transient, epochs = shape
    rs = np.random.RandomState(1000 * H + 10 * n_in + T)
    a = 1.0 / np.sqrt(H)
    init = tuple(rs.uniform(-a, a, (S,) + s) for s in ((4 * H, n_in), (4 * H, H), (4 * H,), (4 * H,), (n_out, H), (n_out,)))
    sign = lambda *s: np.where(rs.rand(*s) < 0.5, -1.0, 1.0)       # noqa: E731
    case = dict(init=init,
                in_scale=rs.uniform(0.5, 2.0, (G, n_in)), in_shift=sign(G, n_in) * rs.uniform(0.05, 0.2, (G, n_in)),
                t_scale=rs.uniform(0.5, 2.0, (G, n_out)), t_shift=sign(G, n_out) * rs.uniform(0.05, 0.2, (G, n_out)))
    case["U"] = rs.randn(G, t_in, n_in) / case["in_scale"][:, None, :]             # unit variance after scaling
    case["D"] = rs.randn(G, T, n_out)
    kw = dict(group_offset=off, in_scale=case["in_scale"], in_shift=case["in_shift"], t_scale=case["t_scale"],
              t_shift=case["t_shift"], epochs=epochs, lr=LR)
    ref = lstm_ref.train_groups(case["U"], case["D"], init, transient, **kw)
    diff = lambda a, b: max(max(float(np.abs(a[n] - b[n]).max()) for n in NAMES),                # noqa: E731
                            float((np.abs(a["loss"] - b["loss"]) / np.abs(b["loss"])).max()))
    s = max(diff(lstm_ref.train_groups(case["U"], case["D"], init, transient, reverse=True, **kw), ref),
            diff(lstm_ref.train_groups(case["U"], case["D"], init, transient, nudge=True, **kw), ref))
    if train_macs(shape) <= LONGDOUBLE_MACS:
        ld = lstm_ref.train_groups(case["U"], case["D"], init, transient, groups=[0], dtype=np.longdouble, **kw)
        s = max(s, diff(ld, {n: ref[n][:1] for n in NAMES + ("loss",)}))
    case.update(ref=ref, s=s, bound=max(16.0 * epochs * LR * T * (H + n_in + 1) * 2.0 ** -53, 64.0 * s))
    for v in list(case.values()) + list(ref.values()) + list(init):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def make_bank(shape, c, groups=slice(None)):
    n_in, H, n_out = shape[:3]
    bank = lstm_mod.LstmBank(n_in, n_out, H, n_groups=shape[5])
    bank.set_scaling(c["in_scale"][groups], c["in_shift"][groups], c["t_scale"][groups], c["t_shift"][groups])
    return bank


def train(shape, c, groups=slice(None), first=0, want_loss=False):
    off, transient, epochs = shape[7:]
    bank = make_bank(shape, c, groups)
    bank.train(c["U"][groups], c["D"][groups], c["init"], transient=transient, epochs=epochs, lr=LR,
               group_offset=off + first, want_loss=want_loss)
    return bank


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_training_matches_the_float64_restatement(shape):
    c = make_case(shape)
    ref = c["ref"]
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
          ref["loss"][0, 0], ref["loss"][0, -1])
    assert loss.shape == ref["loss"].shape and rel <= c["bound"]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_a_group_alone_and_any_chunking_are_bitwise_the_batch(shape):
    import torch
    H, T, G, S, off = shape[1], shape[4], shape[5], shape[6], shape[7]
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
    if T == 1:                         # no h[-1], no c[-1]: W_hh and the forget-gate rows never see a gradient
        fgt = slice(H, 2 * H)
        for gi in range(G):
            s = (off + gi) % S
            np.testing.assert_array_equal(whole.W_hh[gi].cpu().numpy(), c["init"][1][s])
            for k in (0, 2, 3):
                got = getattr(whole, NAMES[k])[gi].cpu().numpy()
                np.testing.assert_array_equal(got[fgt], c["init"][k][s][fgt])
                assert np.abs(got[:H] - c["init"][k][s][:H]).min() > 1e-4          # the input gate's rows moved


def test_unserved_shapes_and_precisions_are_refused_with_a_message():
    import torch
    from esn_ofdm_mimo_amd import _lib
    lib = _lib.load()
    z = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device="cuda")   # noqa: E731

    def sets(n_in, H, n_out):
        n_in, H, n_out = max(n_in, 1), max(H, 1), max(n_out, 1)
        return [z(*s) for s in ((1, 4 * H, n_in), (1, 4 * H, H), (1, 4 * H), (1, 4 * H), (1, n_out, H), (1, n_out))]

    def raw(precision, n_in, H, n_out, T, work_bytes=None, transient=0, epochs=3):
        U, D = torch.zeros((1, T, max(n_in, 1)), dtype=torch.float64, device="cuda"), z(1, T, max(n_out, 1))
        init, out = sets(n_in, H, n_out), sets(n_in, H, n_out)
        loss = z(1, max(epochs, 1))
        need = int(lib.esn_lstm_workspace_bytes(n_in, H, n_out, 1, 0, T))
        work = torch.empty(max(1, need // 8), dtype=torch.float64, device="cuda")
        rc = lib.esn_lstm_train(precision, n_in, H, n_out, 1, *[t.data_ptr() for t in init], None, None, None, None,
                                U.data_ptr(), D.data_ptr(), 1, T, T, transient, 0, epochs, 0.01, 0.9, 0.999, 1e-8,
                                *[t.data_ptr() for t in out], loss.data_ptr(), work.data_ptr(),
                                max(need, 8) if work_bytes is None else work_bytes, _lib.stream_handle())
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in out + [loss])        # nothing ran
        return rc, lib.esn_last_error().decode()

    rc, msg = raw(_lib.F64, 4, 129, 4, 74)
    assert rc == -1 and "n_hidden" in msg and "128" in msg, (rc, msg)
    rc, msg = raw(_lib.F64, 4, 0, 4, 74)
    assert rc == -1 and "n_hidden" in msg, (rc, msg)
    rc, msg = raw(_lib.F64, 65, 100, 4, 74)
    assert rc == -1 and "64" in msg, (rc, msg)
    rc, msg = raw(_lib.F64, 4, 100, 9, 74)
    assert rc == -1 and "n_out" in msg, (rc, msg)
    rc, msg = raw(_lib.F64, 4, 100, 4, 4097)
    assert rc == -1 and "4096" in msg, (rc, msg)
    rc, msg = raw(_lib.F64, 4, 100, 4, 74, transient=74)
    assert rc == -1 and "transient" in msg, (rc, msg)
    rc, msg = raw(_lib.F64, 4, 100, 4, 74, epochs=0)
    assert rc == -1 and "epochs" in msg, (rc, msg)
    rc, msg = raw(_lib.F64, 4, 100, 4, 74, work_bytes=8)
    assert rc == -1 and "workspace" in msg, (rc, msg)
    for precision in (_lib.F32, _lib.F16, _lib.BF16):
        rc, msg = raw(precision, 4, 100, 4, 74)
        assert rc == -2 and msg, (precision, rc, msg)
    bank = lstm_mod.LstmBank(4, 4, 129)
    with pytest.raises(ValueError, match="n_hidden"):
        bank.train(np.zeros((1, 74, 4)), np.zeros((1, 74, 4)), [t.cpu().numpy()[0] for t in sets(4, 129, 4)])
    bank = lstm_mod.LstmBank(4, 4)
    bank.set_weights(*lstm_mod.init_weights(4, 4))
    for precision in ("f16", "f32"):
        with pytest.raises(ValueError, match="precision"):
            bank.predict(np.zeros((1, 74, 4)), 1, precision=precision)
    Y = z(1, 74, 4)
    work = torch.empty(1 << 20, dtype=torch.float64, device="cuda")
    args = [4, 100, 4] + [getattr(bank, n).data_ptr() for n in NAMES] + [None, None, None, None, Y.data_ptr(), 1, 1, 74, 74,
            0, Y.data_ptr(), work.data_ptr(), 8 << 20, _lib.stream_handle()]
    for precision in (_lib.F32, _lib.F16, _lib.BF16):
        assert lib.esn_lstm_predict(precision, *args) == -2 and lib.esn_last_error()
    args[1] = 129
    assert lib.esn_lstm_predict(_lib.F64, *args) == -1 and b"n_hidden" in lib.esn_last_error()
    args[1], args[-2] = 100, 8
    assert lib.esn_lstm_predict(_lib.F64, *args) == -1 and b"workspace" in lib.esn_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(Y).all())


@functools.lru_cache(maxsize=None)
def predict_case(shape, fpg):
    """Frames of a ragged last group (fpg > 1), the parameters the restatement trained, the restatement's un-cut output
    and d = max |float64 - longdouble| of it over the first PREDICT_LD_FRAMES frames."""
    n_in, H, n_out, t_in, T, G = shape[:6]
    c = make_case(shape)
    rs = np.random.RandomState(7 + fpg)
    B = G * fpg - (1 if fpg > 1 else 0)
    U = rs.randn(B, t_in, n_in) / c["in_scale"][np.arange(B) // fpg][:, None, :]
    prm = [c["ref"][n] for n in NAMES]
    sc = (c["in_scale"], c["in_shift"], c["t_scale"], c["t_shift"])
    ref = lstm_ref.predict(U, fpg, T, 0, prm, *sc)
    n_ld = min(B, PREDICT_LD_FRAMES)
    ld = lstm_ref.predict(U[:n_ld], fpg, T, 0, prm, *sc, dtype=np.longdouble)
    d = float(np.abs(ld - ref[:n_ld]).max())
    for v in (U, ref):
        v.setflags(write=False)
    return c, U, prm, ref, d


@pytest.mark.parametrize("fpg", [1, 5, 19])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_predict_matches_the_restatement(shape, fpg):
    import torch
    T = shape[4]
    c, U, prm, ref, d = predict_case(shape, fpg)
    bank = make_bank(shape, c)
    bank.set_weights(*prm)
    B = U.shape[0]
    bound = max(64.0 * d, 1e-13 * np.abs(ref).max())
    for transient in sorted({0, shape[8]}):
        Y = bank.predict(U, fpg, T=T, transient=transient)
        got = Y.cpu().numpy()
        assert got.shape == ref[:, transient:].shape and np.isfinite(got).all()
        err = np.abs(got - ref[:, transient:]).max()
        print("predict", IDS[SHAPES.index(shape)], "fpg", fpg, "transient", transient, "err", err, "bound", bound,
              "ratio", err / bound)
        assert err <= bound
    # the last frame alone is bitwise itself inside the batch (the last transient of the loop)
    f = B - 1
    g = f // fpg
    alone = make_bank(shape, c, slice(g, g + 1))
    alone.set_weights(*[t[g:g + 1] for t in prm])
    one = alone.predict(U[f:f + 1], fpg, T=T, transient=transient)
    assert torch.equal(one[0], Y[f])


def test_bank_class_and_train_mimo_lstm_reproduce_the_golden_training():
    from test_gpu_cnn import nmse_bound
    r64, b_prm, b_out = float32_bound()
    init = golden_init()
    b_nmse = nmse_bound(x_hat_temp(r64, np.float64)[0], b_out)
    bank = lstm_mod.LstmBank(4, 4)
    bank.train(ESN_INPUT[None], ESN_OUTPUT[None], init)
    for n in NAMES:
        err = np.abs(stored(n, getattr(bank, n).cpu().numpy()[0]) - GOLD[n]).max()
        print("golden", n, "err", err, "bound", b_prm, "ratio", err / b_prm)
        assert err <= b_prm
    Y = bank.predict(np.ascontiguousarray(INPUTS), 3).cpu().numpy()
    err = np.abs(Y - GOLD["x_hat_temp"]).max()
    print("golden x_hat_temp err", err, "bound", b_out, "ratio", err / b_out)
    assert err <= b_out

    res = lstm_mod.trainMIMOLSTM(ELM["y_cp"][0], ELM["x_cp"][0], 64, 2, 7, 8, init=init)
    ESN_input, ESN_output, model, Delay, idx, dmin, dmax, n_forget, nmse = res
    np.testing.assert_array_equal(ESN_input, ESN_INPUT)
    np.testing.assert_array_equal(ESN_output, ESN_OUTPUT)
    assert (Delay, idx, dmin, dmax, n_forget) == ([3] * 4, 3, 3, 3, int(GOLD["nForgetPoints"]))
    print("trainMIMOLSTM NMSE", nmse, "golden", float(GOLD["NMSE"]), "bound", b_nmse)
    assert abs(nmse - float(GOLD["NMSE"])) <= b_nmse
    for n in NAMES:
        assert np.abs(stored(n, getattr(model, n)) - GOLD[n]).max() <= b_prm
    # the class surface, its parameters drawn as the reference's model draws them
    import torch
    torch.manual_seed(int(GOLD["seed"]))
    net = lstm_mod.LSTM()
    np.testing.assert_array_equal(net.W_hh, init[1])
    net.fit(ESN_INPUT, ESN_OUTPUT)
    for n in NAMES:
        assert np.abs(stored(n, getattr(net, n)) - GOLD[n]).max() <= b_prm
    assert np.abs(net.predict(INPUTS[1]) - GOLD["x_hat_temp"][1]).max() <= b_out
    assert net.loss.shape == (50,) and net.loss[-1] < net.loss[0]


def numpy_lstm_point(src, ebno, si, n_blocks, F, seed, first_block=0):
    """The loop of lstm_point in NumPy on the device's own frames: per-block errors of the two slices, bits per block and
    the smallest distance of an X_hat coordinate from a slicer boundary."""
    from esn_ofdm_mimo_amd.points import lstm_weights
    from esn_ofdm_mimo_amd.frames import _view_real
    p = src.p
    d, T, n_in, n_out = p.delay, p.t_frame + p.delay, 2 * p.n_r, 2 * p.n_t
    data = src.blocks_fast(ebno, si, first_block, n_blocks, F)
    py, px = _view_real(data["pilot_y"]).cpu().numpy(), _view_real(data["pilot_x"]).cpu().numpy()
    dy, bits = _view_real(data["data_y"]).cpu().numpy(), data["data_bits"].cpu().numpy()
    init = lstm_weights(100, n_in, n_out, seed)
    scale = 1.0 / np.sqrt(p.var_x(ebno))
    side, norm = remod_ref.slicer_constants(p.m)
    errs, margin = {"aligned": [], "reference": []}, np.inf
    for g in range(n_blocks):
        U = np.zeros((T, n_in))
        D = np.zeros((T, n_out))
        U[:p.t_frame], D[d:] = py[g], px[g]
        r = lstm_ref.train(U, D, init, p.forget, in_scale=scale, t_scale=scale)
        Y = lstm_ref.predict(dy[g * F:(g + 1) * F], F, T, 0, [r[n][None] for n in NAMES],
                             in_scale=np.full((1, n_in), scale), t_scale=np.full((1, n_out), scale))
        for sl, rows in (("aligned", p.forget), ("reference", 0)):
            r2 = remod_ref.detect_remod(Y[:, rows:rows + p.n_sub], F, p.n_sub, p.cp, d, p.n_t, p.m, [p.p_i(ebno)],
                                        tx_bits=bits[g * F:(g + 1) * F])
            errs[sl].append(int(r2["err"][0]))
            xy = np.stack([r2["X_hat"].real, r2["X_hat"].imag]) * norm          # boundaries at the even integers
            inner = np.abs(xy) < side - 2 + 1.0
            if inner.any():
                margin = min(margin, np.abs(xy - 2.0 * np.rint(xy / 2.0))[inner].min() / norm)
    return {k: np.array(v) for k, v in errs.items()}, F * p.n_sub * p.m * p.n_t, margin


POINT_CASES = [("2x2-N64-qpsk", dict(n_t=2, n_r=2, n_sub=64, m=2, channel="exp"), 15.0),
               ("4x8-N128-16qam", dict(), 21.0)]
POINT_SEED = 3


@pytest.mark.parametrize("name,link,ebno", POINT_CASES, ids=[c[0] for c in POINT_CASES])
def test_lstm_point_counts_what_the_numpy_loop_counts(name, link, ebno):
    """The only BER assertion is on the reference's slice, which is delay + cp rows early and so near one half.  The
    aligned slice is printed, not asserted: 41 000 parameters trained 50 epochs on one pilot over-fit it, as the FNN and
    the CNN do here."""
    from esn_ofdm_mimo_amd import montecarlo as mc
    p = mc.LinkParams(**link)
    src = mc.FrameSource(p, seed=11)
    G, F = 6, 4
    want, nb, margin = numpy_lstm_point(src, ebno, 2, G, F, POINT_SEED)
    assert margin > 1e-8, margin                      # precondition on the NumPy side: nothing sits on a boundary
    ber = {}
    for sl in ("aligned", "reference"):
        err, bits = mc.lstm_point(src, ebno, 2, G, slice=sl, seed=POINT_SEED, frames_per_block=F)
        print("lstm_point", name, sl, "errors", err.cpu().numpy(), "numpy", want[sl], "margin", margin)
        np.testing.assert_array_equal(err.cpu().numpy(), want[sl])
        assert (bits.cpu().numpy() == nb).all()
        ber[sl] = want[sl].sum() / (G * nb)
    print("lstm_point", name, "BER", ber)
    assert 0.45 <= ber["reference"] <= 0.55, ber


def test_lstm_point_is_the_same_in_one_call_and_in_two():
    import torch
    from esn_ofdm_mimo_amd import montecarlo as mc
    src = mc.FrameSource(mc.LinkParams(n_t=2, n_r=2, n_sub=64, m=2, channel="exp"), seed=11)
    kw = dict(seed=POINT_SEED, frames_per_block=4)
    for weights in ("shared", "per_block"):
        e8, b8 = mc.lstm_point(src, 15.0, 1, 8, weights=weights, **kw)
        e3, b3 = mc.lstm_point(src, 15.0, 1, 3, weights=weights, chunk_blocks=2, **kw)
        e5, b5 = mc.lstm_point(src, 15.0, 1, 5, weights=weights, first_block=3, **kw)
        assert torch.equal(e8, torch.cat([e3, e5])) and torch.equal(b8, torch.cat([b3, b5]))
        assert int(b8.sum()) == 8 * 4 * 64 * 2 * 2


def test_lstm_point_refuses_bad_arguments_before_any_device_work():
    from esn_ofdm_mimo_amd import montecarlo as mc
    src = mc.FrameSource(mc.LinkParams(n_t=2, n_r=2, n_sub=64, m=2, channel="exp"), seed=11)
    for bad in (dict(slice="early"), dict(weights="fresh"), dict(n_hidden=129), dict(n_hidden=0), dict(n_hidden=100.0),
                dict(epochs=0), dict(epochs=2.5), dict(lr=-1.0), dict(chunk_blocks=0), dict(frames_per_block=0),
                dict(n_blocks=0), dict(first_block=-1)):
        kw = dict(n_blocks=2)
        kw.update(bad)
        n_blocks = kw.pop("n_blocks")
        with pytest.raises(ValueError):
            mc.lstm_point(src, 15.0, 0, n_blocks, **kw)
