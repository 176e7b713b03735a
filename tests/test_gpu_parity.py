"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle and the
reference-generated golden vectors.  Run with `pytest -m gpu` on an MI355X.

Tolerances (written per test):
  f64 kernels  : 1e-9 relative to max|expected| (float64 round-off + LAPACK-vs-QR);
  f32 MFMA     : 1e-5 relative (SURVEY section 4 tier 2);
  f16/bf16 MFMA: 1e-2 relative AND >= 99.9 % identical hard-decision bits.
"""
import numpy as np
import pytest

from oracle import esn_oracle as eo
from oracle.ofdm_frames import LinkConfig, make_frame, tdlb_mimo_taps

pytestmark = pytest.mark.gpu


def rel_err(got, want):
    return float(np.max(np.abs(got - want)) / (np.max(np.abs(want)) + 1e-300))


@pytest.fixture(scope="module")
def amd():
    from esn_ofdm_mimo_amd import pyESN, helper_mimo_esn_generic, batched
    return pyESN, helper_mimo_esn_generic, batched


PLAIN = {
    "tiny": dict(n_in=3, n_out=2, n_res=8,
                 kw=dict(spectral_radius=0.9, sparsity=0.25, input_scaling=[0.3, 0.2, 0.1],
                         input_shift=[0.0, 0.1, -0.1], teacher_scaling=0.5, teacher_shift=0.05)),
    "c2": dict(n_in=2, n_out=2, n_res=100,
               kw=dict(spectral_radius=0.9, sparsity=0.1, input_scaling=0.05 * np.ones(2),
                       input_shift=np.zeros(2), teacher_scaling=5e-3 * np.ones(2),
                       teacher_shift=np.zeros(2))),
}


@pytest.mark.parametrize("name", list(PLAIN))
@pytest.mark.parametrize("tag,noise", [("n0", 0.0), ("n1", 0.001)])
def test_dropin_fit_predict_vs_reference_golden(amd, golden, name, tag, noise):
    """2-D drop-in: same seed -> same weights, same noise stream -> reference outputs."""
    pyESN = amd[0]
    g, c = golden(name), PLAIN[name]
    tr = int(g["transient"])
    esn = pyESN.ESN(c["n_in"], c["n_out"], c["n_res"], noise=noise, random_state=int(g["seed"]), **c["kw"])
    pred_train = esn.fit(g["u"], g["d"], tr)
    assert esn.fit_status == 0
    assert rel_err(esn.laststate, g[tag + "_laststate"]) < 1e-11
    np.testing.assert_allclose(esn.lastoutput, g[tag + "_lastoutput"], rtol=1e-13)
    assert rel_err(pred_train, g[tag + "_pred_train"]) < 1e-8
    assert rel_err(esn.W_out, g[tag + "_W_out"]) < 1e-6
    assert rel_err(esn.predict(g["u2"], 0, continuation=True), g[tag + "_pred_cont"]) < 1e-8
    assert rel_err(esn.predict(g["u2"], tr, continuation=False), g[tag + "_pred_fresh"]) < 1e-8


def _helper_esn(mod, cfg, n_res, seed, ebno, noise, **extra):
    n_in, n_out = 2 * cfg.n_r, 2 * cfg.n_t
    return mod.ESN(n_in, n_out, n_res, spectral_radius=0.9, sparsity=0.1, noise=noise,
                   input_shift=np.zeros(n_in), input_scaling=cfg.input_scaling(ebno) * np.ones(n_in),
                   teacher_scaling=cfg.teacher_scale * np.ones(n_out), teacher_shift=np.zeros(n_out),
                   feedback_scaling=np.zeros(n_out), random_state=seed, **extra)


HELPER = {"c3": (LinkConfig(n_t=2, n_r=2, n_sub=512), 100), "c4": (LinkConfig(), 512), "c4s": (LinkConfig(), 300)}


@pytest.mark.parametrize("name", list(HELPER))
def test_helper_dropin_vs_reference_golden(amd, golden, name):
    pyESN, helper, _ = amd
    g = golden(name)
    cfg, n_res = HELPER[name]
    seed, ebno = int(g["seed"]), float(g["ebno_db"])
    esn = _helper_esn(pyESN, cfg, n_res, seed, ebno, 0.0)
    ret = helper.trainMIMOESN_generic(esn, 0, cfg.min_delay, cfg.max_delay, cfg.cp, cfg.n_sub, cfg.n_t,
                                      cfg.n_r, cfg.isi, g["pilot_y"], g["pilot_x"])
    x_in, x_out, esn2, delay, d_idx, d_min, d_max, forget, nmse = ret
    assert esn2 is esn and len(ret) == 9
    np.testing.assert_array_equal(x_in, g["esn_in"])
    np.testing.assert_array_equal(x_out, g["esn_out"])
    np.testing.assert_array_equal(delay, g["delay"])
    assert (d_idx, d_min, d_max, forget) == (int(g["d_idx"]), int(g["d_min"]), int(g["d_max"]), int(g["forget"]))
    assert rel_err(esn.laststate, g["n0_laststate"]) < 1e-10
    assert nmse == pytest.approx(float(g["n0_nmse"]), rel=1e-4)
    # W_out through its action on the reference-side extended states
    oracle = eo.OracleESN(2 * cfg.n_r, 2 * cfg.n_t, n_res, spectral_radius=0.9, sparsity=0.1, noise=0.0,
                          input_shift=np.zeros(2 * cfg.n_r),
                          input_scaling=cfg.input_scaling(ebno) * np.ones(2 * cfg.n_r),
                          teacher_scaling=cfg.teacher_scale * np.ones(2 * cfg.n_t),
                          teacher_shift=np.zeros(2 * cfg.n_t), random_state=seed)
    oracle.fit(x_in, x_out, forget)
    ext = oracle._ext_states[forget:]
    assert rel_err(ext @ esn.W_out.T, ext @ g["n0_W_out"].T) < 1e-7
    # data frames: reference predictions with the reference's W_out
    esn.W_out = g["n0_W_out"]
    for y_cp, want in zip(g["data_y"], g["data_pred"]):
        got = esn.predict(eo.pack_rx(y_cp, d_max), forget, continuation=False)
        assert rel_err(got, want) < 1e-8


def _c4_batch(golden, amd, precision, noise=0.0):
    pyESN = amd[0]
    g = golden("c4")
    cfg, n_res = HELPER["c4"]
    esn = _helper_esn(pyESN, cfg, n_res, int(g["seed"]), float(g["ebno_db"]), noise)
    esn.W_out = g["n0_W_out"]
    d = int(g["d_max"])
    u = np.stack([eo.pack_rx(y, d) for y in g["data_y"]])
    got = esn.predict(u, int(g["forget"]), continuation=False, precision=precision)
    return g, cfg, got


@pytest.mark.parametrize("precision,tol", [("f64", 1e-8), ("f32", 1e-5), ("f16", 1e-2), ("bf16", 3e-2)])
def test_batched_predict_c4_vs_reference_golden(amd, golden, precision, tol):
    """16 frames of the 4x8 N_res=512 case in one launch vs the reference's own predictions."""
    g, cfg, got = _c4_batch(golden, amd, precision)
    want = g["data_pred"]
    assert got.shape == want.shape
    err = rel_err(got, want)
    assert err < tol, (precision, err)
    # hard decisions: identical bits on >= 99.9 % of positions
    const = eo.unit_qam(cfg.m)
    p_i = cfg.p_i(float(g["ebno_db"]))
    same = tot = 0
    for a, b in zip(got, want):
        ba = eo.hard_bits(eo.time_to_freq(eo.outputs_to_time_signals(a, g["delay"], int(g["d_min"]), cfg.n_sub, cfg.n_t), cfg.n_sub, p_i), const, cfg.m)
        bb = eo.hard_bits(eo.time_to_freq(eo.outputs_to_time_signals(b, g["delay"], int(g["d_min"]), cfg.n_sub, cfg.n_t), cfg.n_sub, p_i), const, cfg.m)
        same += int(np.sum(ba == bb))
        tot += ba.size
    # bf16 (8 significant bits) is offered for range, not accuracy: 99 % is its bar
    assert same / tot >= (0.99 if precision == "bf16" else 0.999), (precision, same / tot)


@pytest.mark.parametrize("precision", ["f64", "f32", "f16"])
def test_ragged_batch_and_groups(amd, precision):
    """3 groups x 37 frames (not a multiple of any tile), per-group W_out and scalings, short inputs
    (T_in < T: zero rows synthesised) -- every frame must equal its own single-frame f64 result."""
    _, _, batched = amd
    rs = np.random.RandomState(3)
    n_in, n_out, n_res, t_in, t, tr, G, F = 4, 2, 40, 20, 23, 3, 3, 37
    w, w_in, w_fb = eo.draw_weights(rs, n_in, n_out, n_res, 0.9, 0.1)
    bank = batched.ReservoirBank(n_in, n_out, n_res, w, w_in, w_fb, noise=0.0)
    in_scale = rs.rand(G, n_in) + 0.5
    in_shift = rs.randn(G, n_in) * 0.1
    t_scale = rs.rand(G, n_out) + 0.5
    t_shift = rs.randn(G, n_out) * 0.1
    bank.set_scaling(in_scale, in_shift, t_scale, t_shift)
    w_out = rs.randn(G, n_out, n_res + n_in) * 0.1
    bank.set_readout(w_out)
    u = rs.randn(G * F, t_in, n_in)
    x0 = rs.randn(G, n_res) * 0.1
    y0 = rs.randn(G, n_out) * 0.1
    got = bank.predict(u, F, T=t, transient=tr, precision=precision, x0=x0, y0=y0).cpu().numpy()
    assert got.shape == (G * F, t - tr, n_out)
    tol = {"f64": 1e-10, "f32": 2e-5, "f16": 2e-2}[precision]
    for b in (0, 1, 36, 37, 73, 74, 110):
        grp = b // F
        o = eo.OracleESN(n_in, n_out, n_res, noise=0.0, input_scaling=in_scale[grp], input_shift=in_shift[grp],
                         teacher_scaling=t_scale[grp], teacher_shift=t_shift[grp], random_state=1)
        o.W, o.W_in, o.W_feedb, o.W_out = w, w_in, w_fb, w_out[grp]
        o.laststate, o.lastoutput = x0[grp], y0[grp]
        upad = np.vstack([u[b], np.zeros((t - t_in, n_in))])
        want = o.predict(upad, tr, continuation=True)
        assert rel_err(got[b], want) < tol, (precision, b, rel_err(got[b], want))


@pytest.mark.parametrize("n_res,n_in,n_out,G,F", [(256, 16, 8, 5, 75), (512, 16, 8, 5, 75), (1024, 16, 8, 5, 75),
                                                  (512, 4, 4, 5, 75), (512, 2, 2, 5, 75), (512, 16, 8, 2, 301),
                                                  (384, 8, 6, 3, 37)])
@pytest.mark.parametrize("noise_mode,noise", [("none", 0.0), ("counter", 1e-3), ("tensor", 1e-3)])
def test_skewed_schedule_matches_in_step_schedule(amd, noise_mode, noise, n_res, n_in, n_out, G, F):
    """The fp16 predict kernel of 8-wave tilings (N_res 256 / 512 / 1024: 128, 128 and 64 frames per
    tile) runs the skewed wave schedule; the debug knob skew=0 selects the in-step schedule of the same arithmetic.  Ragged groups (tiles straddle groups and padding slots), short
    inputs (rows past T_in are zeros), per-group read-outs, initial state / feedback, both noise modes."""
    import os
    _, _, batched = amd
    rs = np.random.RandomState(11)
    t_in, t, tr = 30, 34, 4
    w, w_in, w_fb = eo.draw_weights(rs, n_in, n_out, n_res, 0.9, 0.1)
    bank = batched.ReservoirBank(n_in, n_out, n_res, w, w_in, w_fb, noise=noise)
    in_scale, in_shift = rs.rand(G, n_in) * 0.2 + 0.1, rs.randn(G, n_in) * 0.05
    t_scale, t_shift = rs.rand(G, n_out) + 0.5, rs.randn(G, n_out) * 0.1
    bank.set_scaling(in_scale, in_shift, t_scale, t_shift)
    w_out = rs.randn(G, n_out, n_res + n_in) * 0.004           # weak feedback: rounding differences are not amplified
    bank.set_readout(w_out)
    u = rs.randn(G * F - 9, t_in, n_in)                       # last group is short
    x0, y0 = rs.randn(G, n_res) * 0.1, rs.randn(G, n_out) * 0.1
    kw = dict(T=t, transient=tr, precision="f16", x0=x0, y0=y0, noise_mode=noise_mode, seed=5)
    if noise_mode == "tensor":
        if (n_res, n_in) != (512, 16):
            pytest.skip("tensor noise: one shape is enough")
        kw["noise_u"] = rs.rand(u.shape[0], t, n_res)
    from esn_ofdm_mimo_amd import _lib
    assert os.environ.get("ESN_SKEW") is None
    assert _lib.recur_path(False, "f16", bank.shape, u.shape[0], F) == ("skew16" if 256 < n_res <= 512 else "mfma")
    skew = bank.predict(u, F, **kw).cpu().numpy()
    _lib.debug_set("skew", "0")
    try:
        plain = bank.predict(u, F, **kw).cpu().numpy()
    finally:
        _lib.debug_set("skew", "1")
    assert skew.shape == plain.shape == (G * F - 9, t - tr, n_out)
    # 257..512 units: the default is the 16x16x32 kernel (esn_recur_skew16_impl.h: its own weight / read-out images, k
    # order and LDS layout); knob s16=0 selects the 32x32x16 skewed kernel on the same inputs and noise draws
    _lib.debug_set("s16", "0")
    try:
        assert _lib.recur_path(False, "f16", bank.shape, u.shape[0], F) == "mfma"
        skew32 = bank.predict(u, F, **kw).cpu().numpy()
    finally:
        _lib.debug_set("s16", "1")
    assert rel_err(skew, skew32) < (2e-3 if noise == 0.0 else 8e-3), rel_err(skew, skew32)
    assert rel_err(skew32, plain) < (2e-3 if noise == 0.0 else 8e-3), rel_err(skew32, plain)
    if 256 < n_res <= 512 and noise_mode == "counter":
        assert not np.array_equal(skew, skew32)                      # (the knob did select another kernel)
    # same weights, same noise draws; only the summation order of the read-out and the rounding of
    # the noise addition (packed half: one more rounding to fp16 per state) differ
    assert rel_err(skew, plain) < (2e-3 if noise == 0.0 else 8e-3), rel_err(skew, plain)
    if noise == 0.0:
        for b in (0, F - 1, F, 2 * F - 50, G * F - 10):
            grp = b // F
            o = eo.OracleESN(n_in, n_out, n_res, noise=0.0, input_scaling=in_scale[grp], input_shift=in_shift[grp],
                             teacher_scaling=t_scale[grp], teacher_shift=t_shift[grp], random_state=1)
            o.W, o.W_in, o.W_feedb, o.W_out = w, w_in, w_fb, w_out[grp]
            o.laststate, o.lastoutput = x0[grp], y0[grp]
            want = o.predict(np.vstack([u[b], np.zeros((t - t_in, n_in))]), tr, continuation=True)
            assert rel_err(skew[b], want) < 2e-2, (b, rel_err(skew[b], want))


@pytest.mark.parametrize("precision,tol", [("f64", 1e-11), ("f32", 1e-5)])
def test_harvest_batch_shared_reservoir(amd, precision, tol):
    """G pilots through one shared reservoir: E[g] equals the oracle's extended states."""
    _, _, batched = amd
    rs = np.random.RandomState(11)
    n_in, n_out, n_res, t, G = 6, 4, 70, 33, 5
    w, w_in, w_fb = eo.draw_weights(rs, n_in, n_out, n_res, 0.9, 0.1)
    bank = batched.ReservoirBank(n_in, n_out, n_res, w, w_in, w_fb, noise=0.0)
    in_scale, t_scale = rs.rand(G, n_in) + 0.5, rs.rand(G, n_out) + 0.5
    bank.set_scaling(in_scale, None, t_scale, None)
    u, d = rs.randn(G, t, n_in), rs.randn(G, t, n_out)
    E = bank.harvest(u, d, precision=precision).cpu().numpy()
    for g in range(G):
        o = eo.OracleESN(n_in, n_out, n_res, noise=0.0, input_scaling=in_scale[g], teacher_scaling=t_scale[g],
                         random_state=1)
        o.W, o.W_in, o.W_feedb = w, w_in, w_fb
        o.fit(u[g], d[g], 0)
        assert rel_err(E[g], o._ext_states) < tol


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_float32_extended_states_fast_path(amd, precision):
    """esn_harvest_batch_f32 / esn_readout_solve_chol_batch_f32: the same harvest stored as float32 and
    the same float64 Cholesky arithmetic on it.  State columns must be bit-identical to the float64
    harvest (MFMA states are float32/fp16 values), input columns equal to float32 rounding, and the
    read-out equal to the float64-E read-out far below the fit's own accuracy."""
    import torch
    _, _, batched = amd
    rs = np.random.RandomState(21)
    n_in, n_out, n_res, t, tr, G = 16, 8, 512, 138, 10, 37
    w, w_in, w_fb = eo.draw_weights(rs, n_in, n_out, n_res, 0.9, 0.1)
    bank = batched.ReservoirBank(n_in, n_out, n_res, w, w_in, w_fb, noise=1e-3)
    bank.set_scaling(rs.rand(G, n_in) * 0.2 + 0.1, rs.randn(G, n_in) * 0.05, rs.rand(G, n_out) + 0.5,
                     rs.randn(G, n_out) * 0.1)
    u, d = rs.randn(G, t, n_in), rs.randn(G, t, n_out) * 0.3
    e64 = bank.harvest(u, d, precision=precision, noise_mode="counter", seed=9)
    e32 = bank.harvest(u, d, precision=precision, noise_mode="counter", seed=9, e_dtype="f32")
    assert e32.dtype == torch.float32 and e32.shape == e64.shape
    assert torch.equal(e32[..., :n_res].double(), e64[..., :n_res])                  # states: exact
    assert torch.equal(e32[..., n_res:], e64[..., n_res:].float())                   # inputs: one rounding
    w64, st64 = bank.solve(e64, d, tr, method="chol")
    w32, st32 = bank.solve(e32, d, tr, method="chol")
    assert int(st64.sum()) == 0 and int(st32.sum()) == 0
    assert rel_err(w32.cpu().numpy(), w64.cpu().numpy()) < 1e-6
    # QR on float32 states goes through a float64 copy
    wq, _ = bank.solve(e32, d, tr, method="qr")
    assert rel_err(wq.cpu().numpy(), w64.cpu().numpy()) < 1e-5
    with pytest.raises(Exception):
        bank.harvest(u[:2], d[:2], precision="f64", e_dtype="f32")


def test_per_group_reservoirs(amd):
    """Reference-faithful mode: one (W, W_in, W_fb) per group, fit + predict against the oracle."""
    _, _, batched = amd
    rs = np.random.RandomState(5)
    n_in, n_out, n_res, t, G, F = 4, 2, 48, 40, 3, 5
    ws = [eo.draw_weights(np.random.RandomState(100 + g), n_in, n_out, n_res, 0.9, 0.2) for g in range(G)]
    bank = batched.ReservoirBank(n_in, n_out, n_res, np.stack([w[0] for w in ws]), np.stack([w[1] for w in ws]),
                                 np.stack([w[2] for w in ws]), noise=0.0)
    u = rs.randn(G, t, n_in)
    d = np.tanh(u @ rs.randn(n_in, n_out)) + 0.3 * np.roll(u[:, :, :n_out], 1, axis=1)   # learnable teacher
    bank.fit(u, d, transient=4, precision="f64", noise_mode="none")
    assert int(bank.fit_status.sum().item()) == 0
    u2 = rs.randn(G * F, t, n_in)
    got = bank.predict(u2, F, transient=2, precision="f64").cpu().numpy()
    got32 = bank.predict(u2, F, transient=2, precision="f32").cpu().numpy()
    for g in range(G):
        o = eo.OracleESN(n_in, n_out, n_res, noise=0.0, random_state=1)
        o.W, o.W_in, o.W_feedb = ws[g]
        o.fit(u[g], d[g], 4)
        assert rel_err(bank.W_out[g].cpu().numpy() @ o._ext_states[4:].T, o.W_out @ o._ext_states[4:].T) < 1e-8
        o.W_out = bank.W_out[g].cpu().numpy()
        for f in range(F):
            want = o.predict(u2[g * F + f], 2, continuation=False)
            assert rel_err(got[g * F + f], want) < 1e-9
            # 36 equations / 52 unknowns: the min-norm W_out amplifies float32 state round-off
            # (cancellation in the readout), hence the looser float32 bound
            assert rel_err(got32[g * F + f], want) < 5e-3


@pytest.mark.parametrize("method,tol", [("qr", 1e-9), ("chol", 1e-7)])
@pytest.mark.parametrize("rows,cols", [(128, 528), (40, 40), (512, 104), (300, 90),
                                       # Gram dimension beyond 128: the workspace (out-of-LDS) Cholesky kernel --
                                       # 4x8 at N = 512 (512 x 528), N_res = 300 at N = 512 (512 x 316), ragged tiles
                                       (512, 528), (512, 316), (200, 700), (130, 131), (333, 150)])
def test_readout_solve_vs_pinv(amd, rows, cols, method, tol):
    _, _, batched = amd
    rs = np.random.RandomState(rows + cols)
    G, n_out, tr = 3, 4, 5
    bank = batched.ReservoirBank(cols - 2, n_out, 2, np.zeros((2, 2)), np.zeros((2, cols - 2)), np.zeros((2, n_out)))
    E = rs.randn(G, rows + tr, cols)
    E[:, :, :3] *= 1e-3                      # uneven column scales
    D = rs.randn(G, rows + tr, n_out)
    t_scale = rs.rand(G, n_out) + 0.5
    bank.set_scaling(None, None, t_scale, None)
    W, status = bank.solve(E, D, tr, method=method)
    assert int(status.sum().item()) == 0
    for g in range(G):
        want = (np.linalg.pinv(E[g, tr:]) @ (D[g, tr:] * t_scale[g])).T
        assert rel_err(W[g].cpu().numpy(), want) < tol


def test_chol_flags_rank_deficiency_and_qr_repairs(amd):
    """A duplicated row makes the Gram singular: the Cholesky path must say so (status 1), and the
    QR re-solve of the flagged group must match pinv's minimum-norm answer on the consistent part."""
    _, _, batched = amd
    rs = np.random.RandomState(8)
    G, rows, cols, n_out = 3, 20, 50, 2
    bank = batched.ReservoirBank(cols - 2, n_out, 2, np.zeros((2, 2)), np.zeros((2, cols - 2)), np.zeros((2, n_out)))
    E = rs.randn(G, rows, cols)
    D = rs.randn(G, rows, n_out)
    E[1, 7] = E[1, 3]
    D[1, 7] = D[1, 3]                       # consistent duplicate: pinv solution exists and is finite
    W, status = bank.solve(E, D, 0, method="chol")
    st = status.cpu().numpy()
    assert st[0] == 0 and st[2] == 0 and st[1] == 1
    import torch
    n = bank.resolve_failed(torch.as_tensor(E, device=W.device), D, 0, W, status)
    assert n == 1
    for g in (0, 2):
        assert rel_err(W[g].cpu().numpy(), (np.linalg.pinv(E[g]) @ D[g]).T) < 1e-7
    # flagged group after QR: reproduces the teacher on every row (the duplicate included)
    assert rel_err(E[1] @ W[1].cpu().numpy().T, D[1]) < 1e-6


def test_big_chol_float32_states_and_rank_flag(amd):
    """The workspace Cholesky kernel on float32 extended states (the batched fit's storage) and its pivot flag."""
    import torch
    _, _, batched = amd
    rs = np.random.RandomState(77)
    G, rows, cols, n_out = 4, 256, 528, 8
    bank = batched.ReservoirBank(cols - 2, n_out, 2, np.zeros((2, 2)), np.zeros((2, cols - 2)), np.zeros((2, n_out)))
    E = rs.randn(G, rows, cols).astype(np.float32)
    D = rs.randn(G, rows, n_out)
    E[2, 100] = E[2, 17]
    D[2, 100] = D[2, 17]
    W, status = bank.solve(torch.as_tensor(E, device="cuda"), D, 0, method="chol")
    st = status.cpu().numpy()
    assert list(st) == [0, 0, 1, 0]
    for g in (0, 1, 3):
        want = (np.linalg.pinv(E[g].astype(np.float64)) @ D[g]).T
        assert rel_err(W[g].cpu().numpy(), want) < 1e-7
    n = bank.resolve_failed(torch.as_tensor(E, device="cuda").double(), D, 0, W, status)
    assert n == 1
    assert rel_err(E[2].astype(np.float64) @ W[2].cpu().numpy().T, D[2]) < 1e-6


def test_detect_count_vs_oracle(amd, golden):
    _, _, batched = amd
    g = golden("c4")
    cfg = LinkConfig()
    bits = np.unpackbits(g["data_bits"])[:np.prod(g["data_bits_shape"])].reshape(g["data_bits_shape"])
    pred = g["data_pred"]                                  # [16, 128, 8]
    p_i = cfg.p_i(float(g["ebno_db"]))
    bank = batched.ReservoirBank(2, 2, 2, np.zeros((2, 2)), np.zeros((2, 2)), np.zeros((2, 2)))
    F = 8                                                  # two groups of 8 frames
    err, nb, xh = bank.detect_count(pred, bits.astype(np.uint8), np.array([p_i, p_i]), F, cfg.n_sub, cfg.n_t,
                                    cfg.m, want_xhat=True)
    const = eo.unit_qam(cfg.m)
    want_err = np.zeros(2, dtype=np.int64)
    for i, (y, b) in enumerate(zip(pred, bits)):
        x_hat = eo.time_to_freq(eo.outputs_to_time_signals(y, g["delay"], int(g["d_min"]), cfg.n_sub, cfg.n_t), cfg.n_sub, p_i)
        got_x = xh[i].cpu().numpy().view(np.complex128).reshape(cfg.n_sub, cfg.n_t)
        assert rel_err(got_x, x_hat) < 1e-12
        want_err[i // F] += eo.count_bit_errors(b, eo.hard_bits(x_hat, const, cfg.m))
    np.testing.assert_array_equal(err.cpu().numpy(), want_err)        # integer work: bit-exact
    np.testing.assert_array_equal(nb.cpu().numpy(), [F * cfg.n_sub * cfg.m * cfg.n_t] * 2)


@pytest.mark.parametrize("n_sub,n_t,m", [(64, 4, 4), (128, 2, 2), (32, 1, 6), (256, 3, 4), (2048, 5, 2)])
def test_detect_count_shapes(amd, n_sub, n_t, m):
    """Even and odd log2 N (paired radix-2 stages + a lone last stage), 1..5 antennas (N=2048 x 5
    needs two workgroups per frame), 4/16/64-QAM: spectrum vs numpy FFT, counts bit-exact."""
    _, _, batched = amd
    rs = np.random.RandomState(n_sub + n_t)
    B, F = 7, 3
    const = eo.unit_qam(m)
    bits = rs.randint(0, 2, (B, n_sub * m, n_t)).astype(np.uint8)
    p_i = np.array([0.7, 1.3, 2.1])
    bank = batched.ReservoirBank(2, 2, 2, np.zeros((2, 2)), np.zeros((2, 2)), np.zeros((2, 2)))
    y = rs.randn(B, n_sub, 2 * n_t) * np.sqrt(n_sub)
    err, nb, xh = bank.detect_count(y, bits, p_i, F, n_sub, n_t, m, want_xhat=True)
    want = np.zeros(3, dtype=np.int64)
    for i in range(B):
        x_t = y[i, :, 0::2] + 1j * y[i, :, 1::2]                                  # [N, n_t]
        x_hat = np.fft.fft(x_t, axis=0) / n_sub / np.sqrt(p_i[i // F])
        got = xh[i].cpu().numpy().view(np.complex128).reshape(n_sub, n_t)
        assert rel_err(got, x_hat) < 1e-12
        want[i // F] += eo.count_bit_errors(bits[i], eo.hard_bits(got, const, m))
    np.testing.assert_array_equal(err.cpu().numpy(), want)
    np.testing.assert_array_equal(nb.cpu().numpy(), [3 * n_sub * m * n_t, 3 * n_sub * m * n_t, n_sub * m * n_t])


def test_counter_noise_statistics(amd):
    """The counter generator is zero-mean uniform of width `noise`; outputs stay within the
    perturbation the reference's own state noise causes (statistical, not bit-equal)."""
    pyESN = amd[0]
    rs = np.random.RandomState(2)
    esn = pyESN.ESN(3, 2, n_reservoir=64, spectral_radius=0.5, noise=0.01, random_state=9)
    esn.W_out = rs.randn(2, 67) * 0.0
    esn.W_out[0, :64] = 1.0 / 64          # y0 = mean(state)
    esn.W_out[1, 0] = 1.0                 # y1 = state[0]
    u = np.zeros((512, 50, 3))
    esn.teacher_forcing = False
    esn._bank = None
    y = esn.predict(u, 10, continuation=False, precision="f32", seed=123)
    # with zero input and no feedback x = noise*(u-0.5) + tanh(W x_prev): |x| <~ noise
    s = y[:, :, 1].ravel()
    assert abs(s.mean()) < 3e-4
    assert 0.8 * 0.01 / np.sqrt(12) < s.std() < 1.4 * 0.01 / np.sqrt(12)
    y2 = esn.predict(u, 10, continuation=False, precision="f32", seed=123)
    np.testing.assert_array_equal(y, y2)                 # same seed -> same stream
    y3 = esn.predict(u, 10, continuation=False, precision="f32", seed=124)
    assert np.abs(y3 - y).max() > 0


def _golden_batch(golden, amd, name, cfg, n_res, precision, w_out_key="n0_W_out"):
    pyESN = amd[0]
    g = golden(name)
    esn = _helper_esn(pyESN, cfg, n_res, int(g["seed"]), float(g["ebno_db"]), 0.0)
    esn.W_out = g[w_out_key]
    u = np.stack([eo.pack_rx(y, int(g["d_max"])) for y in g["data_y"]])
    return g, u, esn.predict(u, int(g["forget"]), continuation=False, precision=precision)


@pytest.mark.parametrize("name,precision,tol", [
    ("c3", "f32", 1e-5), ("c3", "f16", 1e-2),          # 2x2, N=512 (T=522), N_res=100: (4,1,2) tiles
    ("c4s", "f32", 1e-5), ("c4s", "f16", 1e-2),        # 4x8, N_res=300 (padded to 512 rows)
    ("c5", "f16", 2e-2),                                # 4x8, N_res=2048: 16-wave tiles, fp16 only
])
def test_other_geometries_vs_reference_golden(amd, golden, name, precision, tol):
    """Every tile geometry of the MFMA kernel against the reference's own predictions."""
    cfg, n_res = {"c3": HELPER["c3"], "c4s": HELPER["c4s"], "c5": (LinkConfig(), 2048)}[name]
    if name == "c3":
        # 512 equations / 104 unknowns fitted WITHOUT state noise is ill-conditioned (cond ~1e5,
        # SURVEY 7.2): that W_out amplifies any state round-off (float32: 3e-4, fp16: 0.4), which says
        # nothing about the kernels.  Use the reference's W_out of its default noise=0.001 fit and
        # the pinned oracle for the expected outputs.
        g, u, got = _golden_batch(golden, amd, name, cfg, n_res, precision, "n1_W_out")
        o = eo.OracleESN(2 * cfg.n_r, 2 * cfg.n_t, n_res, spectral_radius=0.9, sparsity=0.1, noise=0.0,
                         input_shift=np.zeros(2 * cfg.n_r),
                         input_scaling=cfg.input_scaling(float(g["ebno_db"])) * np.ones(2 * cfg.n_r),
                         teacher_scaling=cfg.teacher_scale * np.ones(2 * cfg.n_t),
                         teacher_shift=np.zeros(2 * cfg.n_t), random_state=int(g["seed"]))
        o.W_out = g["n1_W_out"]
        want = np.stack([o.predict(x, int(g["forget"]), continuation=False) for x in u])
    else:
        g, u, got = _golden_batch(golden, amd, name, cfg, n_res, precision)
        want = g["data_pred"]
    assert got.shape == want.shape
    assert rel_err(got, want) < tol, (name, precision, rel_err(got, want))


def test_f32_kernel_rejects_what_it_cannot_hold(amd):
    """float32 state of N_res=2048 does not fit LDS: the library must say so, not fall back."""
    from esn_ofdm_mimo_amd import _lib
    pyESN = amd[0]
    esn = pyESN.ESN(2, 2, n_reservoir=1100, random_state=4, noise=0.0)
    esn.W_out = np.zeros((2, 1102))
    with pytest.raises(_lib.EsnHipError, match="does not support"):
        esn.predict(np.zeros((2, 5, 2)), continuation=False, precision="f32")


@pytest.mark.parametrize("precision", ["f64", "f32", "f16", "bf16"])
@pytest.mark.parametrize("n_in,n_out,tf", [(3, 5, True), (1, 1, True), (6, 12, True), (5, 2, False)])
def test_odd_shapes_and_flags(amd, precision, n_in, n_out, tf):
    """Shapes off the fast paths: odd n_in (no LDS-DMA, kin_p not a power of two), n_out > 8 (two
    readout images in fp16), a single frame, transient = T-1, teacher_forcing off."""
    _, _, batched = amd
    rs = np.random.RandomState(100 * n_in + n_out)
    n_res, t, G, F = 70, 17, 2, 3
    w, w_in, w_fb = eo.draw_weights(rs, n_in, n_out, n_res, 0.8, 0.2)
    bank = batched.ReservoirBank(n_in, n_out, n_res, w, w_in, w_fb, teacher_forcing=tf, noise=0.0)
    t_scale = rs.rand(G, n_out) + 0.5
    bank.set_scaling(None, rs.randn(G, n_in) * 0.1, t_scale, None)
    w_out = rs.randn(G, n_out, n_res + n_in) * 0.05
    bank.set_readout(w_out)
    u = rs.randn(G * F, t, n_in) * 0.5
    tol = {"f64": 1e-10, "f32": 2e-5, "f16": 2e-2, "bf16": 2e-1}[precision]   # bf16: 8 significant bits
    for tr in (0, t - 1):
        got = bank.predict(u, F, transient=tr, precision=precision).cpu().numpy()
        assert got.shape == (G * F, t - tr, n_out)
        for b in range(G * F):
            grp = b // F
            o = eo.OracleESN(n_in, n_out, n_res, noise=0.0, input_shift=bank.in_shift[grp].cpu().numpy(),
                             teacher_scaling=t_scale[grp], teacher_forcing=tf, random_state=1)
            o.W, o.W_in, o.W_feedb, o.W_out = w, w_in, w_fb, w_out[grp]
            want = o.predict(u[b], tr, continuation=False)
            assert rel_err(got[b], want) < tol, (precision, n_in, n_out, tr, b, rel_err(got[b], want))
    one = bank.predict(u[:1], F, transient=0, precision=precision).cpu().numpy()     # a single frame
    full0 = bank.predict(u, F, transient=0, precision=precision).cpu().numpy()[0]
    if precision == "f64":      # ONE float64 sequence runs on the LDS-resident cluster kernel: other summation order
        assert rel_err(one[0], full0) < 1e-12
    else:
        np.testing.assert_array_equal(one[0], full0)


def test_argument_validation_on_device(amd):
    from esn_ofdm_mimo_amd import _lib
    _, _, batched = amd
    bank = batched.ReservoirBank(2, 2, 8, np.zeros((8, 8)), np.zeros((8, 2)), np.zeros((8, 2)), noise=0.0)
    with pytest.raises(AttributeError):
        bank.predict(np.zeros((2, 4, 2)), 2, precision="f64")          # predict before fit
    bank.set_readout(np.zeros((1, 2, 10)))
    with pytest.raises(ValueError, match="transient"):
        bank.predict(np.zeros((2, 4, 2)), 2, transient=4, precision="f64")   # transient >= T
    with pytest.raises(ValueError):
        bank.predict(np.zeros((4, 4, 2)), 2, precision="f64")          # 2 groups, readout holds 1


@pytest.mark.parametrize("precision,n_res,tol", [("f64", 48, 1e-9), ("f32", 48, 5e-3), ("f16", 512, 2e-2), ("f64", 512, 1e-9)])
def test_weight_sets_share_tiles_set_major(amd, precision, n_res, tol):
    """Reference-faithful mode with MORE groups than weight sets (group g uses set g % n_wsets, as the sweep's
    pool of pre-drawn reservoirs does): the kernels lay the slot axis out set-major, so a tile packs several
    groups of ONE set (20 groups over 8 sets: three per set for sets 0-3, two for sets 4-7; ragged last group).
    Harvest + solve + predict per group against the oracle with that group's own weights."""
    _, _, batched = amd
    rs = np.random.RandomState(17)
    n_in, n_out, t, G, F, S = 16, 8, 40, 20, 21, 8
    ws = [eo.draw_weights(np.random.RandomState(300 + k), n_in, n_out, n_res, 0.9, 0.2) for k in range(S)]
    bank = batched.ReservoirBank(n_in, n_out, n_res, np.stack([w[0] for w in ws]), np.stack([w[1] for w in ws]),
                                 np.stack([w[2] for w in ws]), noise=0.0)
    in_scale, t_scale = rs.rand(G, n_in) * 0.1 + 0.05, rs.rand(G, n_out) + 0.5
    bank.set_scaling(in_scale, None, t_scale, None)
    u = rs.randn(G, t, n_in)
    d = np.tanh(u[:, :, :n_out] * 0.1 + 0.05 * np.roll(u[:, :, :n_out], 1, axis=1))
    E = bank.harvest(u, d, precision=precision, noise_mode="none").cpu().numpy()
    w_out = rs.randn(G, n_out, n_res + n_in) * 0.01
    bank.set_readout(w_out)
    B = G * F - 5
    u2 = rs.randn(B, t, n_in)
    got = bank.predict(u2, F, transient=3, precision=precision, noise_mode="none").cpu().numpy()
    for g in (0, 7, 8, 13, 19):
        o = eo.OracleESN(n_in, n_out, n_res, noise=0.0, input_scaling=in_scale[g], teacher_scaling=t_scale[g], random_state=1)
        o.W, o.W_in, o.W_feedb = ws[g % S]
        o.fit(u[g], d[g], 0)
        assert rel_err(E[g], o._ext_states) < (1e-10 if precision == "f64" else 1e-2 if precision == "f16" else 1e-5), (g, precision)
        o.W_out = w_out[g]
        for b in (g * F, min(g * F + F - 1, B - 1)):
            want = o.predict(u2[b], 3, continuation=False)
            assert rel_err(got[b], want) < tol, (precision, g, b, rel_err(got[b], want))
