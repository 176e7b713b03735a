"""The CPU oracle against the reference drivers' OWN main loops (tests/golden/loop_*.npz).

The fixtures were written by executing the loop statements of three reference driver scripts
(make_golden.py, case_driver_loop).  Here every recorded block and frame is recomputed by the
oracle from the fixture's bits and taps, with the noise replayed from the recorded state of the
global NumPy stream in the driver's draw order, and compared sample for sample:

  frame recipe, channel, estimators, linear detectors ... 1e-12 of the array's largest magnitude
  OracleESN fit / predict, state noise on ................ the same bound
  helper return values, every running error counter ..... exactly equal

Exact counters are a fair demand because the generator only accepts a seed whose every recorded
X_hat component stays 1e3 * 1e-9 * max|X_hat| away from a decision boundary (stored as *_margin).

The tests also print cond(E) of every block's noise-on extended-state matrix and assert that
10 * cond(E) * 2**-52 stays below driver_loop.ESN_BOUND, the bound tests/test_gpu_driver_loop.py
grants the QR / Cholesky readout of the GPU against the reference's pinv."""

import numpy as np
import pytest

from oracle import baselines as ob
from oracle import driver_loop as dl
from oracle import esn_oracle as eo
from oracle import ofdm_frames as of

TOL = 1e-12


def close(got, want, what, tol=TOL):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    top = np.abs(want).max()
    dev = np.abs(got - want).max() / top
    print(f"{what}: {dev:.2e} of max")
    assert dev <= tol, (what, dev)


def check_conditioning(esn, transient, what):
    """cond(E) of the rows the readout is fitted on; the GPU bound must not rest on a luckier matrix."""
    c = float(np.linalg.cond(esn._ext_states[transient:]))
    print(f"{what}: E {esn._ext_states[transient:].shape}, cond(E) {c:.4g}, cond(E) * 2**-52 {c * 2.0 ** -52:.2e}")
    assert 10 * c * 2.0 ** -52 <= dl.ESN_BOUND, (what, c)


def esn_kwargs(cfg, scale_ebno):
    n_in, n_out = 2 * cfg.n_r, 2 * cfg.n_t
    return dict(spectral_radius=0.9, sparsity=0.1, input_shift=np.zeros(n_in),
                input_scaling=cfg.input_scaling(scale_ebno) * np.ones(n_in),
                teacher_scaling=cfg.teacher_scale * np.ones(n_out), teacher_shift=np.zeros(n_out),
                feedback_scaling=np.zeros(n_out))


def global_rng(state):
    np.random.set_state(state)
    return np.random.mtrand._rand


def train_from_state(fx, pre, i, cfg, scale_ebno, n_res, pilot_y, pilot_x):
    """OracleESN drawn from the global stream at the recorded state (weights first, then the state
    noise of the helper's fit / predict / fit), exactly as the driver's ESN(...) with no random_state."""
    rng = global_rng(dl.rng_state(fx, pre + f"esn{i}_state"))
    esn = eo.OracleESN(2 * cfg.n_r, 2 * cfg.n_t, n_res, random_state=rng, **esn_kwargs(cfg, scale_ebno))
    assert esn.noise == 0.001
    ret = eo.train_mimo_esn(esn, 0, cfg.min_delay, cfg.max_delay, cfg.cp, cfg.n_sub, cfg.n_t, cfg.n_r, cfg.isi,
                            pilot_y, pilot_x)
    helper = np.r_[np.asarray(ret[3]).ravel(), ret[4], ret[5], ret[6], ret[7]]
    np.testing.assert_array_equal(helper, fx[pre + f"esn{i}_helper"])
    close(ret[8], fx[pre + f"esn{i}_nmse"], pre + f"esn{i}_nmse", 1e-9)
    check_conditioning(esn, ret[7], pre + f"esn{i}")
    return esn, ret


def esn_xhat(esn, ret, cfg, ebno, y_cp, state):
    global_rng(state)
    x_hat, _ = eo.detect_frame(esn, y_cp, ret[3], ret[5], ret[6], ret[7], cfg.n_sub, cfg.n_t, cfg.p_i(ebno),
                               eo.unit_qam(cfg.m), cfg.m)
    return x_hat


def check_counters(fx, tag, pre, cfg, tx_bits, xhats):
    before, after = dl.counters(fx, pre + "counts_before"), dl.counters(fx, pre + "counts")
    const = eo.unit_qam(cfg.m)
    for name, x in xhats.items():
        x2 = np.asarray(x).reshape(cfg.n_sub, -1)
        errs = eo.count_bit_errors(tx_bits.reshape(cfg.n_sub * cfg.m, -1), eo.hard_bits(x2, const, cfg.m))
        c = dl.COUNTER_OF[tag][name]
        assert before[c] + errs == after[c], (pre, name, before[c], errs, after[c])
        assert dl.decision_margin(fx[pre + name], const) == pytest.approx(float(fx[pre + name + "_margin"]))
        assert float(fx[pre + name + "_margin"]) >= 1e3 * 1e-9 * np.abs(fx[pre + name]).max()
    assert set(xhats) == set(dl.COUNTER_OF[tag]) == {str(n) for n in fx["xhat_names"]}
    for c in dl.BIT_COUNTERS:
        if c in after:
            assert after[c] - before[c] == tx_bits.size


@pytest.mark.parametrize("tag", ["v2", "nbf"])
def test_mimo_driver_loop(golden, tag):
    fx = golden("loop_" + tag)
    cfg = dl.link_config(fx)
    n_res = int(fx["param_nInternalUnits"])
    assert fx["ebno_db"].min() <= 12 and fx["ebno_db"].max() >= 18
    gen = dl.code_generator(fx) if tag == "v2" else None
    for j, b, kk_pilot, ebno in dl.blocks(fx):
        pre = f"p{j}_b{b}_"
        taps_ref = fx[pre + "taps"]
        rng = global_rng(dl.rng_state(fx, pre + "state"))
        # ---- channel draw
        if tag == "v2":
            taps = of.tdlb_mimo_taps(cfg, int(1234 + ebno) + kk_pilot)      # its own Generator, not the global stream
        else:
            taps = of.exp_pdp_taps(cfg, rng)
        close(taps, taps_ref, pre + "taps")
        # ---- pilot and LS companion, one noise draw
        pf = ob.pilot_frames(cfg, ebno, taps_ref, rng)
        np.testing.assert_array_equal(pf["bits"], dl.bits(fx, pre + "pilot_bits"))
        for got, key in ((pf["X_LS"], "X_LS"), (pf["x_cp"], "pilot_x"), (pf["y_cp"], "pilot_y"),
                         (pf["y_ls_cp"], "pilot_y_ls")):
            close(got, fx[pre + key], pre + key)
        # the driver draws nothing between the pilot's noise and the ESN's weights
        assert dl.same_state(np.random.get_state(), dl.rng_state(fx, pre + "esn0_state"))
        # ---- estimators
        close(ob.estimate_channel(cfg, ebno, fx[pre + "X_LS"], fx[pre + "pilot_y_ls"]), fx[pre + "H_MMSE"], pre + "H_MMSE")
        h_ls = ob.estimate_channel(cfg, ebno, fx[pre + "X_LS"], fx[pre + "pilot_y_ls"], ls_only=True)
        if pre + "H_LS" in fx.files:        # every block of loop_nbf; loop_v2 keeps it at the first point only (size)
            close(h_ls, fx[pre + "H_LS"], pre + "H_LS")
        else:
            assert tag == "v2" and j == 1
        h_true = ob.taps_to_freq(cfg, taps_ref)
        if tag == "nbf":                    # the 4x8 driver forms no perfect-CSI channel
            close(h_true, fx[pre + "H_true"], pre + "H_true")
        # ---- ESN(s): weights and state noise from the global stream
        esns = [train_from_state(fx, pre, 0, cfg, ebno, n_res, fx[pre + "pilot_y"], fx[pre + "pilot_x"])]
        if tag == "nbf":
            # second ESN: the same pilot symbols at the fixed training power, a fresh noise draw that follows
            # the first ESN's training in the stream
            _, x_fix, x_fix_pa = of.modulate(pf["bits"], cfg, dl.TRAIN_EBNO_FIXED_DB)
            close(x_fix, fx[pre + "pilot_x_fixed"], pre + "pilot_x_fixed")
            close(of.channel(x_fix_pa, taps_ref, cfg, np.random.mtrand._rand), fx[pre + "pilot_y_fixed"],
                  pre + "pilot_y_fixed")
            assert dl.same_state(np.random.get_state(), dl.rng_state(fx, pre + "esn1_state"))
            esns.append(train_from_state(fx, pre, 1, cfg, dl.TRAIN_EBNO_FIXED_DB, n_res, fx[pre + "pilot_y_fixed"],
                                         fx[pre + "pilot_x_fixed"]))
        # ---- data frames of this block
        for kk in dl.frames_of(fx, j, b):
            fp = f"p{j}_f{kk}_"
            tx_bits = dl.bits(fx, fp + "bits")
            rng = global_rng(dl.rng_state(fx, fp + "state"))
            if tag == "v2":         # coded bits: k_info randint draws per stream through the test-made G
                info = [rng.randint(0, 2, size=(gen.shape[1],), dtype=np.int8) for _ in range(cfg.n_t)]
                np.testing.assert_array_equal(np.stack([(gen @ u) % 2 for u in info], axis=1), tx_bits)
            else:                   # the driver's uncoded branch
                np.testing.assert_array_equal(of.random_bits(cfg, rng), tx_bits)
            _, x_cp, x_pa = of.modulate(tx_bits.astype(np.int32), cfg, ebno)
            close(x_cp, fx[fp + "x_cp"], fp + "x_cp")
            close(of.channel(x_pa, taps_ref, cfg, rng), fx[fp + "y_cp"], fp + "y_cp")
            assert dl.same_state(np.random.get_state(), dl.rng_state(fx, fp + "predict0_state"))
            y_cp = fx[fp + "y_cp"]
            xh = {}
            names = ("X_hat_ESN",) if tag == "v2" else ("X_hat_ESN_m", "X_hat_ESN_f")
            for i, name in enumerate(names):
                xh[name] = esn_xhat(*esns[i], cfg, ebno, y_cp, dl.rng_state(fx, fp + f"predict{i}_state"))
            xh["X_hat_MMSE"] = ob.mmse_detect(cfg, ebno, fx[pre + "H_MMSE"], y_cp)
            if tag == "nbf":
                xh["X_hat_PerfZF"] = ob.linear_detect(cfg, ebno, h_true, y_cp, reg=0)
                xh["X_hat_LS_ZF"] = ob.linear_detect(cfg, ebno, h_ls, y_cp, reg=0)
            for name, x in xh.items():
                close(x, fx[fp + name], fp + name)
            check_counters(fx, tag, fp, cfg, tx_bits, xh)
    if tag == "nbf":
        assert max(b for _, b, _, _ in dl.blocks(fx)) == 1      # two coherence blocks at one point


def test_siso_driver_loop(golden):
    """Flat unit-modulus channel, QPSK, no CP, no helper: esn.fit on the pilot, then predict with the
    reference's default continuation=True.  predict never updates laststate / lastoutput (only fit does), so
    every frame restarts from the state and teacher output fit() left: frames are independent of each other."""
    fx = golden("loop_siso")
    cfg = dl.link_config(fx)
    assert (cfg.n_t, cfg.n_r, cfg.cp, cfg.m) == (1, 1, 0, 2)
    n_res = int(fx["param_nInternalUnits"])
    gen = dl.code_generator(fx)
    for j, b, kk_pilot, ebno in dl.blocks(fx):
        pre = f"p{j}_b{b}_"
        rng = global_rng(dl.rng_state(fx, pre + "state"))
        taps = of.flat_taps(cfg, rng)
        close(taps, fx[pre + "taps"], pre + "taps")
        assert abs(abs(taps[0, 0, 0]) - 1) < 1e-15
        pf = ob.flat_pilot(cfg, ebno, fx[pre + "taps"], rng)
        for got, key in ((pf["X_p"], "X_pilot"), (pf["x_cp"], "pilot_x"), (pf["y_cp"], "pilot_y")):
            close(got, fx[pre + key], pre + key)
        h_est = ob.flat_ls_estimate(cfg, ebno, fx[pre + "X_pilot"], fx[pre + "pilot_y"])
        close(h_est, fx[pre + "H_est"], pre + "H_est")
        assert dl.same_state(np.random.get_state(), dl.rng_state(fx, pre + "esn0_state"))
        esn = eo.OracleESN(2, 2, n_res, random_state=rng, **esn_kwargs(cfg, ebno))
        y, x = fx[pre + "pilot_y"], fx[pre + "pilot_x"]
        esn.fit(np.column_stack([y.real, y.imag]), np.column_stack([x.real, x.imag]))
        h = fx[pre + "taps"][0, 0, 0]
        check_conditioning(esn, 0, pre + "esn0")
        for kk in dl.frames_of(fx, j, b):
            fp = f"p{j}_f{kk}_"
            tx_bits = dl.bits(fx, fp + "bits")
            rng = global_rng(dl.rng_state(fx, fp + "state"))
            u = rng.randint(0, 2, size=(gen.shape[1],), dtype=np.int8)
            np.testing.assert_array_equal((gen @ u) % 2, tx_bits)
            _, x_cp, x_pa = of.modulate(tx_bits.astype(np.int32).reshape(-1, 1), cfg, ebno)
            close(x_cp[:, 0], fx[fp + "x_cp"], fp + "x_cp")
            close(of.channel(x_pa, fx[pre + "taps"], cfg, rng)[:, 0], fx[fp + "y_cp"], fp + "y_cp")
            assert dl.same_state(np.random.get_state(), dl.rng_state(fx, fp + "predict0_state"))
            y_cp = fx[fp + "y_cp"]
            global_rng(dl.rng_state(fx, fp + "predict0_state"))
            out = esn.predict(np.column_stack([y_cp.real, y_cp.imag]))          # continuation=True, transient 0
            nop = cfg.no / cfg.p_i(ebno)
            xh = {"X_hat_ESN": eo.time_to_freq([out[:, 0] + 1j * out[:, 1]], cfg.n_sub, cfg.p_i(ebno))[:, 0],
                  "X_hat_MMSE": ob.flat_detect(cfg, ebno, h, y_cp, nop),
                  "X_hat_ZF": ob.flat_detect(cfg, ebno, h, y_cp, 0.0),
                  "X_hat_LS": ob.flat_detect(cfg, ebno, fx[pre + "H_est"], y_cp, 0.0)}
            for name, xv in xh.items():
                close(xv, fx[fp + name], fp + name)
            check_counters(fx, "siso", fp, cfg, tx_bits, xh)
