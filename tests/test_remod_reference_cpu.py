"""(no GPU) The restatements behind decision-directed tracking, and what of the feature needs no device:

  * tests/remod_ref.py: for error-free decisions its D_hat IS the transmitter's pre-PA frame
    (oracle.ofdm_frames.modulate(...)[1]), delayed: 1e-12 of max, the bound the generated frames are held to;
  * tests/tracking_ref.py: with a window that covers everything and the "genie" teacher on a static channel, the last
    read-out is the single fit on the stacked true frames;
  * esn_detect_remod is exported, typed by the binding and checks its arguments before any HIP call (-1, the limit named
    in esn_last_error()); the ABI version stays 10;
  * the argument errors of DetectorSweep(track=...) and ReservoirBank.detect_remod that precede the first device call."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import remod_ref  # noqa: E402
import tracking_ref  # noqa: E402
from oracle import esn_oracle as eo  # noqa: E402
from oracle.ofdm_frames import LinkConfig, exp_pdp_taps, make_frame, modulate, random_bits  # noqa: E402


@pytest.mark.parametrize("n_sub,n_t,m,isi,delay", [(16, 1, 2, 1, 0), (32, 2, 4, 8, 3), (128, 4, 4, 8, 3), (64, 5, 6, 8, 0)])
def test_error_free_decisions_give_back_the_transmitted_frame(n_sub, n_t, m, isi, delay):
    cfg = LinkConfig(n_t=n_t, n_r=n_t, n_sub=n_sub, m=m, isi=isi)
    rs = np.random.RandomState(n_sub + n_t + m)
    ebno, B = 17.0, 3
    p_i = cfg.p_i(ebno)
    bits = np.stack([random_bits(cfg, rs) for _ in range(B)])
    mods = [modulate(b, cfg, ebno) for b in bits]
    # the frame the detector sees when the ESN is perfect: the body of the pre-PA transmit signal
    Y = np.zeros((B, n_sub, 2 * n_t))
    for f, (_, x_cp, _) in enumerate(mods):
        Y[f, :, 0::2], Y[f, :, 1::2] = x_cp[cfg.cp:].real, x_cp[cfg.cp:].imag
    out = remod_ref.detect_remod(Y, 2, n_sub, cfg.cp, delay, n_t, m, np.array([p_i, p_i]), tx_bits=bits)
    assert out["err"].tolist() == [0, 0] and out["bits"].tolist() == [2 * n_sub * m * n_t, n_sub * m * n_t]
    assert np.array_equal(out["dec_bits"], bits.astype(np.uint8))
    for f, (x_f, x_cp, _) in enumerate(mods):
        want = eo.pack_delay_io(np.zeros((n_sub + cfg.cp, n_t), dtype=complex), x_cp, delay, n_sub, cfg.cp, n_t, n_t)[1]
        assert out["D_hat"][f].shape == want.shape == (delay + cfg.cp + n_sub, 2 * n_t)
        dev = np.abs(out["D_hat"][f] - want).max()
        print(f"frame {f}: max |D_hat - modulate| = {dev:.2e} of {np.abs(want).max():.2e}")
        assert dev <= 1e-12 * np.abs(want).max()
        assert np.abs(out["X_hat"][f] - x_f).max() <= 1e-12


def test_genie_with_a_full_window_is_one_fit_on_the_stacked_true_frames():
    cfg = LinkConfig(n_t=2, n_r=2, n_sub=16, m=2, isi=8)
    ebno, F, n_res = 21.0, 4, 12
    rs = np.random.RandomState(3)
    taps = exp_pdp_taps(cfg, rs)
    frames = [make_frame(cfg, ebno, taps, rs) for _ in range(1 + F)]
    d, forget = cfg.delay, cfg.delay + cfg.cp
    w = eo.draw_weights(np.random.RandomState(5), 4, 4, n_res, 0.9, 0.1)
    kw = dict(noise=0.0, input_scaling=cfg.input_scaling(ebno) * np.ones(4), teacher_scaling=cfg.teacher_scale * np.ones(4),
              random_state=1, weights=w)
    got = tracking_ref.track_block(eo.OracleESN(4, 4, n_res, **kw), frames[0]["y_cp"], frames[0]["x_cp"],
                                   np.stack([f["y_cp"] for f in frames[1:]]), np.stack([f["bits"] for f in frames[1:]]),
                                   np.stack([f["x_cp"] for f in frames[1:]]), cfg.n_sub, cfg.cp, 2, 2, d, cfg.p_i(ebno),
                                   cfg.m, "genie", F + 1)
    one = eo.OracleESN(4, 4, n_res, **kw)
    E, D = [], []
    for f in frames[:F]:                        # the pilot and data symbols 0 .. F - 2: the last symbol is never trained on
        x_in, x_out = eo.pack_delay_io(f["y_cp"], f["x_cp"], d, cfg.n_sub, cfg.cp, 2, 2)
        one.fit(x_in, x_out, forget)
        E.append(one._ext_states[forget:])
        D.append(one.scale_teacher(x_out)[forget:])
    want = (np.linalg.pinv(np.vstack(E)) @ np.vstack(D)).T
    assert got["W_out"].shape == want.shape and len(got["cond"]) == F
    assert np.abs(got["W_out"] - want).max() <= 1e-9 * np.abs(want).max()
    # and a window of one forgets everything but the last symbol trained on
    last = tracking_ref.track_block(eo.OracleESN(4, 4, n_res, **kw), frames[0]["y_cp"], frames[0]["x_cp"],
                                    np.stack([f["y_cp"] for f in frames[1:]]), np.stack([f["bits"] for f in frames[1:]]),
                                    np.stack([f["x_cp"] for f in frames[1:]]), cfg.n_sub, cfg.cp, 2, 2, d, cfg.p_i(ebno),
                                    cfg.m, "genie", 1)
    want1 = (np.linalg.pinv(E[-1]) @ D[-1]).T
    assert np.abs(last["W_out"] - want1).max() <= 1e-9 * np.abs(want1).max()
    assert got["errors"][0] == last["errors"][0]            # symbol 0 is detected by the pilot fit either way


def test_symbol_is_exported_typed_and_checks_before_any_device_call():
    from esn_ofdm_mimo_amd import _lib, build
    build.build_library(verbose=False)
    lib = _lib.load()
    assert "esn_remod.hip" in build.SOURCES and "esn_detect.hip" in build.SOURCES
    assert _lib.ABI_VERSION == 10 and lib.esn_abi_version() == 10
    assert len(_lib.SIGNATURES["esn_detect_remod"][1]) == 16
    p = 64                                      # never dereferenced: the checks run first
    ok = dict(Y=p, B=3, F=1, N=16, cp=7, delay=3, n_t=2, m=2, p_i=p, tx=p, err=p, nb=p, xh=None, db=None, D=p)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.esn_detect_remod(a["Y"], a["B"], a["F"], a["N"], a["cp"], a["delay"], a["n_t"], a["m"], a["p_i"], a["tx"],
                                  a["err"], a["nb"], a["xh"], a["db"], a["D"], None)
        return rc, lib.esn_last_error()

    for kw, word in ((dict(Y=None), b"null"), (dict(p_i=None), b"null"), (dict(D=None), b"null"),
                     (dict(err=None), b"err_count"), (dict(nb=None), b"err_count"),
                     (dict(B=0), b"invalid sizes"), (dict(F=0), b"invalid sizes"), (dict(n_t=0), b"invalid sizes"),
                     (dict(n_t=17), b"16"), (dict(N=24), b"power of two"), (dict(N=4096), b"2048"),
                     (dict(m=3), b"even"), (dict(m=12), b"even"), (dict(cp=16), b"[0, N)"), (dict(cp=-1), b"[0, N)"),
                     (dict(delay=-1), b"delay"), (dict(delay=(1 << 20) + 1), b"delay")):
        rc, msg = call(**kw)
        assert rc == -1 and b"esn_detect_remod" in msg and word in msg, (kw, rc, msg)


def test_sweep_argument_errors_come_before_the_device():
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep, LinkParams
    p = LinkParams.block_fading(2, 2, n_sub=16)
    for kw, word in ((dict(track="directed"), "track must be"), (dict(track="genie", track_window=0), "track_window"),
                     (dict(track="decisions", ridge_grid=[1e-3, 1e-2]), "ridge_grid"),
                     (dict(track="decisions", train_ebno=12.0), "train_ebno"),
                     (dict(track="genie", io="f32", precision="f32"), "io='f32'")):
        with pytest.raises(ValueError, match=word):
            DetectorSweep(p, n_reservoir=16, **kw)
    with pytest.raises(ValueError, match="continuation"):
        DetectorSweep(dataclasses.replace(p, continuation=True), n_reservoir=16, track="decisions")
