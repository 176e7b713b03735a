"""Reservoir ensembles on the device: ensemble.EnsembleBank against the NumPy ensemble (tests/ensemble_ref.py), and
montecarlo.ensemble_point anchored to DetectorSweep -- one member is that sweep bit for bit -- with its keys: counters
independent of chunking, members independent of each other, and the one-pilot gain the feature is for."""
import numpy as np
import pytest

import ensemble_ref as er
from oracle import esn_oracle as eo
from oracle.ofdm_frames import LinkConfig, make_frame, tdlb_mimo_taps

pytestmark = pytest.mark.gpu


def rel_err(got, want):
    return float(np.max(np.abs(got - want)) / (np.max(np.abs(want)) + 1e-300))


@pytest.fixture(scope="module")
def mc():
    from esn_ofdm_mimo_amd import montecarlo
    return montecarlo


# ---- against the oracle: 2x2, N = 32, QPSK, float64, no state noise, K = 3, 2 blocks x 3 frames
EBNO, K, BLOCKS, FRAMES = 12.0, 3, 2, 3


def _oracle_case(n_res):
    cfg = LinkConfig(n_t=2, n_r=2, n_sub=32, m=2)
    n_in, n_out = 2 * cfg.n_r, 2 * cfg.n_t
    rs = np.random.RandomState(100 + n_res)
    weights = [eo.draw_weights(rs, n_in, n_out, n_res, 0.9, 0.1) for _ in range(K)]
    d = (cfg.min_delay + cfg.max_delay) // 2
    forget = d + cfg.cp
    kw = dict(spectral_radius=0.9, sparsity=0.1, noise=0.0, input_scaling=cfg.input_scaling(EBNO) * np.ones(n_in),
              input_shift=np.zeros(n_in), teacher_scaling=cfg.teacher_scale * np.ones(n_out), teacher_shift=np.zeros(n_out))
    U, D, W_out, data_u, bits, Y, ext = [], [], [], [], [], [], []
    for b in range(BLOCKS):
        taps = tdlb_mimo_taps(cfg, 50 + b)
        pilot = make_frame(cfg, EBNO, taps, rs)
        x_in, x_out = eo.pack_delay_io(pilot["y_cp"], pilot["x_cp"], d, cfg.n_sub, cfg.cp, cfg.n_t, cfg.n_r)
        ens = er.OracleEnsemble(K, n_in, n_out, n_res, rs, weights=weights, **kw)
        ens.fit(x_in, x_out, forget)
        U.append(x_in)
        D.append(x_out)
        W_out.append(np.stack([m.W_out for m in ens.members]))
        for _ in range(FRAMES):
            fr = make_frame(cfg, EBNO, taps, rs)
            u = eo.pack_rx(fr["y_cp"], d)
            data_u.append(u)
            bits.append(fr["bits"])
            Y.append(ens.predict(u, forget))
        ext.append([m._ext_states[forget:] for m in ens.members])
    Y = np.stack(Y, axis=1)                                  # [K, B, N, 2 n_t]
    p_i = np.full(BLOCKS, cfg.p_i(EBNO))
    err, nb, xh = er.detect_ensemble(Y, p_i, np.stack(bits), FRAMES, cfg.m)
    return dict(cfg=cfg, weights=weights, U=np.stack(U), D=np.stack(D), W_out=np.stack(W_out, axis=1), forget=forget,
                data_u=np.stack(data_u), bits=np.stack(bits).astype(np.uint8), Y=Y, p_i=p_i, err=err, nb=nb, xh=xh,
                ext=ext)


@pytest.mark.parametrize("n_res", [20, 40])
def test_ensemble_bank_against_the_numpy_ensemble(n_res):
    """N_res = 20: 32 rows against 24 columns; N_res = 40: 44 columns, the under-determined fit the ensemble is for.
    Tolerances are those of tests/test_gpu_parity.py for float64: the read-out through its action on the reference's
    extended states 1e-7, outputs 1e-8, both relative to the largest expected magnitude; error counts exact."""
    from esn_ofdm_mimo_amd.batched import ReservoirBank
    from esn_ofdm_mimo_amd.ensemble import EnsembleBank
    c = _oracle_case(n_res)
    cfg = c["cfg"]
    n_in, n_out = 2 * cfg.n_r, 2 * cfg.n_t
    ens = EnsembleBank([ReservoirBank(n_in, n_out, n_res, *w, noise=0.0) for w in c["weights"]])
    ens.set_scaling(np.full((BLOCKS, n_in), cfg.input_scaling(EBNO)), None, np.full((BLOCKS, n_out), cfg.teacher_scale), None)
    ens.fit(c["U"], c["D"], transient=c["forget"], precision="f64", noise_mode="none", method="qr")
    st = ens.fit_status.cpu().numpy()
    assert st.shape == (K, BLOCKS) and not st.any()
    W = ens.W_out.cpu().numpy()
    assert W.shape == c["W_out"].shape == (K, BLOCKS, n_out, n_res + n_in)
    for k in range(K):
        for b in range(BLOCKS):
            ext = c["ext"][b][k]
            e = rel_err(ext @ W[k, b].T, ext @ c["W_out"][k, b].T)
            print("member", k, "block", b, "W_out action", e)
            assert e < 1e-7
    Y = ens.predict(c["data_u"], FRAMES, transient=c["forget"], precision="f64", noise_mode="none")
    assert tuple(Y.shape) == c["Y"].shape
    e = rel_err(Y.cpu().numpy(), c["Y"])
    print("Y", e)
    assert e < 1e-8
    err, nb, me, xh = ens.detect_count(Y, c["bits"], c["p_i"], FRAMES, cfg.n_sub, cfg.n_t, cfg.m,
                                       want_member_counts=True, want_xhat=True)
    print("errors", err.cpu().numpy(), "of", nb.cpu().numpy(), "members", me.cpu().numpy().tolist(), "oracle", c["err"])
    assert np.array_equal(err.cpu().numpy(), c["err"]) and np.array_equal(nb.cpu().numpy(), c["nb"])
    assert rel_err(xh.cpu().numpy(), c["xh"]) < 1e-8
    for k in range(K):
        ek, _, _ = er.detect(c["Y"][k], c["p_i"], c["bits"], FRAMES, cfg.m)
        assert np.array_equal(me.cpu().numpy()[:, k], ek)


# ---- the anchor: one member is the DetectorSweep of the same seed
SMALL = dict(n_t=2, n_r=2, n_sub=64, m=2)


@pytest.mark.parametrize("reservoirs", ["shared", "fresh"])
def test_one_member_is_the_detector_sweep_bitwise(mc, reservoirs):
    p = mc.LinkParams(**SMALL)
    kw = dict(n_reservoir=64, precision="f16", fit_precision="f64", reservoirs=reservoirs)
    _, want = mc.DetectorSweep(p, seed=11, solve_method="auto", **kw).run([15.0], 3, frames_per_block=4)
    src = mc.FrameSource(p, seed=11)
    err, nb = mc.ensemble_point(src, 15.0, 0, 3, n_members=1, frames_per_block=4, **kw)
    got = np.array([int(err.sum()), int(nb.sum())])
    print(reservoirs, "sweep", want[0], "ensemble of one", got)
    assert nb.shape == (3,) and want[0, 1] == 3 * 4 * 64 * 2 * 2 and 0 < want[0, 0]
    assert np.array_equal(got, want[0])


def test_counters_do_not_depend_on_chunking_or_first_block(mc):
    p = mc.LinkParams(**SMALL)
    src = mc.FrameSource(p, seed=3)
    kw = dict(n_members=2, n_reservoir=64, precision="f16", frames_per_block=4, reservoirs="per_block", pool=2,
              member_counts=True)
    whole = [t.cpu().numpy() for t in mc.ensemble_point(src, 12.0, 1, 4, **kw)]
    ones = [t.cpu().numpy() for t in mc.ensemble_point(src, 12.0, 1, 4, chunk_blocks=1, **kw)]
    lo = [t.cpu().numpy() for t in mc.ensemble_point(src, 12.0, 1, 2, **kw)]
    hi = [t.cpu().numpy() for t in mc.ensemble_point(src, 12.0, 1, 2, first_block=2, **kw)]
    assert whole[0].shape == (4,) and whole[2].shape == (4, 2) and whole[0].sum() > 0
    for a, b, l, h in zip(whole, ones, lo, hi):
        assert np.array_equal(a, b)
        assert np.array_equal(a, np.concatenate([l, h]))


def test_members_differ_and_each_is_reproducible_alone(mc):
    """Slab 1 of a two-member bank is what member 1, built on its own from its keys, writes."""
    import torch
    from esn_ofdm_mimo_amd.batched import ReservoirBank
    from esn_ofdm_mimo_amd.ensemble import EnsembleBank
    from esn_ofdm_mimo_amd.points import MEMBER_SEED_STRIDE
    p = mc.LinkParams(**SMALL)
    src = mc.FrameSource(p, seed=5)
    n_in, n_out, n, F, g = 2 * p.n_r, 2 * p.n_t, 64, 3, 2
    data = src.blocks_fast(15.0, 0, 0, g, F)
    d, t = p.delay, p.t_frame
    U = torch.zeros((g, t + d, n_in), dtype=torch.float64, device=src.device)
    D = torch.zeros((g, t + d, n_out), dtype=torch.float64, device=src.device)
    U[:, :t] = mc._view_real(data["pilot_y"])
    D[:, d:d + t] = mc._view_real(data["pilot_x"])
    scal = (np.full((g, n_in), p.input_scaling(15.0)), None, np.full((g, n_out), p.teacher_scale), None)
    seeds = [[mc.stream_seed(5, 0, leg + (k << 24)) for k in range(2)] for leg in (0, 1)]

    def bank(k):
        return ReservoirBank(n_in, n_out, n, *mc.draw_reservoir(n_in, n_out, n, 0.9, 0.1, 5 * 7919 + 17 + MEMBER_SEED_STRIDE * k),
                             noise=0.001, device=src.device)

    def run(ens, sd):
        ens.set_scaling(*scal)
        ens.fit(U, D, transient=p.forget, precision="f64", seed=sd[0], method="qr")
        return ens.predict(mc._view_real(data["data_y"]), F, T=t + d, transient=p.forget, precision="f16", seed=sd[1])

    both = run(EnsembleBank([bank(0), bank(1)]), seeds)
    alone = run(EnsembleBank([bank(1)]), [[seeds[0][1]], [seeds[1][1]]])
    assert tuple(both.shape) == (2, g * F, p.n_sub, n_out)
    assert not torch.equal(both[0], both[1])
    assert torch.equal(both[1], alone[0])


def test_four_small_reservoirs_beat_one_of_equal_flops_at_one_pilot(mc):
    """4x8, N = 128, 16-QAM, 21 dB, ridge 1e-3, 8 blocks x 10 frames: (K = 4, N_res = 256) against (K = 1, N_res = 512).
    The device's frames are not the oracle's, so this is statistical; the margin is that of
    tests/test_ensemble_reference_cpu.py (ratio 0.63 there, standard error 0.003 on each BER, bound 0.8)."""
    src = mc.FrameSource(mc.LinkParams(), seed=2)
    kw = dict(ridge=1e-3, frames_per_block=10, precision="f32", fit_precision="f64")
    e1, n1 = mc.ensemble_point(src, 21.0, 0, 8, n_members=1, n_reservoir=512, **kw)
    e4, n4 = mc.ensemble_point(src, 21.0, 0, 8, n_members=4, n_reservoir=256, **kw)
    single, ens = float(e1.sum()) / float(n1.sum()), float(e4.sum()) / float(n4.sum())
    print("single 512: %.4f   four 256: %.4f   ratio %.3f" % (single, ens, ens / single))
    assert int(n1.sum()) == int(n4.sum()) == 8 * 10 * 128 * 4 * 4
    assert ens <= 0.8 * single


def test_resolve_failed_leaves_clean_fits_alone_and_repairs_a_flagged_one(mc):
    """EnsembleBank.resolve_failed after a Cholesky fit: 0 on clean fits, read-outs untouched; a member's group marked
    flagged (status 1, read-out zeroed) is solved again by QR at its lambda and comes back within the float64 tolerance
    of the Cholesky solution it replaces (1e-7 through its action on the states, as in tests/test_gpu_parity.py)."""
    import torch
    from esn_ofdm_mimo_amd.batched import ReservoirBank
    from esn_ofdm_mimo_amd.ensemble import EnsembleBank
    p = mc.LinkParams(**SMALL)
    src = mc.FrameSource(p, seed=6)
    n_in, n_out, n, g = 2 * p.n_r, 2 * p.n_t, 64, 3
    data = src.blocks_fast(15.0, 0, 0, g, 1)
    d, t = p.delay, p.t_frame
    U = torch.zeros((g, t + d, n_in), dtype=torch.float64, device=src.device)
    D = torch.zeros((g, t + d, n_out), dtype=torch.float64, device=src.device)
    U[:, :t] = mc._view_real(data["pilot_y"])
    D[:, d:d + t] = mc._view_real(data["pilot_x"])
    ens = EnsembleBank([ReservoirBank(n_in, n_out, n, *mc.draw_reservoir(n_in, n_out, n, 0.9, 0.1, 40 + k), noise=0.0,
                                      device=src.device) for k in range(2)])
    ens.set_scaling(np.full((g, n_in), p.input_scaling(15.0)), None, np.full((g, n_out), p.teacher_scale), None)
    Es = ens.fit(U, D, transient=p.forget, precision="f64", noise_mode="none", method="chol", ridge=1e-3)
    assert not ens.fit_status.cpu().numpy().any()
    W0 = ens.W_out.clone()
    assert ens.resolve_failed(Es) == 0 and torch.equal(ens.W_out, W0)
    m = ens.members[1]
    m.fit_status[2] = 1
    m.W_out[2].zero_()
    assert ens.resolve_failed(Es) == 1
    assert not ens.fit_status.cpu().numpy().any()
    ext = Es[1][2, p.forget:].cpu().numpy()
    e = rel_err(ext @ ens.W_out[1, 2].cpu().numpy().T, ext @ W0[1, 2].cpu().numpy().T)
    print("repaired read-out against the Cholesky one", e)
    assert e < 1e-7
    assert torch.equal(ens.W_out[0], W0[0]) and torch.equal(ens.W_out[1, :2], W0[1, :2])
