"""Several pilots per coherence block through every layer: FrameSource.blocks_fast(n_pilots=),
ReservoirBank.fit_pilots, DetectorSweep(n_pilots=).  The method is that of tests/test_gpu_tracking.py: the NumPy
restatement (tests/multipilot_ref.py) is fed the device's own frames and extended states.

W_out bound.  The ridge tests grant a Cholesky solution 1e-7 of max|W| (tests/test_gpu_ridge.py: TOL["chol"]) on inputs
of cond(E) ~ 1e3; for worse conditioned fits the rule of tests/test_gpu_tracking.py applies, 10 cond^2 2^-52 for the
normal equations, with cond taken on the reference's own stacked matrix -- augmented by sqrt(lambda) I, which is the
matrix a ridge solve factorises: W_BOUND = max(1e-7, 10 cond([E; sqrt(lambda) I])^2 2^-52), printed.  Choices are
compared where the reference's two best scores are further apart than twice what that W bound and the summation order
(multipilot_ref.score_bound) can move a score."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multipilot_ref as ref  # noqa: E402
import tracking_ref  # noqa: E402
from oracle import esn_oracle as eo  # noqa: E402

pytestmark = pytest.mark.gpu

G, F, P, N_RES, EBNO, SEED = 3, 6, 3, 32, 21.0, 5
GRID = ref.GRID


def _params(n_sub=64, frames=F, fading="block", m=2):
    from esn_ofdm_mimo_amd.montecarlo import LinkParams
    p = dataclasses.replace(LinkParams.block_fading(2, 2, n_sub=n_sub), m=m, coherence_fixed=frames)
    if fading == "jakes":
        p = dataclasses.replace(p, f_d=0.01 * p.fs / (p.n_sub + p.cp), fading="jakes")
    return p


def _sweep(params=None, n_res=N_RES, noise=0.0, precision="f64", fit_precision="f64", **kw):
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep
    return DetectorSweep(params or _params(), n_reservoir=n_res, precision=precision, fit_precision=fit_precision,
                         seed=SEED, noise=noise, **kw)


# ---- n_pilots = 1 is today's path -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(ridge=1e-3), dict(ridge_grid=GRID)], ids=["pinv", "ridge", "loo"])
def test_one_pilot_is_the_old_sweep(kw):
    a = _sweep(noise=0.001, precision="f32", **kw)
    b = _sweep(noise=0.001, precision="f32", n_pilots=1, **kw)
    _, ca = a.run([EBNO, 9.0], 5, chunk_blocks=3)
    _, cb = b.run([EBNO, 9.0], 5, chunk_blocks=3)
    assert np.array_equal(ca, cb) and int(ca[:, 0].sum()) > 0
    assert a.bank.W_out.cpu().numpy().tobytes() == b.bank.W_out.cpu().numpy().tobytes()


# ---- the frames -----------------------------------------------------------------------------------------------------------
def test_pilot_zero_is_todays_pilot_and_pilots_do_not_depend_on_chunking():
    import torch
    src = _sweep().src
    one = src.blocks_fast(EBNO, 1, 2, 6, F, with_ls_pilot=True)
    many = src.blocks_fast(EBNO, 1, 2, 6, F, with_ls_pilot=True, n_pilots=3)
    for k in one:                                               # every key of today, bytewise
        assert torch.equal(one[k], many[k]), k
    p = src.p
    assert tuple(many["pilots_y"].shape) == (6, 3, p.t_frame, p.n_r)
    assert tuple(many["pilots_x"].shape) == (6, 3, p.t_frame, p.n_t)
    assert tuple(many["pilots_bits"].shape) == (6, 3, p.n_sub * p.m, p.n_t)
    for k1, k3 in (("pilot_y", "pilots_y"), ("pilot_x", "pilots_x"), ("pilot_bits", "pilots_bits"),
                   ("pilot_y_ls", "pilots_y_ls")):
        assert torch.equal(many[k3][:, 0], one[k1]), k1
    for q in range(3):
        for r in range(q):
            assert not torch.equal(many["pilots_bits"][:, q], many["pilots_bits"][:, r])
    parts = [src.blocks_fast(EBNO, 1, 2, 2, F, with_ls_pilot=True, n_pilots=3),
             src.blocks_fast(EBNO, 1, 4, 4, F, with_ls_pilot=True, n_pilots=3)]
    for k in ("pilots_y", "pilots_x", "pilots_bits", "pilots_y_ls", "data_y"):
        assert torch.equal(torch.cat([d[k] for d in parts]), many[k]), k
    picked = src.blocks(EBNO, 1, [7, 2, 3], F, n_pilots=3)       # any subset, any order
    assert torch.equal(picked["pilots_y"], many["pilots_y"][[5, 0, 1]])
    other = src.blocks_fast(EBNO, 2, 2, 6, F, n_pilots=3)        # another Eb/No index: other pilots
    assert not torch.equal(other["pilots_bits"][:, 1], many["pilots_bits"][:, 1])


def test_under_jakes_pilot_p_passes_through_symbol_p():
    import torch
    src = _sweep(_params(fading="jakes")).src
    d = src.blocks_fast(EBNO, 0, 1, 4, F, n_pilots=3, with_ls_pilot=True)
    p = src.p
    assert tuple(d["taps_sym"].shape) == (4, 3 + F, p.n_r, p.n_t, p.isi)
    assert torch.equal(d["taps"], d["taps_sym"][:, 0])
    for q in range(3):
        sid = 0 if q == 0 else 1 + q
        bits, x, y = src.frames(d["taps_sym"][:, q].contiguous(), 1, EBNO, 0, 1, sid, want_x=True)
        assert torch.equal(y, d["pilots_y"][:, q]) and torch.equal(x, d["pilots_x"][:, q])
        assert torch.equal(bits, d["pilots_bits"][:, q])
    _, _, dy = src.frames(d["taps_sym"][:, 3:].reshape(4 * F, p.n_r, p.n_t, p.isi), 1, EBNO, 0, 1 * F, 1)
    assert torch.equal(dy, d["data_y"])


# ---- fit_pilots against the restatement, on the device's own frames and states --------------------------------------
@pytest.fixture(scope="module")
def fitted():
    sw = _sweep(ridge_grid=GRID, n_pilots=P)
    data = sw.src.blocks_fast(EBNO, 0, 0, G, F, n_pilots=P)
    sw.set_snr(EBNO, G)
    E = sw.train_pilots(data["pilots_y"], data["pilots_x"], snr_idx=0, group_offset=0)
    p, bank = sw.p, sw.bank
    rows = p.t_frame + p.delay - p.forget
    E_all, D_all = E.cpu().numpy(), bank.fit_rows[1].cpu().numpy()
    assert E_all.shape == (G, P * rows, N_RES + 2 * p.n_r) and D_all.shape == (G, P * rows, 2 * p.n_t)
    host = dict(p=p, rows=rows, E=E_all, Ds=D_all * p.teacher_scale, W_out=bank.W_out.cpu().numpy(),
                choice=bank.last_ridge_choice.cpu().numpy(), scores=bank.last_ridge_scores.cpu().numpy(),
                lam=bank.last_ridge_lambda.cpu().numpy(), status=bank.fit_status.cpu().numpy(),
                fit_ridge=bank.fit_ridge.cpu().numpy(), weights=tuple(w[0].cpu().numpy() for w in bank.weights),
                data_y=data["data_y"].cpu().numpy().reshape(G, F, p.t_frame, p.n_r),
                data_bits=data["data_bits"].cpu().numpy().reshape(G, F, p.n_sub * p.m, p.n_t))
    want = []
    for g in range(G):
        Es = [host["E"][g, q * rows:(q + 1) * rows] for q in range(P)]
        Dss = [host["Ds"][g, q * rows:(q + 1) * rows] for q in range(P)]
        want.append(ref.fit_pilots(Es, Dss, grid=GRID))
    host["want"] = want
    return host


def _w_bound(E, lam):
    aug = np.vstack([E, np.sqrt(lam) * np.eye(E.shape[1])])
    return max(1e-7, 10 * np.linalg.cond(aug) ** 2 * 2.0 ** -52)


def test_fit_pilots_against_the_restatement(fitted):
    h, rows = fitted, fitted["rows"]
    assert not h["status"].any()
    compared = 0
    for g in range(G):
        w = h["want"][g]
        E_fit, D_fit = h["E"][g, :(P - 1) * rows], h["Ds"][g, :(P - 1) * rows]
        E_val, D_val = h["E"][g, (P - 1) * rows:], h["Ds"][g, (P - 1) * rows:]
        # how far a candidate's score may move: its W within the solve's bound, then the summation order
        W = np.stack([ref.ridge(E_fit, D_fit, lam) for lam in GRID])
        move = np.zeros(len(GRID))
        for l, lam in enumerate(GRID):
            dw = _w_bound(E_fit, lam) * np.abs(W[l]).max()
            dr = np.sqrt(W.shape[1] * np.sum(np.abs(E_val).sum(axis=1) ** 2)) * dw
            move[l] = 2 * np.sqrt(w["scores"][l]) * dr + dr * dr
        move += ref.score_bound(E_val, D_val, W)
        err = np.abs(h["scores"][g] - w["scores"])
        two = np.sort(w["scores"])[:2]
        clear = two[1] - two[0] > 2 * move.max()
        print(f"g={g}: scores device {h['scores'][g]} reference {w['scores']}; |diff| / allowed max "
              f"{(err / move).max():.3e}; choice {h['choice'][g]} (reference {w['choice']}, gap clear: {clear})")
        assert np.all(err <= move), (g, err, move)
        if clear:
            compared += 1
            assert h["choice"][g] == w["choice"]
        lam = GRID[h["choice"][g]]
        assert h["lam"][g] == lam == h["fit_ridge"][g]
        want_w = ref.ridge(h["E"][g], h["Ds"][g], lam)
        bound = _w_bound(h["E"][g], lam)
        rel = np.abs(h["W_out"][g] - want_w).max() / np.abs(want_w).max()
        print(f"    W_out rel err {rel:.3e}, bound {bound:.3e} (lambda {lam:g})")
        assert rel <= bound, (g, rel, bound)
    assert compared >= 1


def test_the_sweep_counts_what_the_restatement_counts_block_by_block(fitted):
    h, p = fitted, fitted["p"]
    want, margins = [], []
    for g in range(G):
        esn = eo.OracleESN(2 * p.n_r, 2 * p.n_t, N_RES, noise=0.0, input_scaling=p.input_scaling(EBNO) * np.ones(2 * p.n_r),
                           teacher_scaling=p.teacher_scale * np.ones(2 * p.n_t), random_state=1, weights=h["weights"])
        lam = GRID[h["choice"][g]]                               # (the device's choice: compared above where clear)
        esn.W_out = ref.ridge(h["E"][g], h["Ds"][g], lam)
        errs, xs = 0, []
        for k in range(F):
            x_hat, bits = eo.detect_frame(esn, h["data_y"][g, k], np.full(2 * p.n_t, p.delay), p.delay, p.delay, p.forget,
                                          p.n_sub, p.n_t, p.p_i(EBNO), eo.unit_qam(p.m), p.m)
            errs += eo.count_bit_errors(h["data_bits"][g, k].astype(int), bits)
            xs.append(x_hat)
        want.append(errs)
        margins.append(tracking_ref.boundary_margin(np.stack(xs), p.m))
    got = []
    for g in range(G):
        sw = _sweep(ridge_grid=GRID, n_pilots=P, rank=g, world_size=G)
        _, c = sw.run([EBNO], G)
        assert int(c[0, 1]) == F * p.n_sub * p.m * p.n_t
        assert int(sw.ridge_choice_counts[EBNO][h["choice"][g]]) == 1 and int(sw.ridge_choice_counts[EBNO].sum()) == 1
        got.append(int(c[0, 0]))
    print(f"errors per block: sweep {got}, restatement {want}; margins to a decision boundary {margins}")
    assert got == want


# ---- invariance ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(ridge_grid=GRID), dict(ridge=1e-3, reservoirs="fresh")], ids=["grid", "ridge_fresh"])
def test_counters_do_not_depend_on_chunking_or_world_size(kw):
    blocks = 6
    kw = dict(kw, noise=0.001, n_pilots=P, precision="f32")
    sw = _sweep(**kw)
    _, want = sw.run([EBNO, 12.0], blocks, chunk_blocks=blocks)
    assert int(want[:, 0].sum()) > 0 and sw.fits_repaired == 0
    picks = dict(sw.ridge_choice_counts)
    for chunk in (1, 4):
        s2 = _sweep(**kw)
        _, c = s2.run([EBNO, 12.0], blocks, chunk_blocks=chunk)
        assert np.array_equal(c, want), chunk
        for e in picks:
            assert np.array_equal(s2.ridge_choice_counts[e], picks[e]) and int(picks[e].sum()) == blocks
    parts = [_sweep(rank=r, world_size=2, **kw) for r in range(2)]
    cs = [s.run([EBNO, 12.0], blocks, chunk_blocks=2)[1] for s in parts]
    assert np.array_equal(cs[0] + cs[1], want)
    for e in picks:
        assert np.array_equal(parts[0].ridge_choice_counts[e] + parts[1].ridge_choice_counts[e], picks[e])


def test_a_group_without_a_choice_is_flagged_and_repaired():
    """Every candidate negative: status 2 from the solve, so no choice -- status 1, W_out zero, and resolve_failed
    leaves the QR solve's verdict (status 2: no finite candidate to fall back to)."""
    import torch
    sw = _sweep(n_pilots=2)
    data = sw.src.blocks_fast(EBNO, 0, 0, 2, F, n_pilots=2)
    sw.set_snr(EBNO, 2)
    p, d = sw.p, sw.p.delay
    U = torch.zeros((2, 2, p.t_frame + d, 2 * p.n_r), dtype=torch.float64, device="cuda")
    D = torch.zeros((2, 2, p.t_frame + d, 2 * p.n_t), dtype=torch.float64, device="cuda")
    from esn_ofdm_mimo_amd.frames import complex_as_io
    U[:, :, :p.t_frame] = complex_as_io(data["pilots_y"])
    D[:, :, d:] = complex_as_io(data["pilots_x"])
    grid = np.array([[1e-3, 1e-2], [-1.0, -2.0]])
    E = sw.bank.fit_pilots(U, D, transient=p.forget, method="auto", ridge_grid=grid)
    assert sw.bank.last_ridge_choice.cpu().tolist()[1] == -1 and sw.bank.last_ridge_choice.cpu().tolist()[0] >= 0
    assert sw.bank.fit_status.cpu().tolist() == [0, 1]
    assert not sw.bank.W_out[1].any() and bool(sw.bank.W_out[0].any())
    assert np.isnan(float(sw.bank.last_ridge_lambda[1]))
    n = sw.bank.resolve_failed(E, sw.bank.fit_rows[1], 0, sw.bank.W_out, sw.bank.fit_status, ridge_grid=grid)
    assert n == 1 and sw.bank.fit_status.cpu().tolist() == [0, 2]
    ok_grid = np.array([[1e-3, 1e-2], [-1.0, 1e-2]])
    E = sw.bank.fit_pilots(U, D, transient=p.forget, method="auto", ridge_grid=ok_grid)
    assert sw.bank.last_ridge_choice.cpu().tolist()[1] == 1 and not sw.bank.fit_status.any()


# ---- the finding, on the device ---------------------------------------------------------------------------------------
def test_four_pilots_with_the_holdout_choice_beat_one_pilot_and_beat_pinv():
    """4x8 TDL-B, N = 128, 16-QAM, N_res = 512, fp16 fit and predict, 21 dB, 8 blocks x 12 data frames.  On the CPU
    oracle (6 blocks) the three BERs are 0.019 / 0.158 / 0.339: orderings 8x and 17x apart."""
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep, LinkParams
    kw = dict(n_reservoir=512, seed=0, precision="f16", fit_precision="f16")
    ber = {}
    for key, more in ((("P1", "pinv"), dict()), (("P4", "grid"), dict(n_pilots=4, ridge_grid=GRID)),
                      (("P4", "pinv"), dict(n_pilots=4))):
        sw = DetectorSweep(LinkParams(), **kw, **more)
        b, c = sw.run([21.0], 8, frames_per_block=12)
        assert int(c[0, 1]) == 8 * 12 * 128 * 4 * 4 and sw.fits_repaired == 0
        ber[key] = float(b[0])
        if "ridge_grid" in more:
            print("picks", sw.ridge_choice_counts[21.0])
            assert int(sw.ridge_choice_counts[21.0].sum()) == 8
    print({" ".join(k): round(v, 5) for k, v in ber.items()})
    assert ber["P4", "grid"] < ber["P1", "pinv"]
    assert ber["P4", "pinv"] > ber["P4", "grid"]
