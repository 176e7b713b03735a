"""The reference side of tests/test_gpu_link_shapes.py, without a GPU:

  * oracle.baselines.pilot_frames at cp = 0 (isi = 1): frames of length N, one noise draw shared by the pilot and its LS
    companion, and a flat noiseless pilot estimated back to the tap's spectrum.  (The cp > 0 outputs are held bytewise to
    the drivers' own loop by tests/test_oracle_driver_loop.py.)
  * the two conditions that keep the device's exact error counts honest, on every counted shape: each reference X_hat stays
    MARGIN_MIN = 1e-7 of the frame's max|X_hat| clear of every slicer boundary (100 x the X_hat bound, so a device value
    inside its bound decides the same bits), and cond(H_k^H H_k + lambda I) < 1e4 on every subcarrier.
  * sensitivity: NumPy restatements of the kernels' steps (tests/link_shapes_ref.py) agree with the oracle inside each
    leg's bound, and each mutant of them -- the ways these kernels could be subtly wrong at ragged shapes -- is more than
    100 x the bound away on at least one shape of the list, so the GPU module would fail on such a kernel.

Every test prints its figures (pytest -s)."""
import math

import numpy as np
import pytest

import link_shapes_ref as ls
from oracle import esn_oracle as eo
from oracle.baselines import estimate_channel, pilot_frames
from oracle.ofdm_frames import LinkConfig, random_bits


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


# ---- pilot_frames at cp = 0 ---------------------------------------------------------------------------------------------
def test_pilot_frames_without_prefix_has_frames_of_length_n_and_shared_noise():
    cfg = LinkConfig(n_t=2, n_r=2, n_sub=16, m=4, isi=1)
    assert cfg.cp == 0
    taps = ls.exp_pdp_taps(cfg, np.random.RandomState(3))
    p = pilot_frames(cfg, ls.EBNO, taps, np.random.RandomState(4))
    assert p["x_cp"].shape == (16, 2) and p["y_cp"].shape == (16, 2) and p["y_ls_cp"].shape == (16, 2)
    # the draws replayed: bits, then per receive antenna randn(T) real and randn(T) imaginary, once for both frames
    rs = np.random.RandomState(4)
    bits = random_bits(cfg, rs)
    np.testing.assert_array_equal(p["bits"], bits)
    noise = np.stack([rs.randn(16) + 1j * rs.randn(16) for _ in range(cfg.n_r)], axis=1)
    for key, pattern in (("y_cp", False), ("y_ls_cp", True)):
        x_cp, y = ls.generator_reference(cfg, ls.EBNO, bits, taps, noise, ls_pattern=pattern)
        np.testing.assert_array_equal(p[key], y)                     # the same statements: bytewise
        if not pattern:
            np.testing.assert_array_equal(p["x_cp"], x_cp)
    # off its comb the LS companion is silent
    assert np.count_nonzero(p["X_LS"]) == 16 and np.all(p["X_LS"][1::2, 0] == 0) and np.all(p["X_LS"][0::2, 1] == 0)


def test_ls_pattern_reference_is_pilot_frames_companion_with_a_prefix():
    """generator_reference(ls_pattern=True), what the GPU module holds the generator's sparse pattern to, is bytewise the
    y_ls_cp of pilot_frames on the same draws at cp > 0 as well (n_t = 3, N = 64: combs of 22 / 21 / 21)."""
    cfg = ls.config(ls.Case(3, 5, 64, 6, 3))
    taps = ls.exp_pdp_taps(cfg, np.random.RandomState(5))
    p = pilot_frames(cfg, ls.EBNO, taps, np.random.RandomState(6))
    rs = np.random.RandomState(6)
    bits = random_bits(cfg, rs)
    t = cfg.n_sub + cfg.cp
    noise = np.stack([rs.randn(t) + 1j * rs.randn(t) for _ in range(cfg.n_r)], axis=1)
    for key, pattern in (("y_cp", False), ("y_ls_cp", True)):
        np.testing.assert_array_equal(p[key], ls.generator_reference(cfg, ls.EBNO, bits, taps, noise, pattern)[1])
    assert [np.count_nonzero(p["X_LS"][:, tx]) for tx in range(3)] == [22, 21, 21]


def test_noiseless_flat_pilot_without_prefix_estimates_the_taps_spectrum():
    """isi = 1: one tap per link, cp = 0 (the tc = 1e-12 prior: r_h = [1]).  Far below the PA's clip level and at an
    Eb/No of 300 dB (the noise is 1e-15 of the signal, the shrinkage 1 / (1 + 1e-31) is 1) both estimates are the tap
    itself on every subcarrier."""
    ebno = 300.0
    cfg = LinkConfig(n_t=2, n_r=3, n_sub=16, m=4, isi=1, clip_db=200.0)
    rs = np.random.RandomState(8)
    taps = ls.exp_pdp_taps(cfg, rs)
    p = pilot_frames(cfg, ebno, taps, rs)
    assert p["y_ls_cp"].shape == (16, 3)
    want = np.broadcast_to(taps[None, :, :, 0], (16, 3, 2))
    h_ls = estimate_channel(cfg, ebno, p["X_LS"], p["y_ls_cp"], ls_only=True)
    h = estimate_channel(cfg, ebno, p["X_LS"], p["y_ls_cp"])
    print("flat noiseless pilot: H_LS", _rel(h_ls, want), " H_MMSE", _rel(h, want))
    # 1e-12: the noise is sqrt(T No) / (sqrt(Pi) N) ~ 1e-15 of the signal, the PA's compression (|x| / A)^2 / 2 ~ 1e-20 and
    # the 1e-12 guard of the LS division 1e-24 of sqrt(Pi); the rest is float64 round-off
    assert _rel(h_ls, want) < 1e-12 and _rel(h, want) < 1e-12


# ---- margin and conditioning --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ls.MARGIN_CASES, ids=str)
def test_counted_references_keep_their_slicer_margin_and_conditioning(case):
    b = ls.link_blocks(case)
    cfg = b["cfg"]
    legs = [("MMSE on the estimate", b["H"], False, ls.mmse_lambda(cfg))]
    if case.n_r >= case.n_t:
        legs.append(("ZF on the true H", b["H_true"], True, 1e-12))
    for name, H, zf, lam in legs:
        x, _ = ls.detect_reference(cfg, H, b["data_y"], b["data_bits"], zf)
        margin, cond = ls.slicer_margin(x, cfg.m), ls.worst_cond(H, lam)
        print(f"{case}  {name}: margin {margin.min():.2e} (per frame {' '.join(f'{v:.1e}' for v in margin)})  "
              f"worst cond {cond:.1f}")
        assert margin.min() >= ls.MARGIN_MIN, (name, margin)
        assert cond < ls.COND_MAX, (name, cond)


# ---- sensitivity --------------------------------------------------------------------------------------------------------
def _gen_distances(mutant):
    """Per leg-A case: max over frames of |restated y - reference y| / max|y|, in units of the generator bound."""
    out = {}
    for case in ls.GEN_CASES:
        g = ls.gen_inputs(case)
        worst = 0.0
        for f in range(ls.G * ls.F):
            args = (g["cfg"], ls.EBNO, g["bits"][f], g["taps"][f // ls.F], g["noise"][f])
            x_ref, y_ref = ls.generator_reference(*args)
            x, y = ls.generator_restated(*args, mutant=mutant)
            worst = max(worst, _rel(y, y_ref), _rel(x, x_ref))
        out[case] = worst / ls.GEN_BOUND
    return out


def _est_distances(mutant, ls_only):
    out = {}
    for case in ls.EST_CASES:
        b = ls.link_blocks(case)
        ref = b["H_ls"] if ls_only else b["H"]
        out[case] = max(_rel(ls.estimate_restated(b["cfg"], ls.EBNO, b["X_LS"][g], b["y_ls_cp"][g], ls_only, mutant),
                             ref[g]) for g in range(ls.G)) / ls.H_BOUND
    return out


def _show(title, dist):
    print(title + ": " + "  ".join(f"{c} {d:.3g}" for c, d in dist.items()))


def test_restatements_agree_with_the_oracle_inside_the_bounds():
    gen, est, est_ls = _gen_distances(None), _est_distances(None, False), _est_distances(None, True)
    _show("generator restated / bound", gen)
    _show("estimate restated / bound", est)
    _show("LS estimate restated / bound", est_ls)
    assert max(gen.values()) < 1 and max(est.values()) < 1 and max(est_ls.values()) < 1
    for case in ls.DET_CASES[:4]:
        b = ls.link_blocks(case)
        x, _ = ls.detect_reference(b["cfg"], b["H"], b["data_y"], b["data_bits"], False)
        const = eo.unit_qam(case.m)
        for xf in x:
            np.testing.assert_array_equal(ls.slice_restated(xf, case.m), eo.hard_bits(xf, const, case.m))


@pytest.mark.parametrize("mutant", ["circular", "dup_rx"])
def test_generator_shapes_tell_the_mutant_from_the_oracle(mutant):
    dist = _gen_distances(mutant)
    _show(f"generator mutant {mutant} / bound", dist)
    assert max(dist.values()) > 100
    if mutant == "dup_rx":                      # only a last receive group with dead slots can show it
        assert all((d > 100) == (c.n_r % 4 != 0) for c, d in dist.items())


@pytest.mark.parametrize("mutant", ["short_comb", "held_tail", "prior_isi"])
def test_estimator_shapes_tell_the_mutant_from_the_oracle(mutant):
    est, est_ls = _est_distances(mutant, False), _est_distances(mutant, True)
    _show(f"estimate mutant {mutant} / bound", est)
    _show(f"LS estimate mutant {mutant} / bound", est_ls)
    assert max(est.values()) > 100
    if mutant == "short_comb":                  # seen where n_t does not divide N, and only there
        assert all((d > 100) == (c.n_sub % c.n_t != 0) for c, d in est.items())
        assert max(est_ls.values()) > 100
    if mutant == "held_tail":                   # every comb of n_t > 1 ends before N - 1 for some tx
        assert all((d > 100) == (c.n_t > 1) for c, d in est_ls.items())
    if mutant == "prior_isi":                   # the one shape with cp + 1 != isi
        assert [c for c, d in est.items() if d > 100] == [c for c in ls.EST_CASES if c.cp is not None]


def test_count_shapes_tell_a_truncating_slicer_from_the_oracle():
    """The counters' bound is exact equality: any differing count is beyond it."""
    worst = {}
    for case in ls.DET_CASES:
        b = ls.link_blocks(case)
        x, errs = ls.detect_reference(b["cfg"], b["H"], b["data_y"], b["data_bits"], False)
        got = np.zeros_like(errs)
        for i, xf in enumerate(x):
            got[i // ls.F] += eo.count_bit_errors(b["data_bits"][i], ls.slice_restated(xf, case.m, "truncate"))
        worst[case] = int(np.abs(got - errs).max())
    _show("truncating slicer: error count off by", worst)
    assert all(d > 0 for d in worst.values())


def test_lds_figures_of_the_shape_tables():
    """The byte counts the shape tables are chosen by."""
    assert ls.gen_lds_bytes(ls.Case(4, 8, 1024, 4, 8)) == 143808 <= ls.LDS_MAX
    assert ls.gen_lds_bytes(ls.Case(2, 4, 2048, 4, 8)) == 148704 <= ls.LDS_MAX
    assert ls.gen_lds_bytes(ls.GEN_REJECTED) == 283072 > ls.LDS_MAX
    assert ls.est_lds_bytes(ls.Case(4, 8, 2048, 4, 8)) == 90256 <= ls.LDS_MAX
    assert max(ls.est_lds_bytes(c) for c in ls.EST_CASES) <= ls.LDS_MAX
    assert ls.det_lds_bytes(ls.DET_REJECTED) == 278528 > ls.LDS_MAX
    assert ls.det_lds_bytes(ls.Case(4, 4, 2048, 4, 8)) == 147456 <= ls.LDS_MAX
    assert all(ls.det_lds_bytes(c) <= ls.LDS_MAX and c.n_t <= ls.MMSE_NT for c in ls.DET_CASES)
    n_t, n_r, n, isi, blocks = ls.TAPS_BIG
    assert blocks * n * n_r * n_t == 16842752 and blocks * n * n_r * n_t - 65535 * 256 == 65792
