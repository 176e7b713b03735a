"""montecarlo.equalized_esn_point on the device: against the NumPy chain (tests/equalize_ref.py) on the frames read back,
its counters' independence of chunking and of a first_block cut, its MMSE counters against
FrameSource.mmse_detect_count, and the finding the feature is for."""
import numpy as np
import pytest

import equalize_ref as qr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mc():
    from esn_ofdm_mimo_amd import montecarlo
    return montecarlo


def rel_err(got, want):
    return float(np.max(np.abs(got - want)) / (np.max(np.abs(want)) + 1e-300))


@pytest.mark.parametrize("link,seed", [(dict(), 4), (dict(n_t=2, n_r=2, n_sub=16), 9)])
def test_point_against_the_numpy_chain(mc, link, seed):
    """float64, no state noise, 2 blocks x 3 frames at 21 dB, N_res 8, ridge 1e-5: the frames, the pilot and the channel
    estimate are read back, the NumPy chain runs on them with the point's reservoir (draw_reservoir of the sweep's seed
    rule), and X_hat agrees within 1e-8 of its largest magnitude, the error counts exactly.  The counts can only be held
    equal where no decision of the chain is a near-tie: the test measures the chain's smallest distance from a slicer
    threshold and asks for 1e-5, a thousand times the X_hat bound; the seeds above are ones where it holds (measured on an
    MI355X: X_hat 4.2e-15 and 9.3e-15, margins 5.7e-4 and 4.0e-4, errors [45 73] and [84 60] on both sides)."""
    ebno, G, F, n_res, ridge = 21.0, 2, 3, 8, 1e-5
    p = mc.LinkParams(**link)
    src = mc.FrameSource(p, seed=seed)
    err, nb, xh = mc.equalized_esn_point(src, ebno, 1, G, n_reservoir=n_res, ridge=ridge, noise=0.0, precision="f64",
                                         frames_per_block=F, want_xhat=True)
    d = src.blocks_fast(ebno, 1, 0, G, F, with_ls_pilot=True)
    H = src.estimate_channel(d["pilot_bits"], d["pilot_y_ls"], ebno).cpu().numpy()
    p_i = np.full(G, p.p_i(ebno))
    _, pilot_rows = qr.equalize(d["pilot_y"].cpu().numpy(), H, p_i, p.no, p.cp, 0, 1)
    _, data_rows = qr.equalize(d["data_y"].cpu().numpy(), H, p_i, p.no, p.cp, 0, F)
    pilot_x, bits = d["pilot_x"].cpu().numpy(), d["data_bits"].cpu().numpy()
    weights = mc.draw_reservoir(2 * p.n_t, 2 * p.n_t, n_res, 0.9, 0.1, seed * 7919 + 17)
    want_x, want_err = [], np.zeros(G, dtype=np.int64)
    for b in range(G):
        esn = qr.make_esn(p.n_t, n_res, p.input_scaling(ebno), p.teacher_scale, ridge, noise=0.0, weights=weights)
        X, hard = qr.chain_block(esn, pilot_rows[b], pilot_x[b], data_rows[b * F:(b + 1) * F], p.n_sub, p.cp, 0, p_i[b], p.m)
        want_x.append(X)
        want_err[b] = sum(int(np.sum(hard[f] != bits[b * F + f])) for f in range(F))
    want_x = np.concatenate(want_x)
    margin = qr.slicer_margin(want_x, p.m)
    e = rel_err(xh.cpu().numpy(), want_x)
    print(link, "X_hat", e, "slicer margin", margin, "errors", err.cpu().numpy(), "chain", want_err)
    assert tuple(xh.shape) == (G * F, p.n_sub, p.n_t)
    assert e < 1e-8
    assert margin > 1e-5
    assert np.array_equal(err.cpu().numpy(), want_err)
    assert np.array_equal(nb.cpu().numpy(), np.full(G, F * p.n_sub * p.m * p.n_t))


def test_counters_do_not_depend_on_chunking_or_first_block_and_mmse_counters_are_the_baselines(mc):
    p = mc.LinkParams(n_t=2, n_r=2, n_sub=64)
    src = mc.FrameSource(p, seed=3)
    kw = dict(frames_per_block=3, reservoirs="per_block", pool=2, want_mmse=True)
    whole = [t.cpu().numpy() for t in mc.equalized_esn_point(src, 12.0, 1, 4, **kw)]
    ones = [t.cpu().numpy() for t in mc.equalized_esn_point(src, 12.0, 1, 4, chunk_blocks=1, **kw)]
    twos = [t.cpu().numpy() for t in mc.equalized_esn_point(src, 12.0, 1, 4, chunk_blocks=2, **kw)]
    lo = [t.cpu().numpy() for t in mc.equalized_esn_point(src, 12.0, 1, 1, **kw)]
    hi = [t.cpu().numpy() for t in mc.equalized_esn_point(src, 12.0, 1, 3, first_block=1, **kw)]
    assert len(whole) == 4 and whole[0].shape == (4,) and whole[0].sum() > 0 and whole[2].sum() > 0
    for a, b, c, l, h in zip(whole, ones, twos, lo, hi):
        assert np.array_equal(a, b) and np.array_equal(a, c)
        assert np.array_equal(a, np.concatenate([l, h]))
    assert np.array_equal(whole[1], np.full(4, 3 * 64 * 4 * 2)) and np.array_equal(whole[3], whole[1])
    d = src.blocks_fast(12.0, 1, 0, 4, 3, with_ls_pilot=True)
    H = src.estimate_channel(d["pilot_bits"], d["pilot_y_ls"], 12.0)
    e, nb = src.mmse_detect_count(H, d["data_y"], d["data_bits"], 3, 12.0)
    assert np.array_equal(whole[2], e.cpu().numpy()) and np.array_equal(whole[3], nb.cpu().numpy())
    plain = [t.cpu().numpy() for t in mc.equalized_esn_point(src, 12.0, 1, 4, frames_per_block=3, reservoirs="per_block",
                                                              pool=2)]
    assert len(plain) == 2 and np.array_equal(plain[0], whole[0])


def test_esn_behind_the_equaliser_makes_at_most_0p6_of_its_errors_on_the_device(mc):
    """4x8, TDL-B, N = 128, 16-QAM, 21 dB, the point's defaults (N_res 8, ridge 1e-5, state noise 1e-3), 16 blocks x 8
    frames: errors <= 0.6 x the LS-MMSE errors on the same frames.  The NumPy chain at this count gave 0.361, 0.380,
    0.363, 0.392 and 0.378 on five sets of blocks (tests/test_equalize_reference_cpu.py has the 12 x 6 run); the device
    gave 2859 against 7142, 0.400.  The cap is a condition, not a measurement."""
    src = mc.FrameSource(mc.LinkParams(), seed=2)
    err, nb, e_mm, n_mm = mc.equalized_esn_point(src, 21.0, 7, 16, frames_per_block=8, want_mmse=True)
    e, m = int(err.sum()), int(e_mm.sum())
    print("ESN behind the equaliser %d, LS-MMSE %d of %d bits: ratio %.3f" % (e, m, int(nb.sum()), e / m))
    assert int(nb.sum()) == int(n_mm.sum()) == 16 * 8 * 128 * 4 * 4 and m > 1000
    assert e <= 0.6 * m
