"""Jakes fading inside a coherence block (esn_gen_taps_doppler, LinkParams.fading = "jakes") on the device.

  * kernel against the closed-form restatement tests/doppler_ref.py with supplied angles: |taps - ref| <= 1e-10
    absolute (the taps have unit mean link energy; a phasor drifts at most about s * 7e-16 over s <= 400
    multiplications and a tap sums at most sqrt(M) sum_p sqrt(P_p) < 16 in magnitude: about 5e-12);
  * bitwise properties of the device's own draws: a block is a function of (seed, global block) and a symbol of
    (seed, global link, s), whatever the launch holds; fd_tsym = 0 is static;
  * the statistics of tests/test_doppler_reference_cpu.py on the device's own draws, same bounds;
  * through FrameSource.blocks_fast and DetectorSweep.run: frames are those of a hand call on taps_sym, counters do not
    depend on chunking or on symbol_counts, the per-symbol counts sum to the totals, fading = "block" is untouched;
  * aging is visible: the late data symbols of a block have a higher BER than the first ones."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import doppler_ref as dr  # noqa: E402

pytestmark = pytest.mark.gpu

FS, DS_NS = 2 * 1.024e6, 300.0
TOL = 1e-10


def _device_taps(kind, n_blocks, n_sym, n_r, n_t, isi, fd_tsym, angles=None, seed=1, link_offset=0):
    import torch
    from esn_ofdm_mimo_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:%d" % torch.cuda.current_device())
    out = torch.full((n_blocks, n_sym, n_r, n_t, isi), float("nan"), dtype=torch.complex128, device=dev)
    ang = None if angles is None else torch.as_tensor(angles, dtype=torch.float64, device=dev).contiguous()
    _lib.check(lib.esn_gen_taps_doppler(kind, n_blocks, n_sym, n_r, n_t, isi, FS, DS_NS, float(fd_tsym), _lib.ptr(ang),
                                        seed, link_offset, _lib.ptr(out), _lib.stream_handle()), "esn_gen_taps_doppler")
    return out


# every size of every axis the kernel's indexing depends on (antennas, blocks, symbols, Doppler) at least once and in
# mixed company: odd block counts, an odd link count (67 x 1: half a wave idle), many workgroups (67 x 32 links), one
# symbol, and 400 symbols for the drift of the recurrence
SHAPES = [  # n_t, n_r, n_blocks, n_sym, fd_tsym
    (1, 1, 1, 1, 0.0), (1, 1, 3, 2, 0.00659), (1, 1, 67, 77, 0.05),
    (2, 2, 1, 77, 0.05), (2, 2, 3, 2, 0.0), (2, 2, 67, 77, 0.00659),
    (4, 8, 1, 77, 0.00659), (4, 8, 3, 77, 0.0), (4, 8, 67, 2, 0.05),
    (2, 2, 3, 400, 0.05),
]


@pytest.mark.parametrize("kind,isi", [(0, 8), (1, 8), (1, 1)])
@pytest.mark.parametrize("n_t,n_r,n_blocks,n_sym,fd_tsym", SHAPES)
def test_kernel_matches_the_closed_form(kind, isi, n_t, n_r, n_blocks, n_sym, fd_tsym):
    n_links = n_blocks * n_r * n_t
    rs = np.random.RandomState(1000 * kind + 100 * isi + n_links + n_sym)
    ang = dr.draw_angles(rs, n_links, kind, isi)
    got = _device_taps(kind, n_blocks, n_sym, n_r, n_t, isi, fd_tsym, angles=ang).cpu().numpy()
    assert np.isfinite(got.view(np.float64)).all()                    # every element was written
    got = got.reshape(n_blocks, n_sym, n_r * n_t, isi).transpose(0, 2, 1, 3).reshape(n_links, n_sym, isi)
    worst = 0.0
    for l0 in range(0, n_links, 256):                                 # (bounds the restatement's memory)
        ref = dr.taps(kind, ang[l0:l0 + 256], isi, fd_tsym, np.arange(n_sym), FS, DS_NS)
        worst = max(worst, np.abs(got[l0:l0 + 256] - ref).max())
    print(f"kind {kind} isi {isi} {n_r}x{n_t} blocks {n_blocks} symbols {n_sym} fd_tsym {fd_tsym}: "
          f"max |taps - ref| = {worst:.3e}")
    assert worst <= TOL, worst
    if kind == 0:
        np.testing.assert_allclose(np.sum(np.abs(got[:, 0]) ** 2, axis=-1), 1.0, rtol=0, atol=1e-12)


@pytest.mark.parametrize("kind", [0, 1])
def test_blocks_and_symbols_do_not_depend_on_the_launch(kind):
    import torch
    args = dict(n_r=2, n_t=2, isi=8, fd_tsym=0.00659)
    lpb = 4
    full = _device_taps(kind, 16, 77, seed=11, **args)
    part = _device_taps(kind, 5, 77, seed=11, link_offset=5 * lpb, **args)
    assert torch.equal(part, full[5:10])                              # blocks 5..9 alone == that slice of 0..15
    short = _device_taps(kind, 16, 10, seed=11, **args)
    assert torch.equal(short, full[:, :10])                           # a symbol does not depend on how many follow
    for b in (0, 3, 15):                                              # a block alone == itself inside any batch
        assert torch.equal(_device_taps(kind, 1, 77, seed=11, link_offset=b * lpb, **args)[0], full[b])
    assert torch.equal(_device_taps(kind, 3, 77, seed=11, link_offset=13 * lpb, **args), full[13:16])
    other = _device_taps(kind, 16, 77, seed=12, **args)
    assert not torch.equal(other, full)
    assert (other[..., 0] - full[..., 0]).abs().min().item() > 0.0    # no first tap in common
    static = _device_taps(kind, 16, 77, seed=11, **dict(args, fd_tsym=0.0))
    assert torch.equal(static, static[:, :1].expand_as(static))      # fd_tsym = 0: every symbol IS symbol 0
    assert torch.equal(static[:, 0], full[:, 0])                      # and symbol 0 does not depend on fd_tsym
    assert not torch.equal(full[:, 1], full[:, 0])


def test_device_draws_have_the_jakes_autocorrelation_and_the_pdp():
    import torch
    symbols = (0, 10, 20, 38, 60, 76)
    t = _device_taps(1, 4096, 77, 2, 2, 8, 0.01, seed=20261018)
    h = t[:, torch.tensor(symbols, device=t.device)].cpu().numpy()    # [4096, 6, 2, 2, 8]
    h = h.reshape(4096, len(symbols), 4, 8).transpose(0, 2, 1, 3).reshape(4096 * 4, len(symbols), 8)
    dr.check_statistics(h, 8, 0.01, symbols)
    # the angles are uniform: no path leans to one side of the Doppler spectrum (mean rotation ~ 0)
    rot = np.mean(h[:, 1] * np.conj(h[:, 0]), axis=0) / np.mean(np.abs(h[:, 0]) ** 2, axis=0)
    assert np.abs(rot.imag).max() <= dr.ACF_TOL


# ---- through the layers -------------------------------------------------------------------------------------------
G, F, N_RES, FD_TSYM = 24, 40, 64, 0.0096          # J0(2 pi 0.0096 s) crosses zero near s = 40
EBNOS = [12.0, 30.0]
# BER of data symbols 30..39 over BER of data symbols 0..3 at 30 dB, and what the NumPy chain gives for it
# (oracle/esn_oracle.py: train_mimo_esn + detect_frame per frame with draw_reservoir's weights, run on the CPU on the
# pilot and data frames the device generated for the very workload of the test: the same taps_sym, bits and noise).
#   * the configuration above (N = 64, N_res = 64, state noise 0.001): oracle 1.231.  Its pilot gives 64 rows for 68
#     read-out columns, the BER is 0.39 already on the first data symbol of a STATIC channel, so no fd_tsym can show a
#     factor 3 (0.5 / 0.39 bounds it; fd_tsym = 0.03 gives 1.27 on the CPU).
#   * the same with N = 128 and no state noise (AGING): oracle 3.933 (BER 0.126 -> 0.495); with state noise 0.001 it is
#     2.197, the noise floor of the first symbols hides the aging.
# The device must show at least half of the oracle's ratio.
ORACLE_RATIO_SMALL, ORACLE_AGING_RATIO = 1.231, 3.933
AGING = dict(n_sub=128, noise=0.0)
EARLY, LATE = slice(0, 4), slice(30, 40)


def _params(n_sub=64, **kw):
    from esn_ofdm_mimo_amd.montecarlo import LinkParams
    p = LinkParams.block_fading(2, 2, n_sub=n_sub)
    f_d = FD_TSYM * p.fs / (p.n_sub + p.cp)
    return dataclasses.replace(p, coherence_fixed=F, f_d=f_d, **kw)


def _sweep(params, **kw):
    from esn_ofdm_mimo_amd.montecarlo import DetectorSweep
    return DetectorSweep(params, n_reservoir=N_RES, precision="f64", fit_precision="f64", seed=5, **kw)


def _print_curve(sc, oracle):
    print("BER per data symbol at 30 dB:", np.round(sc[:, 0] / sc[:, 1], 4).tolist())
    print(f"aging ratio BER[30..39] / BER[0..3] = {aging_ratio(sc):.3f} (NumPy chain on the same frames: {oracle})")


def aging_ratio(counts):
    """counts int64 [F, 2] (errors, bits) per data symbol -> BER(LATE) / BER(EARLY); an error-free head counts as one
    error (the ratio is then a lower bound)."""
    early = max(int(counts[EARLY, 0].sum()), 1) / int(counts[EARLY, 1].sum())
    late = int(counts[LATE, 0].sum()) / int(counts[LATE, 1].sum())
    return late / early


@pytest.fixture(scope="module")
def jakes_run():
    sw = _sweep(_params(fading="jakes"), symbol_counts=True)
    ber, counters = sw.run(EBNOS, G, chunk_blocks=G)
    return sw, ber, counters


def test_params_select_the_mode():
    p = _params(fading="jakes")
    assert p.fading == "jakes" and abs(p.fd_tsym - FD_TSYM) < 1e-15 and p.coherence_symbols == F
    assert _params().fading == "block"


def test_frames_are_those_of_a_hand_call_on_the_symbol_taps():
    import torch
    from esn_ofdm_mimo_amd.montecarlo import FrameSource
    p = _params(fading="jakes")
    src = FrameSource(p, seed=5)
    d = src.blocks_fast(30.0, 1, 3, G, F, with_ls_pilot=True)
    ts = d["taps_sym"]
    assert tuple(ts.shape) == (G, 1 + F, p.n_r, p.n_t, p.isi)
    assert torch.equal(ts, src.taps_doppler(G, 1 + F, 1, 3))
    assert torch.equal(d["taps"], ts[:, 0])
    flat = ts[:, 1:].reshape(G * F, p.n_r, p.n_t, p.isi).contiguous()
    bits, _, dy = src.frames(flat, 1, 30.0, 1, 3 * F, 1)
    assert torch.equal(d["data_y"], dy) and torch.equal(d["data_bits"], bits)
    pbits, px, py = src.frames(ts[:, 0].contiguous(), 1, 30.0, 1, 3, 0, want_x=True)
    assert torch.equal(d["pilot_y"], py) and torch.equal(d["pilot_x"], px) and torch.equal(d["pilot_bits"], pbits)
    _, _, py_ls = src.frames(ts[:, 0].contiguous(), 1, 30.0, 1, 3, 0, ls_pattern=True)
    assert torch.equal(d["pilot_y_ls"], py_ls)
    # the channel really moves: the last data frame is not the one the pilot's taps would have given
    _, _, dy_static = src.frames(d["taps"], F, 30.0, 1, 3 * F, 1)
    assert not torch.equal(dy_static, dy)
    # bits, transmit signal and noise are those of block fading for the same seed: the difference of the two received
    # frames is the difference of the channels alone, and a block-mode source draws the same bits
    blk = FrameSource(_params(), seed=5).blocks_fast(30.0, 1, 3, G, F)
    assert torch.equal(blk["data_bits"], d["data_bits"]) and torch.equal(blk["pilot_bits"], d["pilot_bits"])
    assert "taps_sym" not in blk
    # blocks() (any subset of blocks) goes the same way
    sub = src.blocks(30.0, 1, [4, 5, 9], F)
    assert torch.equal(sub["data_y"][:2 * F], d["data_y"][F:3 * F]) and torch.equal(sub["taps_sym"][2], ts[6])


def test_counters_do_not_depend_on_chunking_or_symbol_counts(jakes_run):
    sw, ber, counters = jakes_run
    assert counters[:, 1].tolist() == [G * F * 64 * 4 * 2] * len(EBNOS)
    for chunk in (7, 1):
        _, c = _sweep(_params(fading="jakes"), symbol_counts=True).run(EBNOS, G, chunk_blocks=chunk)
        assert np.array_equal(c, counters), chunk
    plain = _sweep(_params(fading="jakes"))
    _, c = plain.run(EBNOS, G, chunk_blocks=7)
    assert np.array_equal(c, counters) and plain.symbol_error_counts == {}
    for si, ebno in enumerate(EBNOS):
        sc = sw.symbol_error_counts[ebno]
        assert sc.shape == (F, 2) and sc.dtype == np.int64
        assert sc.sum(axis=0).tolist() == counters[si].tolist()
        assert np.all(sc[:, 1] == G * 64 * 4 * 2)
    # two ranks: the counters add up to the single-rank ones, the per-symbol counts to the single-rank per-symbol ones
    parts = [_sweep(_params(fading="jakes"), symbol_counts=True, rank=r, world_size=2) for r in range(2)]
    cs = [s.run(EBNOS, G, chunk_blocks=5)[1] for s in parts]
    assert np.array_equal(cs[0] + cs[1], counters)
    for ebno in EBNOS:
        assert np.array_equal(parts[0].symbol_error_counts[ebno] + parts[1].symbol_error_counts[ebno],
                              sw.symbol_error_counts[ebno])


def test_block_mode_is_untouched_by_the_new_field(jakes_run):
    from esn_ofdm_mimo_amd.montecarlo import LinkParams
    base = LinkParams.block_fading(2, 2, n_sub=64)                    # built without the new field
    base.coherence_fixed, base.f_d = F, _params().f_d
    _, want = _sweep(base).run(EBNOS, G, chunk_blocks=G)
    sw = _sweep(_params(fading="block"), symbol_counts=True)
    _, got = sw.run(EBNOS, G, chunk_blocks=7)
    assert np.array_equal(got, want)
    assert sw.symbol_error_counts[EBNOS[1]].sum(axis=0).tolist() == want[1].tolist()
    assert not np.array_equal(jakes_run[2], want)                     # and "jakes" is another channel


def test_aging_is_visible():
    """N = 128, no state noise: the NumPy chain gives 3.933 on the same frames; measured on an MI355X: 3.933 (the same
    error count on every one of the 40 symbols); block fading on the same sweep: 0.979."""
    sw = _sweep(_params(AGING["n_sub"], fading="jakes"), noise=AGING["noise"], symbol_counts=True)
    sw.run([30.0], G, chunk_blocks=G)
    sc = sw.symbol_error_counts[30.0]
    _print_curve(sc, ORACLE_AGING_RATIO)
    assert ORACLE_AGING_RATIO >= 3.0
    assert aging_ratio(sc) >= 0.5 * ORACLE_AGING_RATIO, aging_ratio(sc)
    # and it is the Doppler that ages the read-out: under block fading the same sweep shows none
    blk = _sweep(_params(AGING["n_sub"]), noise=AGING["noise"], symbol_counts=True)
    blk.run([30.0], G, chunk_blocks=G)
    flat = aging_ratio(blk.symbol_error_counts[30.0])
    print(f"block fading: ratio {flat:.3f}")
    assert flat < 0.5 * ORACLE_AGING_RATIO


def test_aging_at_the_small_configuration(jakes_run):
    """N = 64, N_res = 64, state noise 0.001 (the configuration of the tests above): the NumPy chain gives 1.231 on the
    same frames, measured on an MI355X: 1.213 -- the read-out is too poor on its first symbol (BER 0.39) to age by a
    factor 3 at any Doppler; the device is held to half of the oracle's ratio all the same."""
    sc = jakes_run[0].symbol_error_counts[30.0]
    _print_curve(sc, ORACLE_RATIO_SMALL)
    assert aging_ratio(sc) >= 0.5 * ORACLE_RATIO_SMALL


def test_python_argument_errors():
    from esn_ofdm_mimo_amd.montecarlo import LinkParams, block_fading_point, coded_ber_point
    sw = _sweep(_params(fading="jakes"))
    for fn in (block_fading_point, coded_ber_point):        # they draw one tap set per block themselves
        with pytest.raises(ValueError, match="block-fading frames only"):
            fn(sw, None, 12.0, 0, 2)
    with pytest.raises(ValueError, match="fading"):
        LinkParams(fading="doppler")
    with pytest.raises(ValueError, match="awgn"):
        LinkParams(channel="awgn", fading="jakes")
    with pytest.raises(ValueError, match="awgn"):
        dataclasses.replace(LinkParams.siso_awgn(), fading="jakes")
