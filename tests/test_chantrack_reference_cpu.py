"""CPU-only checks around esn_channel_track (include/esn_hip.h): the restatement tests/chantrack_ref.py builds the normal
equations it claims (the block-Toeplitz G of the lag sums is the explicit A^H A, its solution is the least-squares
solution of the stacked, regularised system, noise-free spectra give the taps back); the entry point is plain C, typed
by the binding, and returns every unserved shape and a wrong X_hat / bits pair before a device is touched; the ABI
number stays 10; baseline_tracking_point refuses its arguments before it touches its FrameSource."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import c_abi  # noqa: E402
import chantrack_ref as cr  # noqa: E402
from oracle.esn_oracle import unit_qam  # noqa: E402

EPS = 2.0 ** -52

# W, N, n_t, n_r, L, m
CASES = [(1, 16, 1, 1, 2, 2), (2, 32, 2, 3, 8, 4), (1, 128, 4, 8, 8, 4), (3, 32, 4, 8, 4, 6), (1, 64, 2, 2, 8, 2)]


def _draw(case, seed=0):
    W, N, n_t, n_r, L, m = case
    rs = np.random.RandomState(100 * N + 10 * n_t + W + seed)
    X = unit_qam(m)[rs.randint(0, 1 << m, size=(W, N, n_t))]
    taps = (rs.randn(n_r, n_t, L) + 1j * rs.randn(n_r, n_t, L)) * np.exp(-np.arange(L) / 3.0)
    Hf = np.transpose(np.fft.fft(taps, N, axis=2), (2, 0, 1))                       # [N, n_r, n_t]
    Y = np.einsum("krt,fkt->fkr", Hf, X)
    reg = 10 ** rs.uniform(-3, -1, size=L)
    return X, Y, taps, reg, rs


@pytest.mark.parametrize("case", CASES)
def test_lag_sum_gram_is_the_explicit_one(case):
    W, N, n_t, n_r, L, m = case
    X, Y, _, reg, _ = _draw(case)
    A = cr.design(X, L)
    G = cr.gram_from_lags(cr.lag_sums(X, L), reg)
    want = A.conj().T @ A + np.diag(np.tile(reg, n_t))
    assert np.abs(G - want).max() <= 64 * EPS * W * N
    assert np.abs(G - G.conj().T).max() <= 64 * EPS * W * N
    assert np.abs(cr.rhs(X, Y, L) - A.conj().T @ Y.reshape(W * N, n_r)).max() == 0


@pytest.mark.parametrize("case", CASES)
def test_solution_is_the_least_squares_solution(case):
    W, N, n_t, n_r, L, m = case
    X, Y, _, reg, rs = _draw(case)
    Y = Y + 0.05 * (rs.randn(*Y.shape) + 1j * rs.randn(*Y.shape))
    out = cr.solve_estimate(X, Y, L, reg)
    assert out["status"] == 0
    A = cr.design(X, L)
    stacked = np.vstack([A, np.diag(np.sqrt(np.tile(reg, n_t)))])
    target = np.vstack([Y.reshape(W * N, n_r), np.zeros((n_t * L, n_r))])
    want = np.linalg.lstsq(stacked, target, rcond=None)[0].T.reshape(n_r, n_t, L)
    bound = 100 * out["cond"] * EPS
    worst = np.abs(out["taps"] - want).max() / np.abs(want).max()
    print(case, "cond", out["cond"], "worst", worst, "bound", bound)
    assert worst <= bound
    Hw = np.transpose(np.fft.fft(want, N, axis=2), (2, 0, 1))
    assert np.abs(out["H"] - Hw).max() <= L * bound * np.abs(want).max()


@pytest.mark.parametrize("case", CASES)
def test_noise_free_spectra_give_the_taps_back(case):
    W, N, n_t, n_r, L, m = case
    X, Y, taps, _, _ = _draw(case)
    out = cr.solve_estimate(X, Y, L, np.zeros(L))
    assert out["status"] == 0
    assert np.abs(out["taps"] - taps).max() <= 100 * out["cond"] * EPS * np.abs(taps).max()


def test_whole_call_reads_both_decision_forms_and_flags_a_singular_estimate():
    W, N, n_t, n_r, L, m, cp = 2, 32, 2, 2, 4, 4, 3
    rs = np.random.RandomState(3)
    n_est = 3
    idx = rs.randint(0, 1 << m, size=(n_est * W, N, n_t))
    idx[W:2 * W, :, 1] = idx[W:2 * W, :, 0]                    # estimate 1: both antennas send the same symbols
    X = unit_qam(m)[idx]
    bits = ((idx[:, :, None, :] >> np.arange(m)[None, None, :, None]) & 1).reshape(n_est * W, N * m, n_t).astype(np.uint8)
    assert np.array_equal(cr.bits_to_indices(bits, m), idx)
    y = rs.randn(n_est * W, cp + N, n_r) + 1j * rs.randn(n_est * W, cp + N, n_r)
    p_i, reg0 = np.array([1e-3, 2e-3]), np.zeros((2, L))
    a = cr.channel_track(y, W, 2, cp, n_t, L, m, p_i, reg0, X_hat=X * 1.01)
    b = cr.channel_track(y, W, 2, cp, n_t, L, m, p_i, reg0, bits=bits)
    assert a["status"].tolist() == [0, 1, 0] == b["status"].tolist()
    assert np.isnan(a["H"][1]).all() and np.isnan(a["taps"][1]).all()
    for k in ("taps", "H"):
        assert np.array_equal(a[k][[0, 2]], b[k][[0, 2]])
    c = cr.channel_track(y, W, 2, cp, n_t, L, m, p_i, reg0 + 0.5, bits=bits)
    assert c["status"].tolist() == [0, 0, 0] and np.isfinite(c["H"]).all()


def test_map_reg_is_the_prior_of_the_pilot_estimator():
    from oracle import baselines
    from oracle.ofdm_frames import LinkConfig
    cfg = LinkConfig()
    p_i = cfg.p_i(21.0)
    want = (cfg.n_sub + cfg.cp) * cfg.no / (cfg.n_sub * p_i * baselines.isi_magnitude(cfg)[:cfg.isi])
    np.testing.assert_allclose(cr.map_reg(cfg.n_sub, cfg.cp, cfg.isi, cfg.no, p_i), want, rtol=1e-15)


def test_binding_types_the_entry_point_and_the_abi_number_stays():
    import ctypes as C
    from esn_ofdm_mimo_amd import _lib
    assert _lib.ABI_VERSION == 10
    res, args = _lib.SIGNATURES["esn_channel_track"]
    assert res is C.c_int and len(args) == 18
    assert args[3:12] == [C.c_int] * 9
    lib = _lib.load()
    assert lib.esn_abi_version() == 10
    assert lib.esn_channel_track.argtypes == args


# (y, X_hat, bits, n_est, W, epg, N, cp, n_t, n_r, isi, m) with pointers as 0 / 64 (never dereferenced), the word
# the message must hold; the first row is served as far as the checks go and is not in this table
GOOD = (64, 64, 0, 3, 2, 1, 128, 7, 4, 8, 8, 4)
BAD = [
    ((64, 64, 64, 3, 2, 1, 128, 7, 4, 8, 8, 4), "exactly one"), ((64, 0, 0, 3, 2, 1, 128, 7, 4, 8, 8, 4), "exactly one"),
    ((0, 64, 0, 3, 2, 1, 128, 7, 4, 8, 8, 4), "null"),
    ((64, 64, 0, 0, 2, 1, 128, 7, 4, 8, 8, 4), "invalid sizes"), ((64, 64, 0, 3, 2, 0, 128, 7, 4, 8, 8, 4), "invalid sizes"),
    ((64, 64, 0, -1, 2, 1, 128, 7, 4, 8, 8, 4), "invalid sizes"),
    ((64, 64, 0, 3, 0, 1, 128, 7, 4, 8, 8, 4), "window"), ((64, 64, 0, 3, 9, 1, 128, 7, 4, 8, 8, 4), "window"),
    ((64, 64, 0, 3, 2, 1, 96, 7, 4, 8, 8, 4), "power of two"), ((64, 64, 0, 3, 2, 1, 4096, 7, 4, 8, 8, 4), "power of two"),
    ((64, 64, 0, 3, 2, 1, 1, 0, 1, 1, 1, 2), "power of two"),
    ((64, 64, 0, 3, 2, 1, 128, 7, 5, 8, 8, 4), "n_t"), ((64, 64, 0, 3, 2, 1, 128, 7, 0, 8, 8, 4), "n_t"),
    ((64, 64, 0, 3, 2, 1, 128, 7, 4, 9, 8, 4), "n_r"), ((64, 64, 0, 3, 2, 1, 128, 7, 4, 0, 8, 4), "n_r"),
    ((64, 64, 0, 3, 2, 1, 128, 7, 4, 8, 17, 4), "isi"), ((64, 64, 0, 3, 2, 1, 128, 7, 4, 8, 0, 4), "isi"),
    ((64, 64, 0, 3, 2, 1, 16, 7, 4, 8, 8, 4), "unknowns"), ((64, 64, 0, 3, 2, 1, 8, 3, 2, 2, 8, 4), "unknowns"),
    ((64, 64, 0, 3, 2, 1, 128, 128, 4, 8, 8, 4), "cp"), ((64, 64, 0, 3, 2, 1, 128, -1, 4, 8, 8, 4), "cp"),
    ((64, 64, 0, 3, 2, 1, 128, 7, 4, 8, 8, 3), "even"), ((64, 64, 0, 3, 2, 1, 128, 7, 4, 8, 8, 12), "even"),
    ((64, 64, 0, 3, 2, 1, 128, 7, 4, 8, 8, 0), "even"),
    ((64, 64, 0, 3, 2, 1, 2048, 7, 4, 8, 8, 4), "LDS"), ((64, 64, 0, 3, 2, 1, 1024, 7, 4, 8, 8, 4), "LDS"),
    ((72, 64, 0, 3, 2, 1, 128, 7, 4, 8, 8, 4), "aligned"), ((64, 72, 0, 3, 2, 1, 128, 7, 4, 8, 8, 4), "aligned"),
]


def test_every_unserved_shape_returns_minus_one_with_a_message_from_ctypes():
    from esn_ofdm_mimo_amd import _lib
    lib = _lib.load()

    def call(row, taps=64, H=64, status=64, p_i=64, reg=64):
        y, xh, bt, *ints = row
        return lib.esn_channel_track(y or None, xh or None, bt or None, *ints, p_i or None, reg or None, taps or None,
                                     H or None, status or None, None)

    for row, word in BAD:
        assert call(row) == -1, row
        msg = lib.esn_last_error().decode()
        assert "esn_channel_track" in msg and word in msg, (row, msg)
    for kw in (dict(H=0), dict(status=0), dict(p_i=0), dict(reg=0)):
        assert call(GOOD, **kw) == -1 and "null" in lib.esn_last_error().decode(), kw
    assert call(GOOD, taps=72) == -1 and "aligned" in lib.esn_last_error().decode()
    assert call(GOOD, H=72) == -1 and "aligned" in lib.esn_last_error().decode()


C_SRC = r'''
#include <stdio.h>
#include <string.h>
#include "esn_hip.h"
static int said(const char* word) {
    return strstr(esn_last_error(), "esn_channel_track") != 0 && strstr(esn_last_error(), word) != 0;
}
static int call(long y, long xh, long bt, int n_est, int w, int epg, int n, int cp, int nt, int nr, int isi, int m) {
    /* pointers are never dereferenced: the checks run first */
    return esn_channel_track((const double*)y, (const double*)xh, (const uint8_t*)bt, n_est, w, epg, n, cp, nt, nr, isi, m,
                             (const double*)64, (const double*)64, (double*)64, (double*)64, (int*)64, 0);
}
int main(void) {
    if (esn_abi_version() != 10) return 1;
%s
    printf("chantrack abi ok\n");
    return 0;
}
'''


def test_entry_point_links_from_c99_and_validates_without_a_device(tmp_path):
    rows = "\n".join('    if (call(%s) != -1 || !said("%s")) return %d;' % (", ".join(str(v) for v in row), word, 2 + i)
                     for i, (row, word) in enumerate(BAD))
    r = c_abi.compile_and_run(tmp_path, "ct", C_SRC % rows)
    assert "chantrack abi ok" in r.stdout


def test_baseline_tracking_point_refuses_its_arguments_before_the_device():
    from esn_ofdm_mimo_amd import montecarlo, points
    assert montecarlo.baseline_tracking_point is points.baseline_tracking_point

    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError("the FrameSource was touched: " + name)

    for kw, word in ((dict(track="directed"), "track must be"), (dict(track="genie", window=0), "window"),
                     (dict(track="decisions", window=9), "window"), (dict(window=1.5), "window"),
                     (dict(n_blocks=0), "n_blocks"), (dict(first_block=-1), "first_block"),
                     (dict(chunk_blocks=0), "chunk_blocks"), (dict(frames_per_block=0), "frames_per_block")):
        args = dict(dict(ebno_db=21.0, snr_idx=0, n_blocks=2), **kw)
        with pytest.raises(ValueError, match=word):
            points.baseline_tracking_point(NoDevice(), **args)
