"""(no GPU) The NumPy restatement of the SINR-weighted soft outputs (tests/soft_ref.py) against the oracle's LLRs and
against closed forms of the MMSE error share; a deep fade; the argument checks of the four new entry points
(esn_mmse_sinr, esn_qam_llr_weighted, esn_detect_llr[_f32]: plain C additions, the ABI version stays 10) from a
stand-alone C program; the LDS formula behind esn_detect_llr's -2; and the ValueErrors of
montecarlo.coded_equalized_point."""
import types

import numpy as np
import pytest

import c_abi
import equalize_ref as qr
import soft_ref as sr
from oracle import esn_oracle as eo
from oracle import ldpc_oracle as lo

P_I, NO = 3e-4, 1e-5


def _channel(rs, G, N, n_r, n_t):
    return (rs.randn(G, N, n_r, n_t) + 1j * rs.randn(G, N, n_r, n_t)) / np.sqrt(2.0)


@pytest.mark.parametrize("m,N,n_t", [(2, 16, 1), (4, 32, 2), (6, 8, 3)])
def test_unit_weights_give_the_oracles_llrs_and_sigma2_exactly(m, N, n_t):
    rs = np.random.RandomState(m + N)
    B, F = 5, 2
    X = eo.unit_qam(m)[rs.randint(0, 2 ** m, size=(B, N, n_t))] + 0.2 * (rs.randn(B, N, n_t) + 1j * rs.randn(B, N, n_t))
    ones = np.ones((3, N, n_t))
    llr, s2 = sr.llr_weighted(X, ones, ones, m, F)
    for f in range(B):
        assert s2[f] == lo.sigma2_from_decisions(X[f].reshape(-1), m)
        for i in range(n_t):
            assert np.array_equal(llr[f, i], lo.qam_llrs_maxlog(X[f, :, i], m, s2[f]).reshape(-1))
    # a weight scales its symbol's LLRs and nobody else's; the group follows the frame
    w = ones.copy()
    w[1, 3, 0] = 2.0
    llr2, s22 = sr.llr_weighted(X, w, ones, m, F)
    assert np.array_equal(s22, s2)
    d = (llr2 != llr).reshape(B, n_t, N, m)
    assert d[2:4, 0, 3].all() and d.sum() == 2 * m
    assert np.array_equal(llr2[2, 0].reshape(N, m)[3], 2.0 * llr[2, 0].reshape(N, m)[3])


def test_one_stream_has_the_matched_filter_sinr():
    rs = np.random.RandomState(1)
    H = _channel(rs, 2, 8, 3, 1)
    p_i = np.array([P_I, 2 * P_I])
    w, mu, mean = sr.sinr_weights(H, p_i, NO)
    gamma = np.sum(np.abs(H) ** 2, axis=(2, 3)) / (NO / p_i)[:, None]            # |h|^2 / lam
    assert np.allclose(w[:, :, 0] * mean[:, None], gamma, rtol=1e-12)
    assert np.allclose(mu[:, :, 0], gamma / (1.0 + gamma), rtol=1e-12)
    assert np.allclose(w.reshape(2, -1).mean(axis=1), 1.0, rtol=1e-14)


def test_orthogonal_columns_share_one_t_and_unit_weights():
    c, n_t, n_r, N = 0.7, 3, 5, 4
    H = np.zeros((1, N, n_r, n_t), dtype=np.complex128)
    H[0, :, :n_t, :] = c * np.eye(n_t)
    lam = NO / P_I
    w, mu, mean = sr.sinr_weights(H, np.array([P_I]), NO)
    assert np.allclose(1.0 - mu, lam / (c * c + lam), rtol=1e-13)
    assert np.allclose(w, 1.0, rtol=1e-13) and np.allclose(mean, c * c / lam, rtol=1e-13)


def test_weights_and_bias_do_not_change_when_h_and_lambda_scale_together():
    rs = np.random.RandomState(2)
    H = _channel(rs, 2, 8, 4, 3)
    p_i = np.array([P_I, 3 * P_I])
    w, mu, mean = sr.sinr_weights(H, p_i, NO)
    s = 4.0                                                  # a power of two: the products scale exactly
    w2, mu2, mean2 = sr.sinr_weights(s * H, p_i, s * s * NO)
    assert np.allclose(w2, w, rtol=1e-12) and np.allclose(mu2, mu, rtol=1e-12) and np.allclose(mean2, mean, rtol=1e-12)


def test_a_deep_fade_sits_at_the_upper_clamp_and_its_llrs_stay_finite_and_near_zero():
    rs = np.random.RandomState(3)
    N, n_r, n_t, m, kf = 16, 4, 2, 4, 5
    H = _channel(rs, 1, N, n_r, n_t)
    H[0, kf] *= 1e-9
    x = eo.unit_qam(m)[rs.randint(0, 2 ** m, size=(N, n_t))]
    noise = np.sqrt(NO / 2.0) * (rs.randn(N, n_r) + 1j * rs.randn(N, n_r))
    Y = np.sqrt(P_I) * np.einsum("krt,kt->kr", H[0], x) + noise
    X = qr.solve(Y, H[0], P_I, NO)[None]
    w, mu, _ = sr.sinr_weights(H, np.array([P_I]), NO)
    assert np.all(mu[0, kf] == 1.0 - sr.T_MAX) and np.all(mu[0, np.arange(N) != kf] > 0.5)
    llr, s2 = sr.llr_weighted(X, w, mu, m, 1)
    assert np.all(np.isfinite(llr)) and np.isfinite(s2[0])
    llr = llr.reshape(n_t, N, m)
    print("largest |llr| in the fade", np.abs(llr[:, kf]).max(), "median elsewhere", np.median(np.abs(np.delete(llr, kf, 1))))
    assert np.abs(llr[:, kf]).max() < 1e-3 < np.median(np.abs(np.delete(llr, kf, axis=1)))


C_SRC = r'''
#include <stdio.h>
#include <string.h>
#include <stddef.h>
#include "esn_hip.h"
static int named(const char* who, const char* what) {
    return strstr(esn_last_error(), who) != 0 && strstr(esn_last_error(), what) != 0;
}
int main(void) {
    /* never dereferenced: the checks run first */
    const double* pi = (const double*)128;
    const double* H = (const double*)256;
    const double* X = (const double*)512;
    const double* Y = (const double*)1024;
    const float* Yf = (const float*)1024;
    const uint8_t* tx = (const uint8_t*)2048;
    long long* cnt = (long long*)4096;
    double* w = (double*)8192;
    double* mu = (double*)16384;
    double* llr = (double*)32768;
    if (esn_abi_version() != 10) return 1;

    /* esn_mmse_sinr: n_t = 5, N = 12, n_r = 0, null outputs */
    if (esn_mmse_sinr(2, 128, 5, 8, pi, 1e-5, H, w, mu, 0, 0) != -1 || !named("esn_mmse_sinr", "n_t=5")) return 2;
    if (esn_mmse_sinr(2, 12, 4, 8, pi, 1e-5, H, w, mu, 0, 0) != -1 || !named("esn_mmse_sinr", "N=12")) return 3;
    if (esn_mmse_sinr(2, 4096, 4, 8, pi, 1e-5, H, w, mu, 0, 0) != -1 || !named("esn_mmse_sinr", "N=4096")) return 4;
    if (esn_mmse_sinr(2, 128, 4, 0, pi, 1e-5, H, w, mu, 0, 0) != -1 || !named("esn_mmse_sinr", "n_r=0")) return 5;
    if (esn_mmse_sinr(0, 128, 4, 8, pi, 1e-5, H, w, mu, 0, 0) != -1 || !named("esn_mmse_sinr", "n_blocks=0")) return 6;
    if (esn_mmse_sinr(2, 128, 4, 8, pi, 1e-5, H, 0, mu, 0, 0) != -1 || !named("esn_mmse_sinr", "w or mu")) return 7;
    if (esn_mmse_sinr(2, 128, 4, 8, pi, 1e-5, 0, w, mu, 0, 0) != -1 || !named("esn_mmse_sinr", "H")) return 8;

    /* esn_qam_llr_weighted */
    if (esn_qam_llr_weighted(7, 3, 128, 5, 4, X, w, mu, llr, 0, 0) != -1 || !named("esn_qam_llr_weighted", "n_t=5")) return 10;
    if (esn_qam_llr_weighted(7, 3, 128, 4, 3, X, w, mu, llr, 0, 0) != -1 || !named("esn_qam_llr_weighted", "bits_per_sym=3")) return 11;
    if (esn_qam_llr_weighted(7, 3, 12, 4, 4, X, w, mu, llr, 0, 0) != -1 || !named("esn_qam_llr_weighted", "N=12")) return 12;
    if (esn_qam_llr_weighted(7, 0, 128, 4, 4, X, w, mu, llr, 0, 0) != -1 || !named("esn_qam_llr_weighted", "frames_per_group=0")) return 13;
    if (esn_qam_llr_weighted(7, 3, 128, 4, 4, X, w, mu, 0, 0, 0) != -1 || !named("esn_qam_llr_weighted", "llr")) return 14;
    if (esn_qam_llr_weighted(7, 3, 128, 4, 4, 0, w, mu, llr, 0, 0) != -1 || !named("esn_qam_llr_weighted", "X_hat")) return 15;
    if (esn_qam_llr_weighted(0, 3, 128, 4, 4, X, w, mu, llr, 0, 0) != -1 || !named("esn_qam_llr_weighted", "n_frames=0")) return 16;

    /* esn_detect_llr */
    if (esn_detect_llr(Y, 7, 3, 128, 5, 4, pi, tx, cnt, cnt, w, mu, llr, 0, 0, 0) != -1 || !named("esn_detect_llr", "n_t=5")) return 20;
    if (esn_detect_llr(Y, 7, 3, 128, 4, 5, pi, tx, cnt, cnt, w, mu, llr, 0, 0, 0) != -1 || !named("esn_detect_llr", "bits_per_sym=5")) return 21;
    if (esn_detect_llr(Y, 7, 3, 96, 4, 4, pi, tx, cnt, cnt, w, mu, llr, 0, 0, 0) != -1 || !named("esn_detect_llr", "N=96")) return 22;
    if (esn_detect_llr(Y, 7, 0, 128, 4, 4, pi, tx, cnt, cnt, w, mu, llr, 0, 0, 0) != -1 || !named("esn_detect_llr", "frames_per_group=0")) return 23;
    if (esn_detect_llr(Y, 7, 3, 128, 4, 4, pi, tx, cnt, cnt, w, mu, 0, 0, 0, 0) != -1 || !named("esn_detect_llr", "llr")) return 24;
    if (esn_detect_llr(0, 7, 3, 128, 4, 4, pi, tx, cnt, cnt, w, mu, llr, 0, 0, 0) != -1 || !named("esn_detect_llr", "Y")) return 25;
    if (esn_detect_llr(Y, 7, 3, 128, 4, 4, pi, tx, 0, cnt, w, mu, llr, 0, 0, 0) != -1 || !named("esn_detect_llr", "tx_bits")) return 26;
    if (esn_detect_llr((const double*)1032, 7, 3, 128, 4, 4, pi, tx, cnt, cnt, w, mu, llr, 0, 0, 0) != -1 || !named("esn_detect_llr", "aligned")) return 27;

    /* esn_detect_llr_f32, under its own name */
    if (esn_detect_llr_f32(Yf, 7, 3, 128, 5, 4, pi, tx, cnt, cnt, w, mu, llr, 0, 0, 0) != -1 || !named("esn_detect_llr_f32", "n_t=5")) return 30;
    if (esn_detect_llr_f32(Yf, 7, 3, 128, 4, 7, pi, tx, cnt, cnt, w, mu, llr, 0, 0, 0) != -1 || !named("esn_detect_llr_f32", "bits_per_sym=7")) return 31;
    if (esn_detect_llr_f32(Yf, 7, 3, 3, 4, 4, pi, tx, cnt, cnt, w, mu, llr, 0, 0, 0) != -1 || !named("esn_detect_llr_f32", "N=3")) return 32;
    if (esn_detect_llr_f32(Yf, 7, 0, 128, 4, 4, pi, tx, cnt, cnt, w, mu, llr, 0, 0, 0) != -1 || !named("esn_detect_llr_f32", "frames_per_group=0")) return 33;
    if (esn_detect_llr_f32(Yf, 7, 3, 128, 4, 4, pi, tx, cnt, cnt, w, mu, 0, 0, 0, 0) != -1 || !named("esn_detect_llr_f32", "llr")) return 34;
    if (esn_detect_llr_f32((const float*)1028, 7, 3, 128, 4, 4, pi, tx, cnt, cnt, w, mu, llr, 0, 0, 0) != -1 || !named("esn_detect_llr_f32", "aligned")) return 35;

    /* the LDS of one workgroup of the fused tail: 16 (n_t (N + 1) + N/2); the largest served shape is inside 150 KiB */
    if (esn_detect_llr_lds_bytes(128, 4) != 16 * (4 * 129 + 64)) return 40;
    if (esn_detect_llr_lds_bytes(2048, 4) != 147520 || esn_detect_llr_lds_bytes(2048, 4) > 150 * 1024) return 41;
    if (esn_detect_llr_lds_bytes(2048, 5) <= 150 * 1024) return 42;
    if (esn_detect_llr_lds_bytes(0, 4) != 0) return 43;
    printf("soft abi ok\n");
    return 0;
}
'''


def test_soft_entry_points_link_from_c99_and_name_the_argument_they_refuse(tmp_path):
    r = c_abi.compile_and_run(tmp_path, "soft", C_SRC)
    assert "soft abi ok" in r.stdout


def test_binding_types_the_soft_entry_points_and_the_abi_version_stays():
    from esn_ofdm_mimo_amd import _lib
    sig = _lib.SIGNATURES
    for name, n_args in (("esn_mmse_sinr", 11), ("esn_qam_llr_weighted", 11), ("esn_detect_llr", 16),
                         ("esn_detect_llr_f32", 16), ("esn_detect_llr_lds_bytes", 2)):
        assert name in sig and len(sig[name][1]) == n_args, name
    assert _lib.ABI_VERSION == 10
    lib = _lib.load()
    assert lib.esn_abi_version() == 10
    rc = lib.esn_mmse_sinr(2, 128, 5, 8, None, 1e-5, None, None, None, None, None)
    assert rc == -1 and b"esn_mmse_sinr" in lib.esn_last_error()
    # every shape the fused tail serves fits its LDS: the -2 of esn_detect_llr cannot be reached through the checks
    for log2n in range(1, 12):
        for n_t in range(1, 5):
            assert lib.esn_detect_llr_lds_bytes(1 << log2n, n_t) <= 150 * 1024


def _stub_source(**kw):
    """What coded_equalized_point reads of a FrameSource before it touches the device."""
    from esn_ofdm_mimo_amd.link import LinkParams
    return types.SimpleNamespace(p=LinkParams(**kw), seed=0, torch=None, device=None)


def test_point_refuses_what_equalized_esn_point_refuses_and_an_unknown_llr():
    from esn_ofdm_mimo_amd import montecarlo as mc
    src, code = _stub_source(), types.SimpleNamespace(n=512, k=259)
    for kw, word in ((dict(llr="raw"), "llr"), (dict(llr=None), "llr"), (dict(cal_frac=1.0), "cal_frac"),
                     (dict(reservoirs="fresh"), "reservoirs"), (dict(method="svd"), "method"), (dict(io="f16"), "io"),
                     (dict(ridge=-1.0), "ridge"), (dict(frames_per_block=0), "frames_per_block"),
                     (dict(n_reservoir=1), "n_reservoir"), (dict(delay=-1), "delay"),
                     (dict(reservoirs="per_block", pool=0), "pool"), (dict(sparsity=1.0), "spectral radius")):
        with pytest.raises(ValueError, match=word):
            mc.coded_equalized_point(src, code, 12.0, 0, 4, **kw)
    with pytest.raises(ValueError, match="n_blocks"):
        mc.coded_equalized_point(src, code, 12.0, 0, 0)
    with pytest.raises(ValueError, match="no block to decode"):
        mc.coded_equalized_point(src, code, 12.0, 0, 1)
    with pytest.raises(ValueError, match="code's length"):
        mc.coded_equalized_point(src, types.SimpleNamespace(n=64, k=30), 12.0, 0, 4)
    with pytest.raises(ValueError, match="continuation"):
        mc.coded_equalized_point(_stub_source(continuation=True), code, 12.0, 0, 4)
    with pytest.raises(ValueError, match="n_t"):
        mc.coded_equalized_point(_stub_source(n_t=5, n_r=8), code, 12.0, 0, 4)
