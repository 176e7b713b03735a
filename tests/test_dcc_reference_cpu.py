"""The amplifier-aware LS-MMSE detector without a GPU: the NumPy model (tests/dcc_ref.py) held to what it must do by
construction, the slicer margin that keeps the device test's exact counts honest, the C entry points' refusals from a C99
program, the binding, the ValueErrors of montecarlo.dcc_point, and the finding the device test asserts, on the oracle."""
import math
import types

import numpy as np
import pytest

import c_abi
import dcc_ref as dr


@pytest.mark.parametrize("shape", dr.SHAPES, ids=str)
def test_no_distortion_no_correction(shape):
    """An amplifier that never compresses (A = 1e30) predicts no distortion: every pass returns X^0."""
    d = dr.inputs(shape)
    _, _, _, m, cp, n_iter = shape
    for f in (0, dr.FRAMES - 1):
        q = f // dr.PER_GROUP
        xs = dr.dcc_frame(d["y"][f], d["H"][q], d["p_i"][q], 1e30, dr.NO, cp, m, max(n_iter, 2))
        worst = max(np.abs(x - xs[0]).max() for x in xs[1:])
        print(shape, f, "max |X^it - X^0|", worst)
        assert worst <= 1e-12


@pytest.mark.parametrize("shape", [s for s in dr.SHAPES if s[2] >= s[1]], ids=str)
def test_exact_distortion_is_cancelled(shape):
    """A noiseless frame through the true channel and the same amplifier, the transmitted points as decisions, lam -> 0:
    one pass restores X.  (n_r >= n_t: without noise and lam the equaliser has to invert H.)"""
    d = dr.inputs(shape)
    n, n_t, n_r, m, cp, _ = shape
    for f in (0, 3):
        q = f // dr.PER_GROUP
        X = dr.points_from_bits(d["bits"][f], n, m)
        _, x_pa = dr.transmit(X, d["p_i"][q], d["a_clip"][q], cp)
        y = dr.through_channel(x_pa, d["taps"][q])
        x0, x1 = dr.dcc_frame(y, d["H_true"][q], d["p_i"][q], d["a_clip"][q], 1e-30, cp, m, 1, decisions=X)
        print(shape, f, "before", np.abs(x0 - X).max(), "after", np.abs(x1 - X).max())
        assert np.abs(x0 - X).max() > 1e-3                  # there was something to cancel
        assert np.abs(x1 - X).max() <= 1e-9


@pytest.mark.parametrize("shape,frames", [(s, dr.FRAMES) for s in dr.SHAPES] + [(dr.BIG_SHAPE, 1)], ids=str)
def test_slicer_margin_of_every_device_case(shape, frames):
    """No coordinate of any X^{it}, it < n_iter, of the model lies within 1e-7 grid spacings of a decision boundary --
    100 x the X_hat tolerance: a kernel within tolerance cannot legitimately take another decision, and the device test
    excludes nothing."""
    a = dr.answers(shape, frames)
    print(shape, "margin", a["margin"], "err_iter", a["err_iter"].tolist())
    assert a["margin"] >= dr.MARGIN_MIN
    assert dr.lds_bytes(*shape[:3]) <= dr.LDS_MAX < dr.lds_bytes(*dr.REFUSED_SHAPE[:3])


def test_the_shapes_see_both_kinds_of_compression_and_a_changing_count():
    """Group 0 and 2 clip at 0.3 of the rms, group 1 at 3; at least one shape's error count moves from pass to pass (a
    kernel that stopped after one pass would be seen by the counters too, not by X_hat alone)."""
    d = dr.inputs(dr.SHAPES[3])
    rms = np.sqrt(d["p_i"] * dr.SHAPES[3][0])
    assert np.allclose(d["a_clip"] / rms, [0.3, 3.0, 0.3]) and len(set(d["p_i"])) == 3
    assert any(len(set(row)) > 2 for s in dr.SHAPES for row in dr.answers(s)["err_iter"].tolist())


def test_oracle_point_gains_at_least_the_factor_the_device_test_asks():
    """21 dB, 16 blocks x 8 frames of the oracle's 4x8 link, seed dr.POINT_SEED: two passes leave at most a fifth of the
    LS-MMSE detector's errors (measured 7348 -> 787 -> 211 of 262,144 bits)."""
    errs, nbits = dr.oracle_point_errors(2)
    print("errors after 0, 1, 2 passes", errs.tolist(), "of", nbits)
    assert nbits == 16 * 8 * 128 * 4 * 4
    assert errs[0] >= dr.POINT_GAIN * errs[2]


C_SRC = r'''
#include <stdio.h>
#include <string.h>
#include "esn_hip.h"
static int named(const char* what) {
    return strstr(esn_last_error(), "esn_mmse_dcc_detect_count") != 0 && strstr(esn_last_error(), what) != 0;
}
/* never dereferenced: every call below is refused before any HIP call */
static const double* pi = (const double*)128;
static const double* ac = (const double*)192;
static const double* H = (const double*)256;
static const double* y = (const double*)512;
static const uint8_t* tb = (const uint8_t*)1024;
static long long* e = (long long*)2048;
static long long* nb = (long long*)4096;
static double* xh = (double*)8192;
static int call(int n_frames, int fpg, int n, int cp, int n_t, int n_r, int m, int n_iter) {
    return esn_mmse_dcc_detect_count(n_frames, fpg, n, cp, n_t, n_r, m, n_iter, pi, ac, 1e-5, H, y, tb, e, nb, 0, xh, 0);
}
int main(void) {
    int n, n_t, n_r, served = 0, refused = 0;
    if (esn_abi_version() != 10) return 1;
    if (call(7, 3, 12, 3, 4, 8, 4, 2) != -1 || !named("power of two")) return 2;
    if (call(7, 3, 4096, 3, 1, 1, 4, 2) != -1 || !named("N=4096")) return 3;
    if (call(0, 3, 128, 7, 4, 8, 4, 2) != -1 || !named("n_frames")) return 4;
    if (call(7, 0, 128, 7, 4, 8, 4, 2) != -1 || !named("frames_per_group")) return 5;
    if (call(7, 3, 128, 128, 4, 8, 4, 2) != -1 || !named("cp=128")) return 6;
    if (call(7, 3, 128, -1, 4, 8, 4, 2) != -1 || !named("cp=-1")) return 7;
    if (call(7, 3, 128, 7, 5, 8, 4, 2) != -1 || !named("n_t=5")) return 8;
    if (call(7, 3, 128, 7, 0, 8, 4, 2) != -1 || !named("n_t=0")) return 9;
    if (call(7, 3, 128, 7, 4, 0, 4, 2) != -1 || !named("n_r=0")) return 10;
    if (call(7, 3, 128, 7, 4, 8, 3, 2) != -1 || !named("bits_per_sym=3")) return 11;
    if (call(7, 3, 128, 7, 4, 8, 12, 2) != -1 || !named("bits_per_sym=12")) return 12;
    if (call(7, 3, 128, 7, 4, 8, 0, 2) != -1 || !named("bits_per_sym=0")) return 13;
    if (call(7, 3, 128, 7, 4, 8, 4, 9) != -1 || !named("n_iter=9")) return 14;
    if (call(7, 3, 128, 7, 4, 8, 4, -1) != -1 || !named("n_iter=-1")) return 15;
    if (call(1, 1, 1024, 10, 4, 8, 4, 2) != -1 || !named("LDS") || !named("270336")) return 16;
    /* NULL arguments, each by name */
    if (esn_mmse_dcc_detect_count(7, 3, 128, 7, 4, 8, 4, 2, 0, ac, 1e-5, H, y, tb, e, nb, 0, xh, 0) != -1 || !named("p_i"))
        return 17;
    if (esn_mmse_dcc_detect_count(7, 3, 128, 7, 4, 8, 4, 2, pi, 0, 1e-5, H, y, tb, e, nb, 0, xh, 0) != -1 || !named("a_clip"))
        return 18;
    if (esn_mmse_dcc_detect_count(7, 3, 128, 7, 4, 8, 4, 2, pi, ac, 1e-5, 0, y, tb, e, nb, 0, xh, 0) != -1 || !named("H is"))
        return 19;
    if (esn_mmse_dcc_detect_count(7, 3, 128, 7, 4, 8, 4, 2, pi, ac, 1e-5, H, 0, tb, e, nb, 0, xh, 0) != -1 || !named("y_cp"))
        return 20;
    if (esn_mmse_dcc_detect_count(7, 3, 128, 7, 4, 8, 4, 2, pi, ac, 1e-5, H, y, tb, 0, nb, 0, xh, 0) != -1 ||
        !named("err_count"))
        return 21;
    if (esn_mmse_dcc_detect_count(7, 3, 128, 7, 4, 8, 4, 2, pi, ac, 1e-5, H, y, tb, e, 0, 0, xh, 0) != -1 ||
        !named("bit_count"))
        return 22;
    if (esn_mmse_dcc_detect_count(7, 3, 128, 7, 4, 8, 4, 2, pi, ac, 1e-5, H, y, 0, 0, 0, 0, 0, 0) != -1 || !named("X_hat"))
        return 23;
    /* the LDS formula over every served N and n_t and n_r up to 80: the byte count, and which side of 150 KiB the entry
       point puts the shape -- a served shape gets past the LDS check and is refused for its n_iter = 9 instead */
    for (n = 2; n <= 2048; n *= 2)
        for (n_t = 1; n_t <= 4; ++n_t)
            for (n_r = 1; n_r <= 80; ++n_r) {
                const size_t want = 16 * ((size_t)(n_r + 2 * n_t) * n + n / 2);
                if (esn_mmse_dcc_lds_bytes(n, n_t, n_r) != want) return 24;
                if (call(1, 1, n, 0, n_t, n_r, 4, 9) != -1) return 25;
                if (want > 150 * 1024) { if (!named("LDS")) return 26; ++refused; }
                else { if (!named("n_iter=9")) return 27; ++served; }
            }
    if (esn_mmse_dcc_lds_bytes(128, 4, 8) != 33792 || esn_mmse_dcc_lds_bytes(512, 4, 8) != 135168) return 28;
    if (esn_mmse_dcc_lds_bytes(0, 4, 8) != 0 || esn_mmse_dcc_lds_bytes(128, 0, 8) != 0) return 29;
    printf("dcc abi ok: %d shapes served, %d refused\n", served, refused);
    return served > 0 && refused > 0 ? 0 : 30;
}
'''


def test_dcc_entry_points_link_from_c99_and_name_what_they_refuse(tmp_path):
    r = c_abi.compile_and_run(tmp_path, "dcc", C_SRC)
    print(r.stdout)
    assert "dcc abi ok" in r.stdout


def test_binding_types_the_dcc_entry_points():
    import ctypes as C
    from esn_ofdm_mimo_amd import _lib, build
    sig = _lib.SIGNATURES
    assert len(sig["esn_mmse_dcc_detect_count"][1]) == 19 and sig["esn_mmse_dcc_detect_count"][0] is C.c_int
    assert sig["esn_mmse_dcc_lds_bytes"] == (C.c_size_t, [C.c_int] * 3)
    assert "esn_dcc.hip" in build.SOURCES
    assert _lib.ABI_VERSION == 10
    lib = _lib.load()
    assert lib.esn_mmse_dcc_lds_bytes(128, 4, 8) == dr.lds_bytes(128, 4, 8) == 33792
    rc = lib.esn_mmse_dcc_detect_count(7, 3, 128, 7, 4, 8, 4, 2, None, None, 1e-5, None, None, None, None, None, None,
                                       None, None)
    assert rc == -1 and b"esn_mmse_dcc_detect_count" in lib.esn_last_error()


def _stub_source(**kw):
    """What dcc_point reads of a FrameSource before it touches the device."""
    from esn_ofdm_mimo_amd.link import LinkParams
    return types.SimpleNamespace(p=LinkParams(**kw), seed=0, torch=None, device=None)


def test_point_refuses_what_it_does_not_serve():
    from esn_ofdm_mimo_amd import montecarlo as mc
    assert mc.dcc_point is __import__("esn_ofdm_mimo_amd.points", fromlist=["x"]).dcc_point
    src = _stub_source()
    for kw, word in ((dict(chunk_blocks=0), "chunk_blocks"), (dict(frames_per_block=0), "frames_per_block"),
                     (dict(first_block=-1), "first_block"), (dict(n_iter=9), "n_iter"), (dict(n_iter=-1), "n_iter"),
                     (dict(n_iter=2.0), "n_iter"), (dict(a_clip_db_error=math.nan), "a_clip_db_error"),
                     (dict(a_clip_db_error=math.inf), "a_clip_db_error")):
        with pytest.raises(ValueError, match=word):
            mc.dcc_point(src, 21.0, 0, 2, **kw)
    with pytest.raises(ValueError, match="n_blocks"):
        mc.dcc_point(src, 21.0, 0, 0)
    with pytest.raises(ValueError, match="n_t"):
        mc.dcc_point(_stub_source(n_t=5, n_r=8), 21.0, 0, 2)
