"""The fixed-shape instance of the detector tail (detect_count_fixed_kernel<IO32, 7, 4, 4>: N = 128, n_t = 4, 16-QAM)
against the generic kernel, which the knob detect_fixed = "0" selects for every call: err, bits and the bytes of X_hat
are equal over the sample of tools/record_detect_digests.py -- one frame; K - 1, K + 1 and 2 K + 3 frames (K = 8
frames per workgroup) in groups of 3, so several groups inside a workgroup and a ragged last one; 151 frames in groups
of 75, a group boundary inside a workgroup and a last group of one frame; one group over three workgroups; Y zero and
Y with a row of -0.0 (signed zeros through the kept trivial twiddles); counters that already hold values; tx_bits one
byte and Y eight bytes into a larger buffer (the alignment fallback); a shape the instance does not serve -- each
with float64 and float32 Y.  One case is anchored to NumPy (np.fft.fft and the same slicer rule): counts exact, X_hat
to 1e-12 of its largest magnitude, the rule of tests/test_gpu_driver_funcs.py."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_detect_digests", os.path.join(ROOT, "tools", "record_detect_digests.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

CASES = rec.cases()
IDS = [f"{i:02d}-{c['id']}" for i, c in enumerate(CASES)]
pytestmark = pytest.mark.gpu


def same_bits(a, b):
    import torch
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    n_diff = int((a.view(torch.int64) != b.view(torch.int64)).sum())
    assert n_diff == 0, f"{n_diff} of {a.numel()} elements differ"


def both(i, c, want_xhat=True):
    """case i under detect_fixed "1" and "0": {knob: (err, bits, X_hat or None)}"""
    from esn_ofdm_mimo_amd import _lib
    out = {}
    try:
        for knob in ("1", "0"):
            _lib.debug_set("detect_fixed", knob)
            out[knob] = rec.run(i, c, want_xhat)
    finally:
        _lib.debug_set("detect_fixed", "1")
    return out


def test_sample_covers_what_the_fixed_instance_can_get_wrong():
    K = rec.K
    key = {(c["kind"], c["B"], c["F"], c["n_sub"], c["n_t"], c["m"], c["y32"]) for c in CASES}
    for y32 in (False, True):
        for kind, b, f in (("one", 1, 1), ("ragged", K - 1, 3), ("ragged", K + 1, 3), ("ragged", 2 * K + 3, 3),
                           ("bound", 151, 75), ("spread", 20, 20)):
            assert (kind, b, f, 128, 4, 4, y32) in key
        for kind in ("zero", "negz", "twice", "txoff", "yoff"):
            assert (kind, K + 1, 3, 128, 4, 4, y32) in key
        assert ("other", K + 1, 3, 64, 2, 2, y32) in key
    assert 20 > 2 * K and 75 % K != 0                     # "spread" spans three workgroups, "bound" splits one


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_fixed_equals_generic(i):
    import torch
    c = CASES[i]
    out = both(i, c)
    (e1, n1, x1), (e0, n0, x0) = out["1"], out["0"]
    print(c["id"], "err", e1.tolist(), e0.tolist(), "bits", n1.tolist(), n0.tolist())
    assert torch.equal(e1, e0) and torch.equal(n1, n0)
    same_bits(x1, x0)
    groups = (c["B"] + c["F"] - 1) // c["F"]
    per_frame = c["n_sub"] * c["m"] * c["n_t"] * (2 if c["twice"] else 1)
    want_bits = [per_frame * min(c["F"], c["B"] - g * c["F"]) for g in range(groups)]
    assert n1.tolist() == want_bits
    if c["ymode"] == "randn":
        assert int(e1.sum()) > 0


@pytest.mark.parametrize("y32", (False, True), ids=("f64", "f32"))
def test_counters_accumulate(y32):
    """two calls into the same err / bits give twice the counts of one"""
    import torch
    i = next(k for k, c in enumerate(CASES) if c["kind"] == "twice" and c["y32"] == y32)
    twice = rec.run(i, CASES[i])
    once = rec.run(i, dict(CASES[i], twice=False))
    assert torch.equal(twice[0], 2 * once[0]) and torch.equal(twice[1], 2 * once[1])
    same_bits(twice[2], once[2])


@pytest.mark.parametrize("y32", (False, True), ids=("f64", "f32"))
def test_counters_without_xhat(y32):
    import torch
    i = next(k for k, c in enumerate(CASES) if c["kind"] == "ragged" and c["B"] == 2 * rec.K + 3 and c["y32"] == y32)
    with_x = rec.run(i, CASES[i], True)
    without = both(i, CASES[i], False)
    for knob in ("1", "0"):
        assert without[knob][2] is None
        assert torch.equal(without[knob][0], with_x[0]) and torch.equal(without[knob][1], with_x[1])


def test_fixed_against_numpy():
    """B = 7, F = 3 on the fixed path against np.fft.fft and the slicer rule of the reference: idx = i side + j with
    i, j = clip(rint((re, im) norm + side - 1) / 2), natural binary LSB first"""
    i = next(k for k, c in enumerate(CASES) if c["kind"] == "ragged" and c["B"] == rec.K - 1 and not c["y32"])
    c = CASES[i]
    Y, tx, p_i = rec.arrays(i, c)
    B, F, N, n_t, m = c["B"], c["F"], c["n_sub"], c["n_t"], c["m"]
    err, bits, xh = rec.run(i, c)
    side = 1 << (m // 2)
    norm = np.sqrt(2.0 * (side * side - 1) / 3.0)
    y = Y.reshape(B, N, n_t, 2)
    scale = 1.0 / (N * np.sqrt(p_i[np.arange(B) // F]))
    X = np.fft.fft(y[..., 0] + 1j * y[..., 1], axis=1) * scale[:, None, None]                 # [B, N, n_t]
    lev = lambda v: np.clip(np.rint((v * norm + (side - 1)) * 0.5), 0, side - 1).astype(np.int64)
    idx = lev(X.real) * side + lev(X.imag)
    got_bits = (idx[:, :, None, :] >> np.arange(m)[None, None, :, None]) & 1                  # [B, N, m, n_t]
    wrong = (got_bits != tx.reshape(B, N, m, n_t)).reshape(B, -1).sum(axis=1)
    groups = (B + F - 1) // F
    want_err = [int(wrong[g * F:(g + 1) * F].sum()) for g in range(groups)]
    want_bits = [N * m * n_t * min(F, B - g * F) for g in range(groups)]
    print("err", err.tolist(), want_err, "bits", bits.tolist(), want_bits)
    assert err.tolist() == want_err and bits.tolist() == want_bits
    got = xh.cpu().numpy().reshape(B, N, n_t, 2)
    d = np.abs(got[..., 0] + 1j * got[..., 1] - X).max()
    print("max |X_hat - numpy|", d, "of", np.abs(X).max())
    np.testing.assert_allclose(got[..., 0] + 1j * got[..., 1], X, rtol=0, atol=1e-12 * np.abs(X).max())
