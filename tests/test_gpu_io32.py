"""float32 / complex64 I/O of the batched detector pipeline (esn_predict_batch_f32, esn_detect_count_f32,
esn_gen_frames_c64): every served path against its float64 sibling on the widened inputs, BITWISE -- the float32
result must be the float64 one rounded, because the kernels narrow every input to float before any arithmetic."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    import torch
    from esn_ofdm_mimo_amd import _lib, batched, montecarlo
    return torch, _lib, batched, montecarlo


def same_bits(a, b):
    import torch
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    va, vb = (a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else (a.view(torch.int64), b.view(torch.int64))
    n_diff = int((va != vb).sum())
    assert n_diff == 0, f"{n_diff} of {a.numel()} elements differ"


def make_bank(batched, n_in, n_out, n_res, G, n_wsets=1, noise=0.0, seed=0):
    """Random reservoir (row-normalised, spectral radius ~0.9 without an eigen-decomposition), scalings, read-out."""
    rs = np.random.RandomState(seed)
    W = (rs.rand(n_wsets, n_res, n_res) - 0.5) * (rs.rand(n_wsets, n_res, n_res) > 0.9)
    W *= 0.9 / np.sqrt(0.1 * n_res / 12.0)
    W_in = rs.rand(n_wsets, n_res, n_in) * 2 - 1
    W_fb = rs.rand(n_wsets, n_res, n_out) * 2 - 1
    bank = batched.ReservoirBank(n_in, n_out, n_res, W, W_in, W_fb, noise=noise)
    bank.set_scaling(0.5 + rs.rand(G, n_in), 0.1 * rs.randn(G, n_in), 1.0 + rs.rand(G, n_out), 0.1 * rs.randn(G, n_out))
    bank.set_readout(rs.randn(G, n_out, n_res + n_in) * (0.3 / np.sqrt(n_res)))
    return bank, rs


def predict_both(torch, bank, U32, F, T, transient, precision, **kw):
    y32 = bank.predict(U32, F, T=T, transient=transient, precision=precision, io="f32", **kw)
    y64 = bank.predict(U32.double(), F, T=T, transient=transient, precision=precision, **kw)
    torch.cuda.synchronize()
    assert y32.dtype == torch.float32 and y64.dtype == torch.float64
    assert torch.isfinite(y64).all()
    return y32, y64


# (name, precision, n_res, n_in, n_out, knobs): one row per kernel path esn_predict_batch takes for fp32/fp16/bf16
PATHS = [
    ("skew16_f16", "f16", 512, 16, 8, {}),
    ("skew16_bf16", "bf16", 512, 16, 8, {}),
    ("skew32x32_f16", "f16", 512, 16, 8, {"s16": "0"}),
    ("instep_f16", "f16", 512, 16, 8, {"skew": "0"}),
    ("skew16_siso_shape", "f16", 512, 2, 2, {}),          # n_in = 2: 4-byte DMA chunks in the 16x16x32 kernel
    ("skew32x32_nin2", "f16", 256, 2, 2, {}),             # ... and in the 32x32x16 skewed kernel
    ("mfma_f32_300", "f32", 300, 16, 8, {}),
    ("mfma_f16_128", "f16", 128, 16, 8, {}),
    ("big_gemm_2048", "f16", 2048, 16, 8, {}),
    ("big_persistent_2048", "f16", 2048, 16, 8, {"big_gemm": "0"}),
]
RESTORE = {"s16": "1", "skew": "1", "big_gemm": "1"}
# what esn_recur_path answers for each row ("mfma" is the in-step and the 32x32x16 skewed schedule alike)
KERNEL = {"skew16_f16": "skew16", "skew16_bf16": "skew16", "skew16_siso_shape": "skew16", "big_gemm_2048": "big_predict"}


# every path with and without counter noise; the slow 2048 shapes with counter noise only
CASES = [p + (nm,) for p in PATHS for nm in ("none", "counter") if p[2] != 2048 or nm == "counter"]


@pytest.mark.parametrize("name,precision,n_res,n_in,n_out,knobs,noise_mode", CASES,
                         ids=[f"{c[0]}-{c[-1]}" for c in CASES])
def test_predict_f32_is_rounded_f64(mods, name, precision, n_res, n_in, n_out, knobs, noise_mode):
    torch, _lib, batched, _ = mods
    G, F, T, transient = 3, 20, 40, 5
    bank, rs = make_bank(batched, n_in, n_out, n_res, G, noise=1e-3 if noise_mode == "counter" else 0.0)
    U32 = torch.tensor(rs.randn(G * F, T - 3, n_in), dtype=torch.float32, device="cuda")
    try:
        for k, v in knobs.items():
            _lib.debug_set(k, v)
        assert _lib.recur_path(False, precision, bank.shape, G * F, F) == KERNEL.get(name, "mfma")
        y32, y64 = predict_both(torch, bank, U32, F, T, transient, precision, noise_mode=noise_mode, seed=7)
    finally:
        for k in knobs:
            _lib.debug_set(k, RESTORE[k])
    same_bits(y32, y64.float())


def test_predict_f32_unaligned_u_and_tensor_noise(mods):
    """A float32 U that is a view at a 4-byte offset (ReservoirBank.predict re-aligns it; the C entry point asks for
    16-byte rows at n_in = 16); tensor noise; skewed 16x16x32 kernel."""
    torch, _, batched, _ = mods
    G, F, T, n_res = 2, 20, 30, 512
    bank, rs = make_bank(batched, 16, 8, n_res, G, noise=1e-3, seed=3)
    flat = torch.tensor(rs.randn(G * F * T * 16 + 1), dtype=torch.float32, device="cuda")
    U32 = flat[1:].view(G * F, T, 16)
    assert U32.data_ptr() % 16 != 0
    nz = torch.tensor(rs.rand(G * F, T, n_res), dtype=torch.float64, device="cuda")
    y32, y64 = predict_both(torch, bank, U32, F, T, 3, "f16", noise_mode="tensor", noise_u=nz)
    same_bits(y32, y64.float())


def test_predict_f32_siso_continuation(mods):
    """SISO shape (n_in = n_out = 2, N_res 100) with continuation x0 / y0, fp32 and fp16."""
    torch, _, batched, _ = mods
    G, F, T = 2, 24, 50
    bank, rs = make_bank(batched, 2, 2, 100, G, noise=1e-3, seed=5)
    x0 = torch.tensor(np.tanh(rs.randn(G, 100)), device="cuda")
    y0 = torch.tensor(rs.randn(G, 2), device="cuda")
    U32 = torch.tensor(rs.randn(G * F, T, 2), dtype=torch.float32, device="cuda")
    for prec in ("f32", "f16"):
        y32, y64 = predict_both(torch, bank, U32, F, T, 0, prec, x0=x0, y0=y0, seed=11)
        same_bits(y32, y64.float())


def test_predict_f32_weight_sets_with_group_offset(mods):
    torch, _, batched, _ = mods
    G, F, T = 5, 16, 36
    bank, rs = make_bank(batched, 16, 8, 512, G, n_wsets=3, noise=1e-3, seed=9)
    U32 = torch.tensor(rs.randn(G * F, T, 16), dtype=torch.float32, device="cuda")
    y32, y64 = predict_both(torch, bank, U32, F, T, 4, "f16", seed=13, group_offset=2)
    same_bits(y32, y64.float())


def test_predict_f32_rejects_f64(mods):
    torch, _lib, batched, _ = mods
    bank, rs = make_bank(batched, 4, 4, 64, 1)
    U32 = torch.zeros((4, 10, 4), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        bank.predict(U32, 4, precision="f64", io="f32")
    # the C entry point itself answers -2 for ESN_F64
    import ctypes as C
    out = torch.empty((4, 10, 4), dtype=torch.float32, device="cuda")
    rc = bank.lib.esn_predict_batch_f32(_lib.F64, C.byref(bank.shape), _lib.ptr(bank.packed_weights("f64")),
                                        _lib.ptr(bank.packed_readout("f64")), None, None, None, None, _lib.ptr(U32),
                                        4, 4, 10, 10, 0, None, None, 0.0, 0, None, 0, 0, _lib.ptr(out), None, 0,
                                        _lib.stream_handle())
    assert rc == -2 and b"ESN_F64" in bank.lib.esn_last_error()


@pytest.mark.parametrize("n_t,m,n_sub", [(4, 4, 128), (1, 2, 512)], ids=["4x8_16qam", "siso_qpsk"])
def test_detect_count_f32_matches_widened(mods, n_t, m, n_sub):
    torch, _, batched, _ = mods
    rs = np.random.RandomState(21)
    B, F = 12, 4
    bank, _ = make_bank(batched, 2, 2 * n_t, 16, 1)
    Y32 = torch.tensor(rs.randn(B, n_sub, 2 * n_t) * 0.7, dtype=torch.float32, device="cuda")
    bits = torch.tensor(rs.randint(0, 2, (B, n_sub * m, n_t)), dtype=torch.uint8, device="cuda")
    p_i = torch.tensor(0.5 + rs.rand(B // F), device="cuda")
    e32, n32, x32 = bank.detect_count(Y32, bits, p_i, F, n_sub, n_t, m, want_xhat=True)
    e64, n64, x64 = bank.detect_count(Y32.double(), bits, p_i, F, n_sub, n_t, m, want_xhat=True)
    torch.cuda.synchronize()
    assert torch.equal(e32, e64) and torch.equal(n32, n64) and int(e64.sum()) > 0
    same_bits(x32, x64)


@pytest.mark.parametrize("params", ["mimo", "siso"])
def test_gen_frames_c64_is_rounded_c128(mods, params):
    torch, _, _, mc = mods
    p = mc.LinkParams() if params == "mimo" else mc.LinkParams.siso_awgn(n_sub=128)
    src = mc.FrameSource(p, seed=4)
    taps = src.taps(3, 1, 5)
    F = 6
    rs = np.random.RandomState(2)
    bits_in = torch.tensor(rs.randint(0, 2, (3 * F, p.n_sub * p.m, p.n_t)), dtype=torch.uint8, device="cuda")
    noise_in = torch.tensor(rs.randn(3 * F, p.t_frame, 2 * p.n_r), device="cuda")
    cases = [dict(), dict(bits_in=bits_in, noise_in=noise_in), dict(ls_pattern=True)]
    for kw in cases:
        f = 1 if kw.get("ls_pattern") else F
        b64, x64, y64 = src.frames(taps, f, 12.0, 1, 30, 1, want_x=True, **kw)
        b32, x32, y32 = src.frames(taps, f, 12.0, 1, 30, 1, want_x=True, io="c64", **kw)
        torch.cuda.synchronize()
        assert y32.dtype == torch.complex64 and x32.dtype == torch.complex64
        assert torch.equal(b32, b64)
        same_bits(torch.view_as_real(y32), torch.view_as_real(y64.to(torch.complex64)))
        same_bits(torch.view_as_real(x32), torch.view_as_real(x64.to(torch.complex64)))


@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_sweep_f32_io_gives_identical_counters(mods, precision):
    _, _, _, mc = mods
    res = {}
    for io in ("f64", "f32"):
        sw = mc.DetectorSweep(mc.LinkParams(), n_reservoir=512, precision=precision, fit_precision=precision, io=io)
        res[io] = sw.run([6, 12, 18], 8, chunk_blocks=4)
    assert (res["f32"][1] == res["f64"][1]).all(), (res["f32"][1], res["f64"][1])
    assert res["f64"][1][:, 1].min() > 0


def test_sweep_f32_io_2048(mods):
    """N_res 2048 (GEMM-per-step path): Y is rounded from a double, so a detection decision may move."""
    _, _, _, mc = mods
    ber = {}
    for io in ("f64", "f32"):
        sw = mc.DetectorSweep(mc.LinkParams(), n_reservoir=2048, precision="f16", fit_precision="f16", io=io)
        ber[io] = sw.run([12], 4, frames_per_block=32, chunk_blocks=2)[0]
    assert np.allclose(ber["f32"], ber["f64"], rtol=1e-3, atol=0), ber


def test_io_keyword_errors(mods):
    torch, _, batched, mc = mods
    with pytest.raises(ValueError):
        mc.DetectorSweep(mc.LinkParams(), n_reservoir=64, precision="f64", io="f32")
    with pytest.raises(ValueError):
        mc.DetectorSweep(mc.LinkParams(), n_reservoir=64, precision="f16", io="f16")
    bank, _ = make_bank(batched, 4, 4, 64, 1)
    with pytest.raises(ValueError):
        bank.predict(torch.zeros((4, 10, 4), device="cuda"), 4, precision="f32", io="c64")
