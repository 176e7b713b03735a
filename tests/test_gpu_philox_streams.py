"""The Philox streams the generator kernels draw for themselves (csrc/esn_gen.hip, csrc/esn_reservoir.hip) against the
host model tests/philox_ref.py, through the C ABI so that seed and offsets are explicit.  Every case compares the kernel
DRAWING FOR ITSELF with the SAME kernel FED the model's draws (bits_in, gains_in, angles_in, uniforms), or, for the
AWGN, reads the draws back through a zero channel.  The seed has both halves set and every offset crosses 2^32 inside
the launch (philox_ref.SEED / FRAME_OFFSET / LINK_OFFSET / FIRST_SET), so the high words of key and counter count.
tests/test_philox_reference_cpu.py shows, without a GPU, that every wrong stream (frame + 1, position + 1, words
exchanged, a high half dropped, antennas exchanged) differs from the right one in most samples at these very shapes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import philox_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu

FS_HZ, DS_NS = 2 * 1.024e6, 300.0            # LinkParams' sampling rate and delay spread: TDL-B delays up to 2.9 samples

# Largest |device sample - float64 model| (real or imaginary part) of the AWGN over all cases of
# test_noise_equals_the_model, both entry points, measured on the MI355X: 1.051e-6 (n_r = 8, T = 135, complex128; the
# largest |z| there is 4.0).  The kernel's Box-Muller runs on v_log_f32 / v_sqrt_f32 / v_sin_f32 / v_cos_f32.
NOISE_MEASURED = 1.051e-6
NOISE_TOL = 4 * NOISE_MEASURED


@pytest.fixture(scope="module")
def gpu():
    import torch
    from esn_ofdm_mimo_amd import _lib
    return torch, _lib, _lib.load()


def dev(torch, a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def gen_frames(gpu, N, cp, n_t, n_r, isi, m, taps, *, n_frames=pr.N_FRAMES, fpb=1, ls=0, p_i=2e-3, a_clip=1.0, no=1e-5,
               bits_in=None, noise_in=None, seed=pr.SEED, frame_offset=pr.FRAME_OFFSET, c64=False, guard=0):
    """One esn_gen_frames / esn_gen_frames_c64 call.  taps complex [n_blocks, n_r, n_t, isi].  Returns numpy
    (bits [B, N m, n_t], x_cp [B, T, n_t], y_cp [B, T, n_r], the `guard` bytes behind bits)."""
    torch, _lib, lib = gpu
    T, n_blocks = N + cp, (n_frames + fpb - 1) // fpb
    assert taps.shape == (n_blocks, n_r, n_t, isi)
    taps_d = dev(torch, taps.astype(np.complex128))
    pi_d, ac_d = dev(torch, np.full(n_blocks, p_i)), dev(torch, np.full(n_blocks, a_clip))
    nbits = n_frames * N * m * n_t
    bits = torch.full((nbits + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    cdt = torch.complex64 if c64 else torch.complex128
    x_cp = torch.empty((n_frames, T, n_t), dtype=cdt, device="cuda")
    y_cp = torch.empty((n_frames, T, n_r), dtype=cdt, device="cuda")
    bi, ni = dev(torch, bits_in), dev(torch, noise_in)
    name = "esn_gen_frames_c64" if c64 else "esn_gen_frames"
    _lib.check(getattr(lib, name)(n_frames, fpb, N, cp, n_t, n_r, isi, m, ls, _lib.ptr(pi_d), _lib.ptr(ac_d), no,
                                  _lib.ptr(taps_d), _lib.ptr(bi), _lib.ptr(ni), seed, frame_offset, _lib.ptr(bits),
                                  _lib.ptr(x_cp), _lib.ptr(y_cp), _lib.stream_handle()), name)
    torch.cuda.synchronize()
    b = bits.cpu().numpy()
    return b[:nbits].reshape(n_frames, N * m, n_t), x_cp.cpu().numpy(), y_cp.cpu().numpy(), b[nbits:]


def some_taps(n_blocks, n_r, n_t, isi, seed=0):
    rs = np.random.RandomState(seed)
    return (rs.randn(n_blocks, n_r, n_t, isi) + 1j * rs.randn(n_blocks, n_r, n_t, isi)) / np.sqrt(2 * isi)


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- bits and transmitter ---------------------------------------------------------------------------------------------
def check_bits_case(gpu, N, n_t, m, ls, n_r, isi, guard=0):
    cp = isi - 1
    taps = some_taps(pr.N_FRAMES, n_r, n_t, isi)
    want = pr.draws("bits", pr.SEED, pr.FRAME_OFFSET, pr.N_FRAMES, N, n_t, m)
    own = gen_frames(gpu, N, cp, n_t, n_r, isi, m, taps, ls=ls, guard=guard)
    fed = gen_frames(gpu, N, cp, n_t, n_r, isi, m, taps, ls=ls, bits_in=want, guard=guard)
    bad = own[0] != want
    print(f"N={N} n_t={n_t} m={m} ls={ls}: {int(bad.sum())} of {want.size} bits differ from the model; "
          f"x_cp bitwise {same_bytes(own[1], fed[1])}, y_cp bitwise {same_bytes(own[2], fed[2])}")
    np.testing.assert_array_equal(fed[0], want)                  # (the supplied bits come back)
    np.testing.assert_array_equal(own[0], want)
    assert np.isfinite(own[1]).all() and np.abs(own[1]).max() > 0
    assert same_bytes(own[1], fed[1])                            # same bits, same float64 arithmetic
    assert same_bytes(own[2], fed[2])                            # and the same noise: it does not depend on the bits path
    if ls:                                                       # sparse pilot: the frames are not those of ls = 0
        full = gen_frames(gpu, N, cp, n_t, n_r, isi, m, taps, ls=0, bits_in=want)
        assert n_t == 1 or not same_bytes(own[1], full[1])
    return own, fed


@pytest.mark.parametrize("ls", [0, 1])
@pytest.mark.parametrize("N,n_t,m", pr.BITS_SHAPES, ids=lambda v: str(v))
def test_bits_equal_the_model_and_the_transmitter_follows(gpu, N, n_t, m, ls):
    """bits_in = NULL: `bits` equal frame_bits exactly, and x_cp (and y_cp) are bitwise those of a second call fed the
    model's bits -- for the m = 4, n_t = 4 branch (16-byte bit stores, its own constellation and pilot-pattern code) and
    the general one (32 // m symbols per word, ragged last call), with ls_pattern 0 and 1."""
    big = N == 1024
    check_bits_case(gpu, N, n_t, m, ls, n_r=1 if big else 2, isi=1 if big else 2)


@pytest.mark.parametrize("ls", [0, 1])
@pytest.mark.parametrize("N,n_t,m", pr.BITS_SMALL_N, ids=lambda v: str(v))
def test_bits_below_one_call_of_the_headline_shape_stay_inside_their_frame(gpu, N, n_t, m, ls):
    """m = 4, n_t = 4 with fewer than 8 subcarriers: less than one call of the 16-byte-store branch, which writes 8 whole
    subcarriers per call.  The kernel takes the general branch there; the bytes behind `bits` stay as they were."""
    own, fed = check_bits_case(gpu, N, n_t, m, ls, n_r=2, isi=2, guard=256)
    assert (own[3] == 0xA5).all() and (fed[3] == 0xA5).all()


def test_the_seed_and_the_frame_offset_enter_with_both_halves(gpu):
    """The comparisons above run at one (seed, offset); here the device itself shows that changing only the HIGH half of
    the seed, or moving the offset by 2^32, gives other bits, and that frame f of a launch at offset o is frame 0 of a
    launch at o + f."""
    N, n_t, m, n_r, isi = 8, 4, 4, 2, 2
    taps = some_taps(pr.N_FRAMES, n_r, n_t, isi)
    base = gen_frames(gpu, N, 1, n_t, n_r, isi, m, taps)
    hi_seed = gen_frames(gpu, N, 1, n_t, n_r, isi, m, taps, seed=pr.SEED ^ (1 << 40))
    hi_off = gen_frames(gpu, N, 1, n_t, n_r, isi, m, taps, frame_offset=pr.FRAME_OFFSET + 2 ** 32)
    assert (base[0] != hi_seed[0]).mean() > 0.3 and (base[0] != hi_off[0]).mean() > 0.3
    assert (base[2] != hi_seed[2]).mean() > 0.99 and (base[2] != hi_off[2]).mean() > 0.99
    one = gen_frames(gpu, N, 1, n_t, n_r, isi, m, taps[2:], n_frames=1, frame_offset=pr.FRAME_OFFSET + 2)
    assert same_bytes(one[0][0], base[0][2]) and same_bytes(one[2][0], base[2][2])


# ---- AWGN -------------------------------------------------------------------------------------------------------------
def noise_readback(gpu, T, n_r, c64):
    """The kernel's own noise samples [3, T, n_r]: zero taps make y_cp = sqrt(T No / 2) z exactly; divide it out."""
    N, cp = {9: (8, 1), 71: (64, 7), 135: (128, 7)}[T]
    no = 1e-5
    taps = np.zeros((1, n_r, 1, 1), dtype=np.complex128)
    _, _, y, _ = gen_frames(gpu, N, cp, 1, n_r, 1, 2, taps, fpb=pr.N_FRAMES, no=no, c64=c64)
    return y, np.sqrt(float(T) * no * 0.5)


@pytest.mark.parametrize("T", pr.NOISE_T)
@pytest.mark.parametrize("n_r", pr.NOISE_NR)
def test_noise_equals_the_model(gpu, n_r, T):
    """Both store paths (esn_gen_frames: complex128; esn_gen_frames_c64: complex64, one 16-byte store per antenna pair
    when n_r is even) against frame_noise, for n_r = 1, 2, 3, 8 (half-used pair, odd tail, two antenna groups) and
    T = 9, 71, 135 (less than one 64-sample chunk, ragged second chunk, three chunks).

    The kernel's Box-Muller is float32 hardware transcendentals against a float64 model, so the tolerance cannot be
    derived; it is four times the largest difference measured on the MI355X over all these cases and both entry points,
    4 x 1.051e-6 = 4.2e-6 (per case the measured maxima run from 1.7e-7 at n_r = 1, T = 9 to 1.05e-6 at n_r = 8,
    T = 135, the same to three digits in complex128 and complex64), and must stay below 1e-4: a stream error moves a
    unit-variance sample by O(1), and the CPU test shows that every wrong stream exceeds 1e-4 on nearly every sample it
    reaches.  The complex64 output is also bitwise the
    complex128 output rounded, for odd and even n_r."""
    want = pr.draws("noise", pr.SEED, pr.FRAME_OFFSET, pr.N_FRAMES, T, n_r)
    y64, sig = noise_readback(gpu, T, n_r, False)
    y32, _ = noise_readback(gpu, T, n_r, True)
    e64, e32 = y64 / sig - want, y32.astype(np.complex128) / sig - want
    d64 = np.maximum(np.abs(e64.real), np.abs(e64.imag))
    d32 = np.maximum(np.abs(e32.real), np.abs(e32.imag))
    print(f"n_r={n_r} T={T}: max |device - model| c128 {d64.max():.3e}  c64 {d32.max():.3e}  (max |z| {np.abs(want).max():.2f})")
    assert y32.dtype == np.complex64 and same_bytes(y32, y64.astype(np.complex64))
    assert NOISE_TOL == 4 * NOISE_MEASURED and NOISE_TOL < 1e-4
    assert d64.max() <= NOISE_TOL, d64.max()
    assert d32.max() <= NOISE_TOL, d32.max()


# ---- taps -------------------------------------------------------------------------------------------------------------
def gen_taps(gpu, kind, n_blocks, n_r, n_t, isi, gains=None, seed=pr.SEED, link_offset=pr.LINK_OFFSET):
    torch, _lib, lib = gpu
    out = torch.full((n_blocks, n_r, n_t, isi), float("nan"), dtype=torch.complex128, device="cuda")
    g = dev(torch, gains)
    _lib.check(lib.esn_gen_taps(kind, n_blocks, n_r, n_t, isi, FS_HZ, DS_NS, _lib.ptr(g), seed, link_offset,
                                _lib.ptr(out), _lib.stream_handle()), "esn_gen_taps")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("n_r,n_t", pr.TAP_ANTENNAS)
@pytest.mark.parametrize("kind,isi", pr.TAP_KINDS)
def test_taps_equal_the_kernel_fed_the_model_gains(gpu, kind, isi, n_r, n_t):
    """esn_gen_taps drawing for itself against esn_gen_taps with gains_in = link_gains, for TDL-B, exponential PDP and
    the flat channel; link_offset = 2^32 - 2 across 3 blocks.  Within 1e-12 of the largest tap (the float64 bar of
    tests/test_gpu_framegen.py): the device's log / sincospi and NumPy's log / cos / sin differ by ulps only."""
    n_blocks, paths = 3, pr.tap_paths(kind, isi)
    g = pr.draws("gains", pr.SEED, pr.LINK_OFFSET, n_blocks * n_r * n_t, paths)            # [links, paths] complex
    own = gen_taps(gpu, kind, n_blocks, n_r, n_t, isi)
    fed = gen_taps(gpu, kind, n_blocks, n_r, n_t, isi, gains=g)
    err = np.abs(own - fed).max() / np.abs(fed).max()
    print(f"kind={kind} isi={isi} {n_r}x{n_t}: max |own - fed| / max |tap| = {err:.2e}")
    assert np.isfinite(fed).all() and np.abs(fed).max() > 0
    assert err <= 1e-12
    # the links are distinct draws (a constant would pass the comparison above)
    flat = fed.reshape(-1, isi)
    assert len({r.tobytes() for r in flat}) == flat.shape[0]


# ---- Doppler ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fd_tsym", [0.0, 0.05])
@pytest.mark.parametrize("n_sym", [1, 5])
@pytest.mark.parametrize("kind", [0, 1])
def test_doppler_taps_equal_the_kernel_fed_the_model_angles(gpu, kind, n_sym, fd_tsym):
    """esn_gen_taps_doppler drawing for itself against angles_in = doppler_angles.  a and phi are (w + 0.5) / 2^31, exact
    in float64 on both sides, and everything after them is the same code: bitwise."""
    torch, _lib, lib = gpu
    n_blocks, n_r, n_t, isi = 3, 2, 3, 8
    ang = pr.draws("angles", pr.SEED, pr.LINK_OFFSET, n_blocks * n_r * n_t, pr.tap_paths(kind, isi))

    def run(angles):
        out = torch.full((n_blocks, n_sym, n_r, n_t, isi), float("nan"), dtype=torch.complex128, device="cuda")
        a = dev(torch, angles)
        _lib.check(lib.esn_gen_taps_doppler(kind, n_blocks, n_sym, n_r, n_t, isi, FS_HZ, DS_NS, fd_tsym, _lib.ptr(a),
                                            pr.SEED, pr.LINK_OFFSET, _lib.ptr(out), _lib.stream_handle()),
                   "esn_gen_taps_doppler")
        torch.cuda.synchronize()
        return out.cpu().numpy()

    own, fed = run(None), run(ang)
    print(f"kind={kind} n_sym={n_sym} fd_tsym={fd_tsym}: max |own - fed| = {np.abs(own - fed).max():.2e}")
    assert np.isfinite(fed).all() and np.abs(fed).max() > 0
    assert same_bytes(own, fed)
    links = fed[:, 0].reshape(-1, isi)
    assert len({r.tobytes() for r in links}) == links.shape[0]


# ---- reservoirs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_res,n_in,n_out,sparsity", pr.RES_SHAPES)
def test_reservoirs_equal_the_kernel_fed_the_model_uniforms(gpu, n_res, n_in, n_out, sparsity):
    """esn_gen_reservoirs drawing for itself against uniforms = reservoir_uniforms: W, W_in and W_fb bitwise, for two sets
    at first_set = 2^32 - 1 (the second set's counter has its high word set)."""
    torch, _lib, lib = gpu
    n_sets = 2
    u = pr.draws("uniforms", pr.SEED, pr.FIRST_SET, n_sets, n_res, n_in, n_out)

    def run(uniforms):
        W = torch.full((n_sets, n_res, n_res), float("nan"), dtype=torch.float64, device="cuda")
        W_in = torch.full((n_sets, n_res, n_in), float("nan"), dtype=torch.float64, device="cuda")
        W_fb = torch.full((n_sets, n_res, n_out), float("nan"), dtype=torch.float64, device="cuda")
        ud = dev(torch, uniforms)
        _lib.check(lib.esn_gen_reservoirs(n_res, n_in, n_out, sparsity, pr.SEED, pr.FIRST_SET, n_sets, _lib.ptr(ud),
                                          _lib.ptr(W), _lib.ptr(W_in), _lib.ptr(W_fb), _lib.stream_handle()),
                   "esn_gen_reservoirs")
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (W, W_in, W_fb)]

    own, fed = run(None), run(u)
    for name, a, b in zip(("W", "W_in", "W_fb"), own, fed):
        print(f"n_res={n_res} {name}: {int((a != b).sum())} of {a.size} entries differ")
        assert np.isfinite(b).all()
        assert same_bytes(a, b), name
    # the fed run is the NumPy expression on the model's uniforms; set first_set + i lies in slot (first_set + i) % n_sets
    nn = n_res * n_res
    for i in range(n_sets):
        slot = (pr.FIRST_SET + i) % n_sets
        w = np.where(u[i, nn:2 * nn] < sparsity, 0.0, u[i, :nn] - 0.5).reshape(n_res, n_res)
        assert same_bytes(fed[0][slot], w)
        assert same_bytes(fed[1][slot], (u[i, 2 * nn:2 * nn + n_res * n_in] * 2.0 - 1.0).reshape(n_res, n_in))
        assert same_bytes(fed[2][slot], (u[i, 2 * nn + n_res * n_in:] * 2.0 - 1.0).reshape(n_res, n_out))
    assert not same_bytes(fed[0][0], fed[0][1])
    zeros = float((fed[0] == 0.0).mean())
    assert abs(zeros - sparsity) <= 4 * np.sqrt(sparsity * (1 - sparsity) / fed[0].size)


# ---- the Python layer -------------------------------------------------------------------------------------------------
def frames_key(seed, *parts):
    """FrameSource._key restated: h = seed; for each part  h = (h * 6364136223846793005 + part + 0x9E3779B97F4A7C15)
    mod 2^64."""
    h = seed & (2 ** 64 - 1)
    for k in parts:
        h = (h * 6364136223846793005 + k + 0x9E3779B97F4A7C15) % 2 ** 64
    return h


@pytest.mark.parametrize("si,first_block", [(0, 5), (3, 2)])
def test_blocks_fast_is_the_c_abi_with_the_derived_seeds_and_offsets(gpu, si, first_block):
    """FrameSource.blocks_fast(ebno, si, first_block, G, F) equals hand calls of the C ABI with what frames.py derives
    from (seed, SNR index, first block):

        key(parts) = fold of  h <- (h * 6364136223846793005 + part + 0x9E3779B97F4A7C15) mod 2^64  from h = seed
        taps    esn_gen_taps    seed = key(si, 1),  link_offset  = first_block * n_r * n_t
        pilots  esn_gen_frames  seed = key(si, 2),  frame_offset = first_block,      1 frame per block
        data    esn_gen_frames  seed = key(si, 3),  frame_offset = first_block * F,  F frames per block
        p_i = 10^(ebno / 10) No and a_clip = sqrt(p_i N) 10^(clip_db / 20) for every block.

    So a block's draws depend on (seed, SNR index, block index) alone -- what the multi-rank runs rely on.  The data
    bits are also the model's for that key and offset."""
    torch, _lib, lib = gpu
    from esn_ofdm_mimo_amd.montecarlo import FrameSource, LinkParams
    p = LinkParams()
    seed, ebno, G, F = 11, 9.0, 2, 3
    got = FrameSource(p, seed=seed).blocks_fast(ebno, si, first_block, G, F)
    torch.cuda.synchronize()
    p_i = 10 ** (ebno / 10) * p.no
    a_clip = np.sqrt(p_i * p.n_sub) * 10 ** (p.clip_db / 20)
    assert p_i == p.p_i(ebno) and a_clip == p.a_clip(ebno)
    taps = gen_taps(gpu, 0, G, p.n_r, p.n_t, p.isi, seed=frames_key(seed, si, 1),
                    link_offset=first_block * p.n_r * p.n_t)
    kw = dict(p_i=p_i, a_clip=a_clip, no=p.no)
    pil = gen_frames(gpu, p.n_sub, p.cp, p.n_t, p.n_r, p.isi, p.m, taps, n_frames=G, fpb=1,
                     seed=frames_key(seed, si, 2), frame_offset=first_block, **kw)
    dat = gen_frames(gpu, p.n_sub, p.cp, p.n_t, p.n_r, p.isi, p.m, taps, n_frames=G * F, fpb=F,
                     seed=frames_key(seed, si, 3), frame_offset=first_block * F, **kw)
    assert same_bytes(got["taps"].cpu().numpy(), taps)
    assert same_bytes(got["pilot_bits"].cpu().numpy(), pil[0])
    assert same_bytes(got["pilot_x"].cpu().numpy(), pil[1])
    assert same_bytes(got["pilot_y"].cpu().numpy(), pil[2])
    assert same_bytes(got["data_bits"].cpu().numpy(), dat[0])
    assert same_bytes(got["data_y"].cpu().numpy(), dat[2])
    np.testing.assert_array_equal(dat[0], pr.draws("bits", frames_key(seed, si, 3), first_block * F, G * F,
                                                   p.n_sub, p.n_t, p.m))
    np.testing.assert_array_equal(pil[0], pr.draws("bits", frames_key(seed, si, 2), first_block, G, p.n_sub, p.n_t, p.m))
