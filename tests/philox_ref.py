"""The Philox4x32-10 streams of the generators restated in numpy (no GPU, no torch): what csrc/esn_gen.hip and
csrc/esn_reservoir.hip draw when the caller supplies no randomness.  tests/test_philox_reference_cpu.py holds the model
to known answers and to literal restatements; tests/test_gpu_philox_streams.py (MI355X) compares every kernel drawing
for itself with the same kernel fed these draws.

The generator (`struct Philox` of esn_gen.hip; `struct ResPhilox` of esn_reservoir.hip repeats it), all arithmetic
modulo 2^32, carried here in uint64 and masked:

    round(c, ka, kb):   p0 = 0xD2511F53 * c[0];  p1 = 0xCD9E8D57 * c[2]            (64-bit products)
                        c = (hi32(p1) ^ c[1] ^ ka,  lo32(p1),  hi32(p0) ^ c[3] ^ kb,  lo32(p0))
    10 rounds; after each  ka += 0x9E3779B9,  kb += 0xBB67AE85;  (ka, kb) starts as the key.

Every stream has key = (lo32(seed), hi32(seed)) and counter = (lo32(g), hi32(g), purpose, position), g the GLOBAL index
of a frame, a link or a weight set (offset + index inside the launch, a 64-bit sum):

    purpose  stream               g                 position                   words used
    1        payload bits         frame             call                       0..3: 32 / m symbols of m bits each
    2        AWGN                 frame             t ((n_r + 1) >> 1) + (rx >> 1)   (0, 1) even antenna, (2, 3) odd one
    3        tap gains            link              path                       (0, 1): one complex Gaussian
    4        Doppler angles       link              path * 16 + sinusoid       0: a, 1: phi
    16       reservoir W          set               element r n_res + c        (0, 1) value, (2, 3) sparsity mask
    17       reservoir W_in       set               element r n_in + c         (0, 1)
    18       reservoir W_fb       set               element r n_out + c        (0, 1)

The functions below state each rule again in their docstrings and return the draws in the layout the kernel's
"supplied randomness" argument takes (bits_in, noise_in, gains_in, angles_in, uniforms), so a test hands them straight
back to the kernel.  `err` (an Err) makes a function draw a WRONG stream on purpose; wrong_streams lists the ones the
suite must tell from the right one.
"""
import collections

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
MASK64 = 2 ** 64 - 1

PURPOSE_BITS, PURPOSE_NOISE, PURPOSE_TAPS, PURPOSE_DOPPLER = 1, 2, 3, 4
RES_PURPOSE_W, RES_PURPOSE_WIN, RES_PURPOSE_WFB = 16, 17, 18
DOPPLER_SINUSOIDS = 16


def _u(x):
    return np.asarray(x, dtype=np.uint64) & M32


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """uint32 [..., 4]: the four output words for counter (c0, c1, c2, c3) and key (k0, k1), broadcast together."""
    c0, c1, c2, c3, ka, kb = np.broadcast_arrays(_u(c0), _u(c1), _u(c2), _u(c3), _u(k0), _u(k1))
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0                 # < 2^64: exact in uint64
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ ka, p1 & M32, (p0 >> S32) ^ c3 ^ kb, p0 & M32
        ka = (ka + np.uint64(0x9E3779B9)) & M32
        kb = (kb + np.uint64(0xBB67AE85)) & M32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


# ---- the errors a test must be able to see ------------------------------------------------------------------------------
#   g_shift       added to the global frame / link / set index               ("frame + 1")
#   pos_shift     added to the counter position                              ("counter position + 1")
#   swap01        words 0 and 1 exchanged
#   drop_seed_hi  the key's second word is 0 instead of hi32(seed)
#   drop_g_hi     the counter's second word is 0 instead of hi32(g)
#   swap_pair     words (0, 1) and (2, 3) exchanged: the even and the odd antenna of a noise pair, value and mask of W
Err = collections.namedtuple("Err", "g_shift pos_shift swap01 drop_seed_hi drop_g_hi swap_pair", defaults=(0, 0, 0, 0, 0, 0))
RIGHT = Err()
WRONG = {"frame + 1": Err(g_shift=1),
         "counter position + 1": Err(pos_shift=1),
         "words 0 <-> 1": Err(swap01=1),
         "high half of seed dropped": Err(drop_seed_hi=1),
         "high half of offset dropped": Err(drop_g_hi=1),
         "even <-> odd antenna (words 0,1 <-> 2,3)": Err(swap_pair=1)}


def _words(seed, g, purpose, pos, err=RIGHT):
    """uint64 [..., 4] (values below 2^32): the words of counter (g, purpose, pos) under key seed, with err applied."""
    seed = int(seed) & MASK64
    g = (int(g) + err.g_shift) & MASK64
    k1 = 0 if err.drop_seed_hi else seed >> 32
    c1 = 0 if err.drop_g_hi else g >> 32
    w = philox4x32_10(g & 0xFFFFFFFF, c1, purpose, np.asarray(pos, dtype=np.uint64) + np.uint64(err.pos_shift),
                      seed & 0xFFFFFFFF, k1).astype(np.uint64)
    if err.swap01:
        w = w[..., [1, 0, 2, 3]]
    if err.swap_pair:
        w = w[..., [2, 3, 0, 1]]
    return w


def frame_bits(seed, gf, N, n_t, m, err=RIGHT):
    """uint8 [N m, n_t]: the payload of global frame gf (bits / bits_in of esn_gen_frames: bit b of subcarrier sc and
    transmitter tx at row sc m + b, column tx).

    Counter (lo32(gf), hi32(gf), 1, call).  A call's four words hold spw = 32 // m symbols each (the spare high bits of
    a word are not used); symbol j of word q of the call is element e = call 4 spw + q spw + j of the frame, elements
    counted transmitter first: sc = e // n_t, tx = e % n_t.  Its constellation index is (w[q] >> (j m)) & (2^m - 1), and
    bit b of the index is the payload bit.  The last call may be ragged: elements >= N n_t do not exist.  The kernel's
    branch for m = 4, n_t = 4 is this rule with spw = 8 (a call is 8 whole subcarriers)."""
    spw = 32 // m
    spc = 4 * spw
    n_el = N * n_t
    calls = (n_el + spc - 1) // spc
    w = _words(seed, gf, PURPOSE_BITS, np.arange(calls), err)                             # [calls, 4]
    j = np.arange(spw, dtype=np.uint64) * np.uint64(m)
    idx = (w[:, :, None] >> j[None, None, :]) & np.uint64((1 << m) - 1)                   # [calls, 4, spw] = element order
    idx = idx.reshape(-1)[:n_el].reshape(N, n_t)
    b = np.arange(m, dtype=np.uint64)
    return ((idx[:, None, :] >> b[None, :, None]) & np.uint64(1)).astype(np.uint8).reshape(N * m, n_t)


def frame_noise(seed, gf, T, n_r, err=RIGHT):
    """complex128 [T, n_r]: the unit-variance-per-component AWGN of global frame gf (y_cp = channel + sqrt(T No / 2) z).

    Counter (lo32(gf), hi32(gf), 2, t ((n_r + 1) >> 1) + (rx >> 1)): one call per PAIR of receive antennas; words
    (0, 1) = (a, b) give the even antenna of the pair, words (2, 3) the odd one (unused when n_r is odd and the pair is
    the last).  From the top 24 bits of each word
        u1 = ((a >> 8) + 0.5) / 2^24,   u2 = (b >> 8) / 2^24,   z = sqrt(-2 ln u1) (cos 2 pi u2 + j sin 2 pi u2).
    The kernel evaluates this with the float32 hardware transcendentals; here it is float64."""
    pairs = (n_r + 1) >> 1
    pos = np.arange(T, dtype=np.uint64)[:, None] * np.uint64(pairs) + np.arange(pairs, dtype=np.uint64)[None, :]
    w = _words(seed, gf, PURPOSE_NOISE, pos & M32, err)                                   # [T, pairs, 4]
    w = w.reshape(T, pairs * 2, 2)[:, :n_r]                                               # antenna rx: words 2 (rx & 1) + {0, 1}
    u1 = ((w[..., 0] >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0
    u2 = (w[..., 1] >> np.uint64(8)).astype(np.float64) / 16777216.0
    rr = np.sqrt(-2.0 * np.log(u1))
    return rr * np.cos(2.0 * np.pi * u2) + 1j * (rr * np.sin(2.0 * np.pi * u2))


def link_gains(seed, gl, n_paths, err=RIGHT):
    """complex128 [n_paths]: the standard-normal pairs (gains_in of esn_gen_taps) of global link gl.

    Counter (lo32(gl), hi32(gl), 3, path); float64 Box-Muller on words 0 and 1:
        u1 = (w0 + 0.5) / 2^32,  u2 = (w1 + 0.5) / 2^32,  g = sqrt(-2 ln u1) (cos 2 pi u2 + j sin 2 pi u2).
    gl = link_offset + (blk n_r + rx) n_t + tx.  n_paths is 23 for kind 0 (TDL-B), isi for kind 1, 1 for kind 2."""
    w = _words(seed, gl, PURPOSE_TAPS, np.arange(n_paths), err)
    u1 = (w[:, 0].astype(np.float64) + 0.5) / 4294967296.0
    u2 = (w[:, 1].astype(np.float64) + 0.5) / 4294967296.0
    rr = np.sqrt(-2.0 * np.log(u1))
    return rr * np.cos(2.0 * np.pi * u2) + 1j * (rr * np.sin(2.0 * np.pi * u2))


def doppler_angles(seed, gl, n_paths, err=RIGHT):
    """float64 [n_paths, 16, 2] = (a, phi) in half-turns, [0, 2): angles_in of esn_gen_taps_doppler for global link gl.

    Counter (lo32(gl), hi32(gl), 4, p 16 + m) for sinusoid m of path p; a = (w0 + 0.5) / 2^31, phi = (w1 + 0.5) / 2^31
    (33 significant bits: exact in float64 on both sides)."""
    w = _words(seed, gl, PURPOSE_DOPPLER, np.arange(n_paths * DOPPLER_SINUSOIDS), err)
    return ((w[:, :2].astype(np.float64) + 0.5) / 2147483648.0).reshape(n_paths, DOPPLER_SINUSOIDS, 2)


def res_uniform(a, b):
    """53-bit uniform in [0, 1) from two words, as NumPy's random_sample builds it: ((a >> 5) 2^26 + (b >> 6)) / 2^53."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    return ((a >> np.uint64(5)).astype(np.float64) * 67108864.0 + (b >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0


def reservoir_uniforms(seed, gs, n_res, n_in, n_out, err=RIGHT):
    """float64 [2 n_res^2 + n_res n_in + n_res n_out]: the row of `uniforms` of esn_gen_reservoirs for global set gs, in
    the reference's draw order  rand(n, n) | mask rand(n, n) | rand(n, n_in) | rand(n, n_out).

    Counter (lo32(gs), hi32(gs), purpose, element): purpose 16 for W, element e = r n_res + c, value = res_uniform(w0, w1)
    and mask = res_uniform(w2, w3); purpose 17 for W_in (element r n_in + c) and 18 for W_fb (element r n_out + c), both
    res_uniform(w0, w1)."""
    nn = n_res * n_res
    ww = _words(seed, gs, RES_PURPOSE_W, np.arange(nn), err)
    wi = _words(seed, gs, RES_PURPOSE_WIN, np.arange(n_res * n_in), err)
    wf = _words(seed, gs, RES_PURPOSE_WFB, np.arange(n_res * n_out), err)
    return np.concatenate([res_uniform(ww[:, 0], ww[:, 1]), res_uniform(ww[:, 2], ww[:, 3]),
                           res_uniform(wi[:, 0], wi[:, 1]), res_uniform(wf[:, 0], wf[:, 1])])


STREAMS = {"bits": frame_bits, "noise": frame_noise, "gains": link_gains, "angles": doppler_angles,
           "uniforms": reservoir_uniforms}


def draws(stream, seed, offset, count, *shape, err=RIGHT):
    """The draws of `count` consecutive global indices offset, offset + 1, ... stacked on a new first axis: the array a
    launch over `count` frames / links / sets takes as its supplied randomness."""
    return np.stack([STREAMS[stream](seed, int(offset) + i, *shape, err=err) for i in range(count)])


def wrong_streams(stream, seed, offset, count, *shape):
    """{name: draws} with each error of WRONG: the same call as draws(...), drawn wrongly in one way."""
    return {name: draws(stream, seed, offset, count, *shape, err=e) for name, e in WRONG.items()}


def reach(stream, name, offset, count, *shape):
    """bool, broadcastable to the samples of draws(stream, seed, offset, count, *shape) (bits: to the symbols
    [count, N, n_t]): the samples error `name` of WRONG can change at all.
      * dropping the high half of the offset is invisible at the indices where that half is zero;
      * exchanging words 0 and 1 leaves alone what words 2 and 3 make: the symbols of the second half of a bits call,
        the odd antenna of a noise pair, the mask uniforms of W;
      * every other error reaches every sample."""
    idx = np.ones(count, dtype=bool)
    if name == "high half of offset dropped":
        idx = np.array([((int(offset) + i) & MASK64) >> 32 != 0 for i in range(count)])
    inner = np.ones((), dtype=bool)
    if name == "words 0 <-> 1":
        if stream == "bits":
            N, n_t, m = shape
            spw = 32 // m
            inner = ((np.arange(N * n_t) % (4 * spw)) // spw < 2).reshape(N, n_t)
        elif stream == "noise":
            T, n_r = shape
            inner = np.broadcast_to(np.arange(n_r) % 2 == 0, (T, n_r))
        elif stream == "uniforms":
            n_res, n_in, n_out = shape
            nn = n_res * n_res
            inner = np.ones(2 * nn + n_res * (n_in + n_out), dtype=bool)
            inner[nn:2 * nn] = False
    return idx.reshape((count,) + (1,) * inner.ndim) & inner[None]


# ---- what the CPU and the GPU test share --------------------------------------------------------------------------------
SEED = 0x0123456789ABCDEF                    # both halves non-zero
FRAME_OFFSET = 2 ** 32 - 1                   # 3 frames: 2^32 - 1, 2^32, 2^32 + 1 -- the counter's second word becomes 1
LINK_OFFSET = 2 ** 32 - 2                    # 3 blocks of links cross the same boundary
FIRST_SET = 2 ** 32 - 1
N_FRAMES = 3

# (N, n_t, m) of the bits cases
BITS_SHAPES = [(8, 4, 4), (128, 4, 4),       # m = 4, n_t = 4 branch: one call, 16 calls
               (8, 3, 6),                    # 24 elements, 20 per call: ragged last call; sc % n_t with n_t = 3
               (16, 4, 2),                   # exactly one full call
               (4, 1, 10),                   # 3 symbols per word, 2 spare bits
               (64, 1, 2),                   # SISO
               (1024, 4, 10)]                # 342 calls for 256 threads: the second pass of the strided loop
BITS_SMALL_N = [(4, 4, 4), (2, 4, 4)]        # m = 4, n_t = 4 below one call of 8 subcarriers
NOISE_NR = [1, 2, 3, 8]                      # half-used pair; one pair; pair + half; two antenna groups of 4
NOISE_T = [9, 71, 135]                       # N + cp = 8 + 1, 64 + 7, 128 + 7: < one 64-sample chunk, ragged second, three
# (kind, isi) -> paths per link of esn_gen_taps
TAP_KINDS = [(0, 1), (0, 8), (0, 16), (1, 1), (1, 8), (2, 1)]
TAP_ANTENNAS = [(1, 1), (2, 3), (8, 4)]      # (n_r, n_t)
RES_SHAPES = [(5, 1, 1, 0.0), (64, 4, 2, 0.2), (130, 16, 8, 0.9)]      # (n_res, n_in, n_out, sparsity)


def tap_paths(kind, isi):
    return 23 if kind == 0 else (isi if kind == 1 else 1)
