"""tests/philox_ref.py, the host model of the generators' Philox streams, held to account without a GPU: known answers
of the round function, a scalar loop in plain Python integers, a literal per-symbol restatement of the bits rule, the
separation of every wrong stream from the right one at the shapes tests/test_gpu_philox_streams.py uses, and the
distribution of the model's own draws."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import philox_ref as pr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# counter / key -> output; the first is the all-zero vector of the published Philox4x32-10 test vectors
KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
          (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def philox_scalar(c, k):
    """The round function in plain Python integers, one counter at a time."""
    c, (ka, kb) = list(c), k
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ ka) & 0xFFFFFFFF, p1 & 0xFFFFFFFF, ((p0 >> 32) ^ c[3] ^ kb) & 0xFFFFFFFF,
             p0 & 0xFFFFFFFF]
        ka, kb = (ka + 0x9E3779B9) & 0xFFFFFFFF, (kb + 0xBB67AE85) & 0xFFFFFFFF
    return tuple(c)


@pytest.mark.parametrize("c,k,want", KNOWN)
def test_known_answers(c, k, want):
    assert philox_scalar(c, k) == want
    got = pr.philox4x32_10(*c, *k)
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert tuple(int(x) for x in got) == want


def test_vectorised_model_equals_the_scalar_loop():
    rs = np.random.RandomState(0)
    c = rs.randint(0, 2 ** 32, (200, 4), dtype=np.uint64)
    k = rs.randint(0, 2 ** 32, (200, 2), dtype=np.uint64)
    c[:4] = [[0xffffffff, 0, 0xffffffff, 0], [0, 0xffffffff, 0, 0xffffffff], [1, 0, 0, 0], [0, 0, 0, 1]]
    got = pr.philox4x32_10(c[:, 0], c[:, 1], c[:, 2], c[:, 3], k[:, 0], k[:, 1])
    assert got.shape == (200, 4)
    for i in range(200):
        assert tuple(int(x) for x in got[i]) == philox_scalar([int(x) for x in c[i]], (int(k[i, 0]), int(k[i, 1]))), i
    # broadcasting: one key, a grid of counters
    grid = pr.philox4x32_10(np.arange(3)[:, None], 7, 2, np.arange(5)[None, :], 11, 13)
    assert grid.shape == (3, 5, 4)
    assert tuple(int(x) for x in grid[2, 4]) == philox_scalar([2, 7, 2, 4], (11, 13))


def test_both_kernel_files_state_the_rounds_the_model_restates():
    """ResPhilox (esn_reservoir.hip) says it repeats Philox (esn_gen.hip): the two bodies are the same text, and carry
    the constants of the model -- one model serves both."""
    def body(path, name):
        src = open(os.path.join(ROOT, "esn_ofdm_mimo_amd", "csrc", path)).read()
        m = re.search(r"struct %s \{(.*?)\n\};" % name, src, re.S)
        assert m, (path, name)
        return m.group(1)
    gen, res = body("esn_gen.hip", "Philox"), body("esn_reservoir.hip", "ResPhilox")
    assert gen == res
    for const in ("0xD2511F53U * c[0]", "0xCD9E8D57U * c[2]", "ka += 0x9E3779B9U", "kb += 0xBB67AE85U", "i < 10"):
        assert const in gen, const
    src = open(os.path.join(ROOT, "esn_ofdm_mimo_amd", "csrc", "esn_gen.hip")).read()
    assert "PURPOSE_BITS = 1, PURPOSE_NOISE = 2, PURPOSE_TAPS = 3, PURPOSE_DOPPLER = 4" in src
    src = open(os.path.join(ROOT, "esn_ofdm_mimo_amd", "csrc", "esn_reservoir.hip")).read()
    assert "RES_PURPOSE_W = 16, RES_PURPOSE_WIN = 17, RES_PURPOSE_WFB = 18" in src


def bits_literal(seed, gf, N, n_t, m):
    """frame_bits one symbol at a time, every index spelled out."""
    spw = 32 // m
    key = (seed & 0xFFFFFFFF, seed >> 32)
    out = np.zeros((N * m, n_t), dtype=np.uint8)
    for sc in range(N):
        for tx in range(n_t):
            e = sc * n_t + tx
            call, r = divmod(e, 4 * spw)
            q, j = divmod(r, spw)
            w = philox_scalar([gf & 0xFFFFFFFF, gf >> 32, 1, call], key)
            idx = (w[q] >> (j * m)) & ((1 << m) - 1)
            for b in range(m):
                out[sc * m + b, tx] = (idx >> b) & 1
    return out


@pytest.mark.parametrize("N,n_t,m", [(8, 4, 4), (8, 3, 6), (16, 4, 2), (4, 1, 10), (64, 1, 2)])
def test_bits_equal_the_literal_restatement(N, n_t, m):
    for gf in (0, pr.FRAME_OFFSET, pr.FRAME_OFFSET + 1):
        got = pr.frame_bits(pr.SEED, gf, N, n_t, m)
        assert got.dtype == np.uint8 and got.shape == (N * m, n_t)
        np.testing.assert_array_equal(got, bits_literal(pr.SEED, gf, N, n_t, m))


def test_other_streams_equal_literal_restatements():
    seed, g = pr.SEED, pr.FRAME_OFFSET + 1
    key = (seed & 0xFFFFFFFF, seed >> 32)
    ctr = lambda purpose, pos: philox_scalar([g & 0xFFFFFFFF, g >> 32, purpose, pos], key)      # noqa: E731
    # noise: antenna 2 of 3 at t = 5 is the even half of pair 1; antenna 1 the odd half of pair 0
    z = pr.frame_noise(seed, g, 9, 3)
    for rx in range(3):
        w = ctr(2, 5 * 2 + (rx >> 1))
        a, b = w[2 * (rx & 1)], w[2 * (rx & 1) + 1]
        rr = np.sqrt(-2.0 * np.log(((a >> 8) + 0.5) / 2 ** 24))
        u2 = (b >> 8) / 2 ** 24
        assert z[5, rx] == complex(rr * np.cos(2 * np.pi * u2), rr * np.sin(2 * np.pi * u2))
    # gains
    gn = pr.link_gains(seed, g, 23)
    w = ctr(3, 22)
    rr = np.sqrt(-2.0 * np.log((w[0] + 0.5) / 2 ** 32))
    assert gn[22] == complex(rr * np.cos(2 * np.pi * (w[1] + 0.5) / 2 ** 32), rr * np.sin(2 * np.pi * (w[1] + 0.5) / 2 ** 32))
    # angles
    an = pr.doppler_angles(seed, g, 8)
    w = ctr(4, 7 * 16 + 9)
    assert an.shape == (8, 16, 2) and an[7, 9, 0] == (w[0] + 0.5) / 2 ** 31 and an[7, 9, 1] == (w[1] + 0.5) / 2 ** 31
    assert (an > 0).all() and (an < 2).all()
    # reservoir uniforms
    n, n_in, n_out = 5, 3, 2
    u = pr.reservoir_uniforms(seed, g, n, n_in, n_out)
    assert u.shape == (2 * n * n + n * n_in + n * n_out,) and (u >= 0).all() and (u < 1).all()
    ru = lambda a, b: ((a >> 5) * 2 ** 26 + (b >> 6)) / 2 ** 53                                   # noqa: E731
    w = ctr(16, 3 * n + 4)
    assert u[3 * n + 4] == ru(w[0], w[1]) and u[n * n + 3 * n + 4] == ru(w[2], w[3])
    w = ctr(17, 4 * n_in + 2)
    assert u[2 * n * n + 4 * n_in + 2] == ru(w[0], w[1])
    w = ctr(18, 4 * n_out + 1)
    assert u[2 * n * n + n * n_in + 4 * n_out + 1] == ru(w[0], w[1])


# ---- every wrong stream is far from the right one at the shapes of the GPU test -----------------------------------------
def differing(stream, right, wrong, m):
    """bool, one entry per SAMPLE: does the wrong stream change it by more than the GPU comparison allows?  Bits
    [count, N, n_t]: a sample is a symbol (the m bits of one subcarrier and transmitter; the comparison is exact, and
    two independent symbols still agree with probability 2^-m).  The others, in the shape of the draws: a complex
    sample, an angle or a uniform changed by more than 1e-4 in some component (1e-4 is the cap on the noise tolerance;
    taps, angles and uniforms are compared far more tightly)."""
    if stream == "bits":
        count, n_t = right.shape[0], right.shape[-1]
        return (right.reshape(count, -1, m, n_t) != wrong.reshape(count, -1, m, n_t)).any(axis=2)
    d = right - wrong
    return np.maximum(np.abs(d.real), np.abs(d.imag)) > 1e-4


def separation_cases():
    F = pr.N_FRAMES
    for N, n_t, m in pr.BITS_SHAPES + pr.BITS_SMALL_N:
        yield "bits", pr.FRAME_OFFSET, F, (N, n_t, m)
    for n_r in pr.NOISE_NR:
        for T in pr.NOISE_T:
            yield "noise", pr.FRAME_OFFSET, F, (T, n_r)
    for kind, isi in pr.TAP_KINDS:
        for n_r, n_t in pr.TAP_ANTENNAS:
            yield "gains", pr.LINK_OFFSET, 3 * n_r * n_t, (pr.tap_paths(kind, isi),)
    for kind in (0, 1):
        yield "angles", pr.LINK_OFFSET, 3 * 2 * 3, (pr.tap_paths(kind, 8),)
    for n_res, n_in, n_out, _ in pr.RES_SHAPES:
        yield "uniforms", pr.FIRST_SET, 2, (n_res, n_in, n_out)


@pytest.mark.parametrize("stream,offset,count,shape", list(separation_cases()),
                         ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_wrong_streams_differ_in_well_over_half_of_the_samples(stream, offset, count, shape):
    """The share is taken over the samples an error can reach at all (philox_ref.reach says which and why: the frame
    whose offset has no high half, the words an exchange does not move).  Outside them the wrong stream IS the right
    one, which is asserted too."""
    m = shape[2] if stream == "bits" else None
    right = pr.draws(stream, pr.SEED, offset, count, *shape)
    wrong = pr.wrong_streams(stream, pr.SEED, offset, count, *shape)
    assert set(wrong) == set(pr.WRONG)
    for name, w in wrong.items():
        assert w.shape == right.shape and w.dtype == right.dtype
        diff = differing(stream, right, w, m)
        sel = pr.reach(stream, name, offset, count, *shape)
        sel = np.broadcast_to(sel.reshape(sel.shape + (1,) * (diff.ndim - sel.ndim)), diff.shape)
        assert sel.any(), (name, "the case must let the error show somewhere")
        assert not diff[~sel].any(), (name, "reach() leaves out samples the error does change")
        share = float(diff[sel].mean())
        # expected: bits 1 - 2^-m >= 0.75 (m = 2: sd 0.03 over the 192 symbols of the smallest case); the others
        # 1 - O(1e-4).  Cases of a few samples (a 1x1 link of one path) get room for one near-coincidence.
        floor = 0.6 if stream == "bits" else (0.99 if sel.sum() >= 400 else 0.9)
        assert share >= floor, f"{stream} {shape}: '{name}' changes only {share:.1%} of the samples (needs {floor:.0%})"


# ---- the model's own draws are what they claim to be --------------------------------------------------------------------
def test_bits_are_balanced_per_bit_position():
    bits = pr.draws("bits", pr.SEED, pr.FRAME_OFFSET, 64, 128, 4, 4).astype(np.float64)      # [64, 512, 4]
    n = bits.size
    assert abs(bits.mean() - 0.5) < 4 * 0.5 / np.sqrt(n)
    per_pos = bits.reshape(64, 128, 4, 4).mean(axis=(0, 1))                                 # [bit, tx]
    assert (np.abs(per_pos - 0.5) < 4 * 0.5 / np.sqrt(n / 16)).all(), per_pos
    b6 = pr.draws("bits", 5, 0, 64, 64, 3, 6).astype(np.float64).reshape(64, 64, 6, 3).mean(axis=(0, 1))
    assert (np.abs(b6 - 0.5) < 4 * 0.5 / np.sqrt(64 * 64)).all(), b6


def test_noise_is_standard_normal_and_the_antennas_of_a_pair_are_independent():
    z = pr.draws("noise", pr.SEED, pr.FRAME_OFFSET, 64, 135, 8)                             # [64, 135, 8]
    n = z.size
    for part in (z.real, z.imag):
        assert abs(part.mean()) < 4 / np.sqrt(n)
        assert abs(part.var() - 1.0) < 4 * np.sqrt(2.0 / n)
        assert abs((part ** 4).mean() - 3.0) < 4 * np.sqrt(96.0 / n)                         # var of x^4 = 105 - 9
    # correlation of independent unit-variance samples: sd 1 / sqrt(n) per coefficient
    e, o = z[..., 0::2].reshape(-1), z[..., 1::2].reshape(-1)
    for a in (e.real, e.imag):
        for b in (o.real, o.imag):
            assert abs(np.mean(a * b)) < 4 / np.sqrt(a.size)
    assert abs(np.mean(z.real * z.imag)) < 4 / np.sqrt(n)
    # neighbours in time and in frame
    assert abs(np.mean(z.real[:, 1:] * z.real[:, :-1])) < 4 / np.sqrt(n)
    assert abs(np.mean(z.real[1:] * z.real[:-1])) < 4 / np.sqrt(n)
    # odd n_r: the same pairs, the last one half used
    z3 = pr.frame_noise(pr.SEED, 9, 71, 3)
    z4 = pr.frame_noise(pr.SEED, 9, 71, 4)
    np.testing.assert_array_equal(z3, z4[:, :3])


def test_gains_angles_and_uniforms_have_their_moments():
    g = pr.draws("gains", pr.SEED, pr.LINK_OFFSET, 2000, 23)
    n = g.size
    for part in (g.real, g.imag):
        assert abs(part.mean()) < 4 / np.sqrt(n) and abs(part.var() - 1.0) < 4 * np.sqrt(2.0 / n)
    assert abs(np.mean(g.real * g.imag)) < 4 / np.sqrt(n)
    a = pr.draws("angles", pr.SEED, pr.LINK_OFFSET, 200, 8)
    assert abs(a.mean() - 1.0) < 4 * np.sqrt(1 / 3.0 / a.size)                               # uniform on [0, 2): var 1/3
    assert abs(np.mean((a[..., 0] - 1) * (a[..., 1] - 1))) < 4 * (1 / 3.0) / np.sqrt(a.size / 2)
    u = pr.reservoir_uniforms(pr.SEED, pr.FIRST_SET, 130, 16, 8)
    assert abs(u.mean() - 0.5) < 4 * np.sqrt(1 / 12.0 / u.size)
    nn = 130 * 130
    assert abs(np.mean((u[:nn] - 0.5) * (u[nn:2 * nn] - 0.5))) < 4 * (1 / 12.0) / np.sqrt(nn)    # value vs mask
