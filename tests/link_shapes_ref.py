"""What tests/test_gpu_link_shapes.py and tests/test_link_shapes_reference_cpu.py share: the ragged shapes at which the
link-level OFDM kernels (gen_frames_kernel, channel_estimate_kernel, mmse_detect_kernel, taps_to_freq_kernel) are held to
oracle/, the supplied inputs of every shape (made once, never changed), the two conditions that keep exact error counts
honest (slicer margin, conditioning), and NumPy restatements of the kernels' steps with the mutants the shapes must tell
from the oracle.  No GPU, no torch.

The references themselves are the oracle's functions (modulate, lfilter, pilot_frames, estimate_channel, linear_detect,
taps_to_freq, hard_bits); the restatements here exist for the mutants alone and are themselves held to the oracle by the CPU
module before a mutant's distance is read."""
import dataclasses
import functools
import math
from typing import NamedTuple, Optional

import numpy as np
from scipy import signal

from oracle import esn_oracle as eo
from oracle.baselines import estimate_channel, linear_detect, pilot_frames, taps_to_freq
from oracle.ofdm_frames import LinkConfig, exp_pdp_taps, make_frame, modulate

EBNO = 15.0
G, F = 2, 2                      # blocks per case, data frames per block

# the project's own bounds (tests/test_gpu_framegen.py, test_gpu_baseline.py, test_gpu_blockfading.py)
GEN_BOUND = 1e-12                # x_cp, y_cp: of max|.| per frame
H_BOUND = 1e-10                  # H: of max|H| per block
XHAT_BOUND = 1e-9                # X_hat: of max|X_hat| per frame
TAPS_FREQ_BOUND = 1e-12          # taps_to_freq: absolute
MARGIN_MIN = 1e-7                # slicer margin of a counted X_hat: 100 x XHAT_BOUND
COND_MAX = 1e4                   # cond(H_k^H H_k + lambda I): 10 cond 2^-52 stays three orders under XHAT_BOUND
MMSE_NT = 4                      # transmit antennas the detector kernel serves
LDS_MAX = 150 * 1024             # dynamic LDS a workgroup of these kernels may ask for


class Case(NamedTuple):
    n_t: int
    n_r: int
    n_sub: int
    m: int
    isi: int
    cp: Optional[int] = None     # None: isi - 1, as every driver has it

    def __str__(self):
        return "x".join(str(v) for v in self if v is not None)


# Leg A (n_t, n_r, N, m, isi) -> what else the case runs
GEN_CASES = [Case(1, 3, 8, 2, 1), Case(3, 5, 64, 6, 3), Case(2, 6, 32, 8, 16), Case(4, 8, 1024, 4, 8),
             Case(2, 4, 2048, 4, 8)]
GEN_LS_PATTERN = [Case(3, 5, 64, 6, 3), Case(1, 3, 8, 2, 1)]
GEN_C64 = [Case(3, 5, 64, 6, 3), Case(1, 3, 8, 2, 1), Case(2, 6, 32, 8, 16)]
GEN_REJECTED = Case(4, 8, 2048, 4, 8)                    # 283,072 bytes of LDS

# Leg B.  The last three are additions: (4,6,256,6,5) and (3,3,16,4,8) are counted in leg C; (4,4,2048,4,8) is the N = 2048
# shape the DETECTOR admits (147,456 bytes; n_r = 8 needs 278,528 and is rejected), so leg C keeps N = 2048;
# (2,3,32,4,4, cp = 9) is the one shape with cp + 1 != isi, without which the prior's normalisation (over cp + 1 taps, not
# isi) cannot be seen: every LinkConfig has cp = isi - 1
EST_CASES = [Case(1, 1, 8, 2, 2), Case(3, 5, 64, 6, 3), Case(3, 2, 32, 4, 4), Case(1, 3, 512, 2, 16),
             Case(2, 3, 1024, 8, 8), Case(4, 2, 128, 4, 64), Case(2, 2, 16, 4, 1), Case(4, 8, 2048, 4, 8),
             Case(4, 6, 256, 6, 5), Case(3, 3, 16, 4, 8), Case(4, 4, 2048, 4, 8), Case(2, 3, 32, 4, 4, 9)]
# Leg C: the blocks of leg B.  The detector's LDS is 16 (n_r N + N/2) bytes
DET_REJECTED = Case(4, 8, 2048, 4, 8)
DET_CASES = [c for c in EST_CASES if c != DET_REJECTED]
MARGIN_CASES = EST_CASES                                 # the reference's margin is measured for the rejected shape too
# Leg D (n_t, n_r, N, isi)
TAPS_CASES = [(3, 5, 8, 1), (1, 1, 2048, 16), (2, 3, 64, 3)]
TAPS_BIG = (4, 8, 2048, 2, 257)                          # + blocks: 16,842,752 outputs > 65535 x 256 = 16,776,960


@dataclasses.dataclass
class WideCpConfig(LinkConfig):
    """A LinkConfig whose cyclic prefix is longer than isi - 1."""
    cp_fixed: int = 0

    @property
    def cp(self):
        return self.cp_fixed


def config(case):
    kw = dict(n_t=case.n_t, n_r=case.n_r, n_sub=case.n_sub, m=case.m, isi=case.isi)
    return LinkConfig(**kw) if case.cp is None else WideCpConfig(cp_fixed=case.cp, **kw)


def gen_lds_bytes(c):
    t = c.n_sub + (c.isi - 1 if c.cp is None else c.cp)
    return 16 * (c.n_t * c.n_sub + c.n_t * t + c.n_sub // 2 + c.n_r * c.n_t * c.isi)


def est_lds_bytes(c):
    return 16 * (2 * c.n_sub + c.n_sub // c.n_t + 1 + c.isi + c.n_sub // 2)


def det_lds_bytes(c):
    return 16 * (c.n_r * c.n_sub + c.n_sub // 2)


# ---- supplied inputs, made once per case --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gen_inputs(case):
    """Leg A: taps [G, n_r, n_t, isi], bits [G F, N m, n_t] uint8, noise [G F, T, n_r] (unit complex normals pairs)."""
    cfg = config(case)
    rs = np.random.RandomState(1000 + case.n_sub + case.n_t + case.isi)
    t = cfg.n_sub + cfg.cp
    taps = np.stack([exp_pdp_taps(cfg, rs) for _ in range(G)])
    bits = (rs.rand(G * F, cfg.n_sub * cfg.m, cfg.n_t) > 0.5).astype(np.uint8)
    noise = rs.randn(G * F, t, cfg.n_r) + 1j * rs.randn(G * F, t, cfg.n_r)
    for a in (taps, bits, noise):
        a.setflags(write=False)
    return dict(cfg=cfg, taps=taps, bits=bits, noise=noise)


def modulate_points(x_f, cfg, ebno):
    """oracle.ofdm_frames.modulate from the constellation points on: (x_cp pre-PA, x_cp post-PA).  Its own statements, so
    that the sparse LS pattern (points off the comb zeroed, as pilot_frames zeroes them) goes through the same chain."""
    x_t = cfg.n_sub * np.fft.ifft(x_f, axis=0)
    x_cp = np.concatenate([x_t[-cfg.cp:], x_t], axis=0) * math.sqrt(cfg.p_i(ebno)) \
        if cfg.cp > 0 else x_t * math.sqrt(cfg.p_i(ebno))
    return x_cp, x_cp / np.sqrt(1 + (np.abs(x_cp) / cfg.a_clip(ebno)) ** 2)


def generator_reference(cfg, ebno, bits, taps, noise, ls_pattern=False):
    """One frame of the generator from oracle.modulate and scipy's lfilter: (x_cp [T, n_t], y_cp [T, n_r])."""
    x_f, x_cp, x_pa = modulate(bits.astype(np.int32), cfg, ebno)
    if ls_pattern:
        on = (np.arange(cfg.n_sub)[:, None] % cfg.n_t) == np.arange(cfg.n_t)[None, :]
        x_cp, x_pa = modulate_points(np.where(on, x_f, 0), cfg, ebno)
    t = x_pa.shape[0]
    y = np.zeros((t, cfg.n_r), dtype=np.complex128)
    for rx in range(cfg.n_r):
        for tx in range(cfg.n_t):
            y[:, rx] += signal.lfilter(taps[rx, tx], np.array([1]), x_pa[:, tx])
        y[:, rx] += math.sqrt(t * cfg.no / 2) * noise[:, rx]
    return x_cp, y


@functools.lru_cache(maxsize=None)
def link_blocks(case):
    """Legs B and C: G blocks of (taps, the oracle's pilot pair, F data frames) from RandomState(N + n_t), and the oracle's
    channel estimates.  Arrays: taps [G, n_r, n_t, isi], pilot_bits [G, N m, n_t], X_LS [G, N, n_t], y_ls_cp [G, T, n_r],
    H / H_ls [G, N, n_r, n_t], H_true, data_bits [G F, N m, n_t], data_y [G F, T, n_r]."""
    cfg = config(case)
    rs = np.random.RandomState(case.n_sub + case.n_t)
    taps, pil, data = [], [], []
    for _ in range(G):
        taps.append(exp_pdp_taps(cfg, rs))
        pil.append(pilot_frames(cfg, EBNO, taps[-1], rs))
        data += [make_frame(cfg, EBNO, taps[-1], rs) for _ in range(F)]
    out = dict(cfg=cfg, taps=np.stack(taps),
               pilot_bits=np.stack([p["bits"] for p in pil]).astype(np.uint8),
               X_LS=np.stack([p["X_LS"] for p in pil]), y_ls_cp=np.stack([p["y_ls_cp"] for p in pil]),
               y_cp=np.stack([p["y_cp"] for p in pil]),
               H=np.stack([estimate_channel(cfg, EBNO, p["X_LS"], p["y_ls_cp"]) for p in pil]),
               H_ls=np.stack([estimate_channel(cfg, EBNO, p["X_LS"], p["y_ls_cp"], ls_only=True) for p in pil]),
               H_true=np.stack([taps_to_freq(cfg, t) for t in taps]),
               data_bits=np.stack([d["bits"] for d in data]).astype(np.uint8),
               data_y=np.stack([d["y_cp"] for d in data]))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def detect_reference(cfg, H, data_y, data_bits, zf):
    """linear_detect of every frame under its block's H [G, N, n_r, n_t]: (X_hat [G F, N, n_t], errors per block [G])."""
    const = eo.unit_qam(cfg.m)
    xs, errs = [], np.zeros(H.shape[0], dtype=np.int64)
    for i in range(data_y.shape[0]):
        x = linear_detect(cfg, EBNO, H[i // F], data_y[i], reg=0 if zf else None)
        xs.append(x)
        errs[i // F] += eo.count_bit_errors(data_bits[i], eo.hard_bits(x, const, cfg.m))
    return np.stack(xs), errs


# ---- the two conditions behind exact counts ---------------------------------------------------------------------------
def slicer_margin(x_hat, m):
    """Per frame of x_hat [B, N, n_t]: the least distance of a Re or Im part from a slicer boundary (midway between two
    neighbouring levels of the unit-power grid), over that frame's max|X_hat|."""
    side = 1 << (m // 2)
    norm = math.sqrt(2.0 * (side * side - 1) / 3.0)
    bounds = np.arange(-(side - 2), side - 1, 2) / norm                    # side - 1 boundaries per axis
    out = []
    for x in x_hat:
        v = np.concatenate([x.real.ravel(), x.imag.ravel()])
        out.append(np.abs(v[:, None] - bounds[None, :]).min() / np.abs(x).max())
    return np.array(out)


def worst_cond(H, lam):
    """max over blocks and subcarriers of cond(H_k^H H_k + lam I), H [G, N, n_r, n_t]."""
    g = np.conj(np.swapaxes(H, -1, -2)) @ H + lam * np.eye(H.shape[-1])
    return float(np.linalg.cond(g).max())


def mmse_lambda(cfg):
    return cfg.no / cfg.p_i(EBNO)


# ---- restatements of the kernels' steps, and their mutants ------------------------------------------------------------
def generator_restated(cfg, ebno, bits, taps, noise, mutant=None):
    """gen_frames_kernel's channel as the kernel walks it: per receive group of four antennas and time sample, the FIR
    over x_pa with zero initial state plus noise, stored into the flat [T n_r] frame.
    mutant "circular": x_pa[t - k] wraps round the frame instead of reading zero before its start.
    mutant "dup_rx": a group's dead slots (antenna index >= n_r) are stored too, holding antenna n_r - 1 (the clamped
    read): they land on the next time sample's first antennas.  Groups are taken in order, so the last group's dead
    stores win, as they would whenever its wave runs last."""
    _, x_cp, x_pa = modulate(bits.astype(np.int32), cfg, ebno)
    t_len, n_r = x_pa.shape[0], cfg.n_r
    y = np.zeros((t_len, n_r), dtype=np.complex128)
    for rx in range(n_r):
        for tx in range(cfg.n_t):
            for k in range(cfg.isi):
                xs = np.roll(x_pa[:, tx], k)
                if mutant != "circular":
                    xs[:k] = 0
                y[:, rx] += taps[rx, tx, k] * xs
        y[:, rx] += math.sqrt(t_len * cfg.no / 2) * noise[:, rx]
    if mutant == "dup_rx":
        flat = np.zeros(t_len * n_r + 4, dtype=np.complex128)
        for rx0 in range(0, n_r, 4):
            for q in range(4):
                flat[np.arange(t_len) * n_r + rx0 + q] = y[:, min(rx0 + q, n_r - 1)]
        y = flat[:t_len * n_r].reshape(t_len, n_r)
    return x_cp, y


def estimate_restated(cfg, ebno, x_ls, y_ls_cp, ls_only=False, mutant=None):
    """channel_estimate_kernel's steps: LS on each transmitter's comb, linear interpolation between comb points with the
    first / last interval extended outwards, IFFT cut to isi taps, shrinkage by the exponential prior, DFT back.
    mutant "short_comb": N // n_t comb points for every tx instead of ceil((N - tx) / n_t).
    mutant "held_tail": behind the last comb point the estimate is held instead of extrapolated.
    mutant "prior_isi": the prior is normalised over isi taps instead of cp + 1."""
    n, n_t, isi, p_i = cfg.n_sub, cfg.n_t, cfg.isi, cfg.p_i(ebno)
    yf = np.fft.fft(y_ls_cp[cfg.cp:], axis=0) / n
    tc = max(cfg.cp / 9, 1e-12)
    r_h = np.exp(-np.arange(isi) / tc) / np.exp(-np.arange(isi if mutant == "prior_isi" else cfg.cp + 1) / tc).sum()
    gain = 1.0 / (((cfg.no / p_i) / (n / 2)) / r_h + 1.0)
    k = np.arange(n)
    h = np.zeros((n, cfg.n_r, n_t), dtype=np.complex128)
    for tx in range(n_t):
        n_p = n // n_t if mutant == "short_comb" else -((tx - n) // n_t)
        sc = tx + n_t * np.arange(n_p)
        hls = yf[sc] / (x_ls[sc, tx] * math.sqrt(p_i) + 1e-12)[:, None]
        i = np.clip((k - tx) // n_t, 0, max(n_p - 2, 0))
        w = (k - (tx + n_t * i)) / n_t
        if mutant == "held_tail":
            w = np.minimum(w, 1.0)
        lo, hi = hls[i], hls[i + 1] if n_p > 1 else hls[i]
        full = lo + w[:, None] * (hi - lo)
        if ls_only:
            h[:, :, tx] = full
        else:
            h[:, :, tx] = np.fft.fft(np.fft.ifft(full, axis=0)[:isi] * gain[:, None], n, axis=0)
    return h


def slice_restated(x_hat, m, mutant=None):
    """det_slice per axis and the natural-binary labels, [N m, n_t] like oracle.hard_bits.
    mutant "truncate": the level index is cut towards zero instead of rounded to nearest."""
    side = 1 << (m // 2)
    norm = math.sqrt(2.0 * (side * side - 1) / 3.0)

    def level(v):
        a = (v * norm + (side - 1)) * 0.5
        return np.clip(np.trunc(a) if mutant == "truncate" else np.rint(a), 0, side - 1).astype(int)

    idx = level(x_hat.real) * side + level(x_hat.imag)
    bits = (idx[:, :, None] >> np.arange(m)[None, None, :]) & 1
    return bits.transpose(0, 2, 1).reshape(x_hat.shape[0] * m, x_hat.shape[1])
