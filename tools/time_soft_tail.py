#!/usr/bin/env python3
"""What the soft tail of the coded leg costs (csrc/esn_soft.hip) at the benchmark's 153 600 frames (N = 128, n_t = 4,
16-QAM, groups of 75) unless told otherwise:

  (a) detect_llr, the fused tail (esn_detect_llr): float64 Y and float32 Y, weights and bias given;
  (b) the unfused pair on the same Y: detect_count(want_xhat=True) (esn_detect_count: the fixed-shape kernel at this
      shape) followed by LdpcCode.llrs(weights, bias) (esn_qam_llr_weighted) -- X_hat written once and read twice;
  (c) a device copy of the fused kernel's bytes: as many bytes read and as many written as (a) reads Y and tx bits and
      writes LLRs, float64 Y;
  (d) mmse_sinr of 2048 blocks (esn_mmse_sinr) beside estimate_channel of the same blocks.

Device events around the calls on preallocated inputs, 3 warm-ups, median of 9, the candidates of a section interleaved
in one process.  The one pass / fail reading: (a) with float64 Y is not slower than (b), both measured in this run; the
ratio and the ratio to the copy are written down whatever they are.  --out FILE also writes the table there
(profiles/soft_tail_time.txt)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from esn_ofdm_mimo_amd import _lib  # noqa: E402
from esn_ofdm_mimo_amd.montecarlo import FrameSource, LinkParams  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=153600)
ap.add_argument("--per-group", type=int, default=75)
ap.add_argument("--sinr-blocks", type=int, default=2048)
ap.add_argument("--out")
a = ap.parse_args()

lib, ptr = _lib.load(), _lib.ptr
prm = LinkParams()
src = FrameSource(prm, seed=1)
dev = src.device
B, F, N, n_t, n_r, m = a.frames, a.per_group, prm.n_sub, prm.n_t, prm.n_r, prm.m
G = (B + F - 1) // F
WARM, REPS, MID = 3, 9, 4
EBNO = 12.0
PI = prm.p_i(EBNO)
stream = _lib.stream_handle()
gen = torch.Generator(device=dev).manual_seed(1)

# Y whose spectrum over N sqrt(Pi) is of the constellation's size: white rows of variance N Pi / 2 per component
Y64 = torch.randn((B, N, 2 * n_t), dtype=torch.float64, device=dev, generator=gen) * (N * PI / 2) ** 0.5
Y32 = Y64.to(torch.float32)
tx = torch.randint(0, 2, (B, N * m, n_t), dtype=torch.uint8, device=dev, generator=gen)
p_i = torch.full((G,), PI, dtype=torch.float64, device=dev)
w = 0.25 + 1.5 * torch.rand((G, N, n_t), dtype=torch.float64, device=dev, generator=gen)
mu = 0.5 + 0.5 * torch.rand((G, N, n_t), dtype=torch.float64, device=dev, generator=gen)
err, nb = (torch.zeros(G, dtype=torch.int64, device=dev) for _ in range(2))
llr = torch.empty((B, n_t, N * m), dtype=torch.float64, device=dev)
llr2 = torch.empty_like(llr)
s2, s2b = (torch.empty(B, dtype=torch.float64, device=dev) for _ in range(2))
xh = torch.empty((B, N, 2 * n_t), dtype=torch.float64, device=dev)
bytes_in, bytes_out = Y64.numel() * 8 + tx.numel(), llr.numel() * 8
n_copy = (bytes_in + bytes_out) // 2
c_src = torch.empty(n_copy, dtype=torch.uint8, device=dev)
c_dst = torch.empty(n_copy, dtype=torch.uint8, device=dev)


def timed(calls):
    """[(name, fn)] -> {name: sorted ms}: interleaved, every repetition runs the calls one after the other."""
    for _ in range(WARM):
        for _, fn in calls:
            fn()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in calls]
          for _ in range(REPS)]
    for r in range(REPS):
        for (s, e), (_, fn) in zip(ev[r], calls):
            s.record(); fn(); e.record()
    torch.cuda.synchronize()
    return {name: sorted(ev[r][i][0].elapsed_time(ev[r][i][1]) for r in range(REPS)) for i, (name, _) in enumerate(calls)}


def row(name, ms, extra=""):
    return f"{name:62s} {ms[MID]:8.3f} ms  ({ms[0]:.3f} .. {ms[-1]:.3f}){extra}"


def fused(Y, name):
    def call():
        _lib.check(getattr(lib, name)(ptr(Y), B, F, N, n_t, m, ptr(p_i), ptr(tx), ptr(err), ptr(nb), ptr(w), ptr(mu),
                                      ptr(llr), ptr(s2), None, stream), name)
    return call


def unfused():
    _lib.check(lib.esn_detect_count(ptr(Y64), B, F, N, n_t, m, ptr(p_i), ptr(tx), ptr(err), ptr(nb), ptr(xh), stream),
               "esn_detect_count")
    _lib.check(lib.esn_qam_llr_weighted(B, F, N, n_t, m, ptr(xh), ptr(w), ptr(mu), ptr(llr2), ptr(s2b), stream),
               "esn_qam_llr_weighted")


def detect_only():
    _lib.check(lib.esn_detect_count(ptr(Y64), B, F, N, n_t, m, ptr(p_i), ptr(tx), ptr(err), ptr(nb), ptr(xh), stream),
               "esn_detect_count")


info = _lib.device_info()
lines = [f"{info['arch']}, {info['cu_count']} CUs; {B} frames in groups of {F}, N = {N}, n_t = {n_t}, {m} bits per symbol; "
         f"device events, {WARM} warm-ups, median (min .. max) of {REPS}, interleaved per section"]
calls = [("detect_llr, float64 Y (fused)", fused(Y64, "esn_detect_llr")),
         ("detect_llr, float32 Y (fused)", fused(Y32, "esn_detect_llr_f32")),
         ("detect_count(X_hat) + llrs(weights, bias) (unfused)", unfused),
         ("  of which detect_count(X_hat)", detect_only),
         ("copy of the fused kernel's bytes (float64 Y)", lambda: c_dst.copy_(c_src))]
t = timed(calls)
f64, f32, unf, det, cpy = (t[name] for name, _ in calls)
lines.append(row(calls[0][0], f64, f"  {(bytes_in + bytes_out) / 1e9 / f64[MID]:.2f} TB/s (Y and tx bits read, LLRs written)"))
lines.append(row(calls[1][0], f32, f"  {(bytes_in - Y64.numel() * 4 + bytes_out) / 1e9 / f32[MID]:.2f} TB/s"))
lines.append(row(calls[2][0], unf))
lines.append(row(calls[3][0], det))
lines.append(row(calls[4][0], cpy, f"  {2 * n_copy / 1e9 / cpy[MID]:.2f} TB/s"))
lines.append(f"    fused / unfused = {f64[MID] / unf[MID]:.3f}   fused / copy = {f64[MID] / cpy[MID]:.3f}   "
             f"fused float32 Y / fused float64 Y = {f32[MID] / f64[MID]:.3f}")
lines.append(f"    per frame: {bytes_in // B} bytes read, {bytes_out // B} written by the fused tail; the unfused pair moves "
             f"{3 * N * n_t * 16} more (X_hat out once, in twice)")
ok = f64[MID] <= unf[MID]
lines.append(f"judged: fused tail (float64 Y) not slower than the unfused pair in the same process: "
             f"{f64[MID]:.3f} ms against {unf[MID]:.3f} ms: " + ("ok" if ok else "MISSED"))
unfused()
fused(Y64, "esn_detect_llr")()
torch.cuda.synchronize()
assert torch.equal(llr, llr2) and torch.equal(s2, s2b), "the two paths disagree"
del c_src, c_dst, xh, llr, llr2, Y64, Y32, tx
torch.cuda.empty_cache()

# (d) the weights: once per block, beside the channel estimate they are computed from
Gs = a.sinr_blocks
d = src.blocks_fast(EBNO, 0, 0, Gs, 1, with_ls_pilot=True)
H = src.estimate_channel(d["pilot_bits"], d["pilot_y_ls"], EBNO)
calls = [(f"mmse_sinr, {Gs} blocks", lambda: src.mmse_sinr(H, EBNO)),
         (f"estimate_channel, {Gs} blocks", lambda: src.estimate_channel(d["pilot_bits"], d["pilot_y_ls"], EBNO))]
t = timed(calls)
for name, _ in calls:
    lines.append(row(name, t[name]))
lines.append(f"    mmse_sinr / estimate_channel = {t[calls[0][0]][MID] / t[calls[1][0]][MID]:.3f}")
print("\n".join(lines))
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
sys.exit(0 if ok else 1)
