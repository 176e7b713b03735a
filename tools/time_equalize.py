#!/usr/bin/env python3
"""What the equaliser's time-domain rows cost (csrc/esn_equalize.hip) at the benchmark's 153 600 frames (4x8, N = 128,
cp = 7, groups of 75) unless told otherwise:

  (a) esn_mmse_equalize_rows with float64 and with float32 rows (no X_hat);
  (b) esn_mmse_detect_count with X_hat written: the kernel whose front half it shares;
  (c) the unfused path built from existing pieces: that X_hat -> torch.fft.ifft -> scale by N sqrt(Pi) -> cat the cyclic
      prefix -> pad -> Re/Im interleaved;
  (d) a device copy of the kernel's bytes: as many bytes read and as many written as (a) reads frames and writes rows;
  (e) what follows the rows at N_res = 8: predict over all frames and fit over one pilot per group, per precision.

Device events around the calls on preallocated inputs, 3 warm-ups, median of 9, the candidates of a section interleaved
in one process.  The one pass / fail reading: (a) with float64 rows is faster than (c).  --out FILE also writes the
table there (profiles/equalize_time.txt)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from esn_ofdm_mimo_amd import _lib  # noqa: E402
from esn_ofdm_mimo_amd.batched import ReservoirBank  # noqa: E402
from esn_ofdm_mimo_amd.sweep import draw_reservoir  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=153600)
ap.add_argument("--per-group", type=int, default=75)
ap.add_argument("--n-sub", type=int, default=128)
ap.add_argument("--cp", type=int, default=7)
ap.add_argument("--n-t", type=int, default=4)
ap.add_argument("--n-r", type=int, default=8)
ap.add_argument("--m", type=int, default=4)
ap.add_argument("--n-res", type=int, default=8)
ap.add_argument("--skip-recurrence", action="store_true", help="leave section (e) out")
ap.add_argument("--out")
a = ap.parse_args()

lib, ptr = _lib.load(), _lib.ptr
dev = torch.device("cuda:%d" % torch.cuda.current_device())
B, F, N, cp, n_t, n_r, m = a.frames, a.per_group, a.n_sub, a.cp, a.n_t, a.n_r, a.m
G, T = (B + F - 1) // F, a.n_sub + a.cp
WARM, REPS, MID = 3, 9, 4
NO, PI = 1e-5, 1e-5 * 10 ** 2.1
stream = _lib.stream_handle()
gen = torch.Generator(device=dev).manual_seed(1)


def cplx(*shape, scale=1.0):
    return torch.view_as_complex(torch.randn(shape + (2,), dtype=torch.float64, device=dev, generator=gen) * scale)


H = cplx(G, N, n_r, n_t, scale=0.5)
y = cplx(B, T, n_r, scale=(N * PI) ** 0.5)
tx = torch.randint(0, 2, (B, N * m, n_t), dtype=torch.uint8, device=dev, generator=gen)
p_i = torch.full((G,), PI, dtype=torch.float64, device=dev)
err = torch.zeros(G, dtype=torch.int64, device=dev)
nb = torch.zeros(G, dtype=torch.int64, device=dev)
rows64 = torch.empty((B, T, 2 * n_t), dtype=torch.float64, device=dev)
rows32 = torch.empty((B, T, 2 * n_t), dtype=torch.float32, device=dev)
xh = torch.empty((B, N, n_t), dtype=torch.complex128, device=dev)
n_copy = (y.numel() * 16 + rows64.numel() * 8) // 2
c_src = torch.empty(n_copy, dtype=torch.uint8, device=dev)
c_dst = torch.empty(n_copy, dtype=torch.uint8, device=dev)
amp = N * PI ** 0.5


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


def kernel64():
    _lib.check(lib.esn_mmse_equalize_rows(B, F, N, cp, 0, n_t, n_r, ptr(p_i), NO, ptr(H), ptr(y), ptr(rows64), None,
                                          stream), "esn_mmse_equalize_rows")


def kernel32():
    _lib.check(lib.esn_mmse_equalize_rows_f32(B, F, N, cp, 0, n_t, n_r, ptr(p_i), NO, ptr(H), ptr(y), ptr(rows32), None,
                                              stream), "esn_mmse_equalize_rows_f32")


def detect():
    _lib.check(lib.esn_mmse_detect_count(B, F, N, cp, n_t, n_r, m, ptr(p_i), NO, ptr(H), ptr(y), ptr(tx), ptr(err),
                                         ptr(nb), ptr(xh), stream), "esn_mmse_detect_count")


def unfused():
    detect()
    z = torch.fft.ifft(xh, dim=1) * amp
    zc = torch.cat([z[:, N - cp:], z], dim=1) if cp else z
    return torch.view_as_real(zc.contiguous()).reshape(B, T, 2 * n_t)


info = _lib.device_info()
lines = [f"{info['arch']}, {info['cu_count']} CUs; {B} frames in groups of {F}, N = {N}, cp = {cp}, {n_t}x{n_r}; device "
         f"events, {WARM} warm-ups, median (min .. max) of {REPS}, interleaved per section"]
calls = [("equalize_rows, float64 rows", kernel64), ("equalize_rows, float32 rows", kernel32),
         ("mmse_detect_count with X_hat", detect), ("unfused: X_hat -> ifft -> scale -> cat CP -> interleave", unfused),
         ("copy of the kernel's bytes (float64 rows)", lambda: c_dst.copy_(c_src))]
t = timed(calls)
k64, k32, det, unf, cpy = (t[name] for name, _ in calls)
gb_in, gb_out = y.numel() * 16 / 1e9, rows64.numel() * 8 / 1e9
lines.append(row(calls[0][0], k64, f"  {(gb_in + gb_out) / k64[MID]:.2f} TB/s (frames read + rows written)"))
lines.append(row(calls[1][0], k32, f"  {(gb_in + gb_out / 2) / k32[MID]:.2f} TB/s"))
lines.append(row(calls[2][0], det))
lines.append(row(calls[3][0], unf))
lines.append(row(calls[4][0], cpy, f"  {2 * n_copy / 1e9 / cpy[MID]:.2f} TB/s"))
lines.append(f"    kernel / unfused = {k64[MID] / unf[MID]:.3f}   kernel / mmse_detect_count = {k64[MID] / det[MID]:.3f}   "
             f"kernel / copy = {k64[MID] / cpy[MID]:.3f}")
# per frame: n_r + n_t transforms of N log2 N / 2 butterflies (10 flops each) and N solves; against 16 T n_r + 16 T n_t bytes
log2n = N.bit_length() - 1
bfly = (n_r + n_t) * (N // 2) * log2n
solve_flops = N * (n_r * (8 * n_t + 8 * n_t * n_t) + 8 * n_t ** 3 // 3 + 40 * n_t)
lines.append(f"    per frame: {16 * T * n_r + 16 * T * n_t} bytes against {bfly} butterflies in LDS and about "
             f"{(10 * bfly + solve_flops) / 1e3:.0f} kflop float64: the copy is the bytes' bound, what stands above it is "
             f"the transforms and the solve")
ok = k64[MID] < unf[MID]
lines.append(f"judged: kernel (float64 rows) faster than the unfused path in the same process: "
             f"{k64[MID]:.3f} ms against {unf[MID]:.3f} ms: " + ("ok" if ok else "MISSED"))
torch.testing.assert_close(unfused(), rows64, rtol=0, atol=1e-9 * float(rows64.abs().max()))   # the two paths agree
del c_src, c_dst, xh, tx
torch.cuda.empty_cache()

if not a.skip_recurrence:
    # (e) what follows the rows: the ESN at N_res = 8 reads 2 n_t columns and writes 2 n_t
    n_io, n = 2 * n_t, a.n_res
    bank = ReservoirBank(n_io, n_io, n, *draw_reservoir(n_io, n_io, n, 0.9, 0.1, 17), noise=0.001, device=dev)
    bank.set_scaling(np.full((G, n_io), 0.005 / (N * PI) ** 0.5), None, np.full((G, n_io), 5e-7), None)
    Up = rows64[::F][:G].contiguous()
    Dp = torch.randn((G, T, n_io), dtype=torch.float64, device=dev, generator=gen) * (N * PI) ** 0.5
    Y64 = torch.empty((B, N, n_io), dtype=torch.float64, device=dev)
    Y32 = torch.empty((B, N, n_io), dtype=torch.float32, device=dev)
    for label, fn in (
            (f"fit, N_res = {n}, float64 harvest + ridge solve, {G} pilots",
             lambda: bank.fit(Up, Dp, transient=cp, precision="f64", method="auto", ridge=1e-5)),
            (f"predict, N_res = {n}, float64 kernel, float64 rows",
             lambda: bank.predict(rows64, F, transient=cp, precision="f64", out=Y64)),
            (f"predict, N_res = {n}, float32 MFMA kernel, float32 rows",
             lambda: bank.predict(rows32, F, transient=cp, precision="f32", io="f32", out=Y32)),
            (f"predict, N_res = {n}, fp16 MFMA kernel, float32 rows",
             lambda: bank.predict(rows32, F, transient=cp, precision="f16", io="f32", out=Y32))):
        try:
            lines.append(row(label, timed([(label, fn)])[label]))
        except (_lib.EsnHipError, ValueError) as e:          # a precision that does not serve so small a reservoir
            lines.append(f"{label:62s} not served: {e}")
print("\n".join(lines))
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
sys.exit(0 if ok else 1)
