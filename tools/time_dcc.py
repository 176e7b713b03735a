#!/usr/bin/env python3
"""What the amplifier-aware LS-MMSE detector costs (csrc/esn_dcc.hip) at the benchmark's 153 600 frames (4x8, N = 128,
cp = 7, 16-QAM, groups of 75) unless told otherwise:

  (a) esn_mmse_detect_count with X_hat written: the kernel whose work every cancellation pass repeats in part;
  (b) esn_mmse_dcc_detect_count with X_hat written at n_iter = 0, 1, 2, 3, and n_iter = 2 with err_iter counted too;
  (c) a device copy of the kernel's bytes: as many read as (b) reads frames and bits, as many written as X_hat.

Device events around the calls on preallocated inputs, 3 warm-ups, median of 9, the candidates interleaved in one process.
The one pass / fail reading: t(n_iter = 2) <= 3 t(a) -- a pass repeats at most (a)'s transform rows (2 n_t <= n_r) and its
solve and has no global traffic, so 1 + n_iter is the operation-count bound.  --out FILE also writes the table there
(profiles/dcc_time.txt)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from esn_ofdm_mimo_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=153600)
ap.add_argument("--per-group", type=int, default=75)
ap.add_argument("--n-sub", type=int, default=128)
ap.add_argument("--cp", type=int, default=7)
ap.add_argument("--n-t", type=int, default=4)
ap.add_argument("--n-r", type=int, default=8)
ap.add_argument("--m", type=int, default=4)
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
a_clip = torch.full((G,), (N * PI) ** 0.5 * 10 ** (3.0 / 20), dtype=torch.float64, device=dev)
err = torch.zeros(G, dtype=torch.int64, device=dev)
nb = torch.zeros(G, dtype=torch.int64, device=dev)
it = torch.zeros((G, 9), dtype=torch.int64, device=dev)
xh = torch.empty((B, N, n_t), dtype=torch.complex128, device=dev)
x0 = torch.empty((B, N, n_t), dtype=torch.complex128, device=dev)
n_copy = (y.numel() * 16 + tx.numel() + xh.numel() * 16) // 2
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


def detect(out=xh):
    _lib.check(lib.esn_mmse_detect_count(B, F, N, cp, n_t, n_r, m, ptr(p_i), NO, ptr(H), ptr(y), ptr(tx), ptr(err),
                                         ptr(nb), ptr(out), stream), "esn_mmse_detect_count")


def dcc(n_iter, counts=False):
    def call():
        _lib.check(lib.esn_mmse_dcc_detect_count(B, F, N, cp, n_t, n_r, m, n_iter, ptr(p_i), ptr(a_clip), NO, ptr(H),
                                                 ptr(y), ptr(tx), ptr(err), ptr(nb), ptr(it) if counts else None, ptr(xh),
                                                 stream), "esn_mmse_dcc_detect_count")
    return call


info = _lib.device_info()
lines = [f"{info['arch']}, {info['cu_count']} CUs; {B} frames in groups of {F}, N = {N}, cp = {cp}, {n_t}x{n_r}, m = {m}; "
         f"device events, {WARM} warm-ups, median (min .. max) of {REPS}, interleaved; LDS per workgroup "
         f"{lib.esn_mmse_dcc_lds_bytes(N, n_t, n_r)} bytes"]
calls = [("mmse_detect_count with X_hat", detect)] + \
        [(f"mmse_dcc_detect_count with X_hat, n_iter = {k}", dcc(k)) for k in range(4)] + \
        [("mmse_dcc_detect_count with X_hat and err_iter, n_iter = 2", dcc(2, True)),
         ("copy of the kernel's bytes", lambda: c_dst.copy_(c_src))]
t = timed(calls)
for name, _ in calls:
    ms = t[name]
    lines.append(f"{name:62s} {ms[MID]:8.3f} ms  ({ms[0]:.3f} .. {ms[-1]:.3f})")
det, two = t[calls[0][0]][MID], t[calls[3][0]][MID]
per_pass = (t[calls[4][0]][MID] - t[calls[1][0]][MID]) / 3
lines.append(f"    a pass costs {per_pass:.3f} ms = {per_pass / det:.2f} of mmse_detect_count; copy: "
             f"{2 * n_copy / 1e9 / t[calls[-1][0]][MID]:.2f} TB/s")
ok = two <= 3 * det
lines.append(f"judged: t(n_iter = 2) <= 3 t(mmse_detect_count with X_hat): {two:.3f} ms against 3 x {det:.3f} = {3 * det:.3f} ms "
             f"(ratio {two / det:.2f}): " + ("ok" if ok else "MISSED"))
detect(x0)
dcc(0)()
torch.cuda.synchronize()
assert torch.equal(torch.view_as_real(x0), torch.view_as_real(xh))             # no pass: the detector, bit for bit
print("\n".join(lines))
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
sys.exit(0 if ok else 1)
