#!/usr/bin/env python3
"""What decide-and-re-modulate costs beside the tail it extends: esn_detect_remod (csrc/esn_remod.hip: two transforms,
Y in and D_hat out) against esn_detect_count on its generic kernel (detect_fixed = "0") and, for scale, on the
fixed-shape kernel, on the same Y -- 153 600 frames of the benchmark's shape (N = 128, n_t = 4, 16-QAM, cp 7, delay 3)
unless told otherwise.  Device events around the bare library calls on preallocated outputs, 3 warm-ups, median of 9,
the launches interleaved in one process.  The goal: at most 2x the generic tail (about twice the bytes, two
transforms).  --out FILE also writes the table there (profiles/detect_remod_time.txt)."""
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
ap.add_argument("--n-t", type=int, default=4)
ap.add_argument("--m", type=int, default=4)
ap.add_argument("--cp", type=int, default=7)
ap.add_argument("--delay", type=int, default=3)
ap.add_argument("--out")
a = ap.parse_args()

lib, ptr = _lib.load(), _lib.ptr
dev = torch.device("cuda:%d" % torch.cuda.current_device())
B, F, N, n_t, m = a.frames, a.per_group, a.n_sub, a.n_t, a.m
G = (B + F - 1) // F
gen = torch.Generator(device=dev).manual_seed(1)
Y = torch.randn((B, N, 2 * n_t), dtype=torch.float64, device=dev, generator=gen) * (N * 0.1) ** 0.5
tx = torch.randint(0, 2, (B, N * m, n_t), dtype=torch.uint8, device=dev, generator=gen)
p_i = torch.full((G,), 0.1, dtype=torch.float64, device=dev)
err = torch.zeros(G, dtype=torch.int64, device=dev)
nb = torch.zeros(G, dtype=torch.int64, device=dev)
D_hat = torch.empty((B, a.delay + a.cp + N, 2 * n_t), dtype=torch.float64, device=dev)
stream = _lib.stream_handle()


def count(knob):
    def fn():
        _lib.debug_set("detect_fixed", knob)
        _lib.check(lib.esn_detect_count(ptr(Y), B, F, N, n_t, m, ptr(p_i), ptr(tx), ptr(err), ptr(nb), None, stream),
                   "esn_detect_count")
    return fn


def remod(with_tx):
    def fn():
        _lib.check(lib.esn_detect_remod(ptr(Y), B, F, N, a.cp, a.delay, n_t, m, ptr(p_i), ptr(tx) if with_tx else None,
                                        ptr(err), ptr(nb), None, None, ptr(D_hat), stream), "esn_detect_remod")
    return fn


KNOB0 = os.environ.get("ESN_DETECT_FIXED", "1")          # what the process started with; put back at the end
calls = [("esn_detect_count, generic kernel", count("0")), ("esn_detect_count, fixed-shape kernel", count("1")),
         ("esn_detect_remod, counting", remod(True)), ("esn_detect_remod, tx_bits NULL", remod(False))]
WARM, REPS = 3, 9
try:
    for _ in range(WARM):
        for _, fn in calls:
            fn()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in calls]
          for _ in range(REPS)]
    for r in range(REPS):                  # interleaved: every repetition runs the launches one after the other
        for (s, e), (_, fn) in zip(ev[r], calls):
            s.record(); fn(); e.record()
    torch.cuda.synchronize()
finally:
    _lib.debug_set("detect_fixed", KNOB0)
info = _lib.device_info()
in_gb = (Y.numel() * 8 + tx.numel()) / 1e9
out_gb = D_hat.numel() * 8 / 1e9
lines = [f"{info['arch']}, {info['cu_count']} CUs; {B} frames in groups of {F}, N = {N}, n_t = {n_t}, m = {m}, cp = {a.cp}, "
         f"delay = {a.delay}; Y + tx_bits {in_gb:.3f} GB, D_hat {out_gb:.3f} GB; device events, {WARM} warm-ups, "
         f"median (min .. max) of {REPS}, interleaved"]
med = {}
for i, (name, _) in enumerate(calls):
    ms = sorted(ev[r][i][0].elapsed_time(ev[r][i][1]) for r in range(REPS))
    med[i] = ms[REPS // 2]
    lines.append(f"{name:40s} {ms[REPS // 2]:8.3f} ms  ({ms[0]:.3f} .. {ms[-1]:.3f})")
lines.append(f"remod (counting) / generic tail = {med[2] / med[0]:.3f} (goal: at most 2); / fixed-shape tail = "
             f"{med[2] / med[1]:.3f}; remod moves {(in_gb + out_gb) / med[2]:.2f} TB/s")
print("\n".join(lines))
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
