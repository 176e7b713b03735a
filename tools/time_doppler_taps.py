#!/usr/bin/env python3
"""What fading="jakes" adds to a sweep chunk: the Doppler tap launch (esn_gen_taps_doppler, 2048 blocks x 76 symbols,
4x8 TDL-B: the benchmark's chunk with its pilot symbol) beside the data-frame launch it feeds (esn_gen_frames, 2048 x 75
frames, one tap set per frame), and for scale the two launches of block fading (esn_gen_taps, esn_gen_frames with 75
frames per tap set).  Device events around the bare library calls on preallocated outputs, 3 warm-ups, median of 9, the
four launches interleaved in one process.  --out FILE also writes the table there (profiles/doppler_taps_time.txt)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from esn_ofdm_mimo_amd import _lib  # noqa: E402
from esn_ofdm_mimo_amd.montecarlo import FrameSource, LinkParams  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=2048)
ap.add_argument("--frames", type=int, default=75)
ap.add_argument("--io", choices=("c128", "c64"), default="c128")
ap.add_argument("--out")
a = ap.parse_args()

p = LinkParams(fading="jakes")
src = FrameSource(p, seed=1)
lib, dev, ptr = src.lib, src.device, _lib.ptr
G, F, EBNO = a.blocks, a.frames, 12.0
B = G * F
cdt = torch.complex64 if a.io == "c64" else torch.complex128
gen = lib.esn_gen_frames_c64 if a.io == "c64" else lib.esn_gen_frames
taps_sym = torch.empty((G, 1 + F, p.n_r, p.n_t, p.isi), dtype=torch.complex128, device=dev)
taps_blk = torch.empty((G, p.n_r, p.n_t, p.isi), dtype=torch.complex128, device=dev)
bits = torch.empty((B, p.n_sub * p.m, p.n_t), dtype=torch.uint8, device=dev)
y_cp = torch.empty((B, p.t_frame, p.n_r), dtype=cdt, device=dev)
pi_f = torch.full((B,), p.p_i(EBNO), dtype=torch.float64, device=dev)
ac_f = torch.full((B,), p.a_clip(EBNO), dtype=torch.float64, device=dev)
stream = _lib.stream_handle()


def doppler_taps():
    _lib.check(lib.esn_gen_taps_doppler(0, G, 1 + F, p.n_r, p.n_t, p.isi, p.fs, p.ds_ns, p.fd_tsym, None, 7, 0,
                                        ptr(taps_sym), stream), "esn_gen_taps_doppler")


def block_taps():
    _lib.check(lib.esn_gen_taps(0, G, p.n_r, p.n_t, p.isi, p.fs, p.ds_ns, None, 7, 0, ptr(taps_blk), stream),
               "esn_gen_taps")


def frames(taps, per_block):
    _lib.check(gen(B, per_block, p.n_sub, p.cp, p.n_t, p.n_r, p.isi, p.m, 0, ptr(pi_f), ptr(ac_f), p.no, ptr(taps),
                   None, None, 9, 0, ptr(bits), None, ptr(y_cp), stream), "esn_gen_frames")


doppler_taps()
block_taps()
data_taps = taps_sym[:, 1:].reshape(B, p.n_r, p.n_t, p.isi).contiguous()
calls = [("jakes: taps, %d blocks x %d symbols" % (G, 1 + F), doppler_taps),
         ("jakes: data frames, one tap set per frame", lambda: frames(data_taps, 1)),
         ("block: taps, %d blocks" % G, block_taps),
         ("block: data frames, %d per tap set" % F, lambda: frames(taps_blk, F))]
WARM, REPS = 3, 9
for _ in range(WARM):
    for _, fn in calls:
        fn()
ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in calls] for _ in range(REPS)]
for r in range(REPS):                      # interleaved: every repetition runs the four launches one after the other
    for (s, e), (_, fn) in zip(ev[r], calls):
        s.record(); fn(); e.record()
torch.cuda.synchronize()
info = _lib.device_info()
lines = [f"{info['arch']}, {info['cu_count']} CUs; 4x8 TDL-B, N = {p.n_sub}, fd_tsym = {p.fd_tsym:.5f}; {B} data frames, "
         f"{a.io}; device events, {WARM} warm-ups, median (min .. max) of {REPS}, interleaved"]
med = {}
for i, (name, _) in enumerate(calls):
    ms = sorted(ev[r][i][0].elapsed_time(ev[r][i][1]) for r in range(REPS))
    med[i] = ms[REPS // 2]
    lines.append(f"{name:44s} {ms[REPS // 2]:8.3f} ms  ({ms[0]:.3f} .. {ms[-1]:.3f})")
lines.append(f"taps / data frames under jakes = {med[0] / med[1]:.3f} (goal: at most 1); a jakes chunk's generator "
             f"costs {med[0] + med[1] - med[2] - med[3]:+.3f} ms more than a block chunk's")
print("\n".join(lines))
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
