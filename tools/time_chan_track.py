#!/usr/bin/env python3
"""Time of the decision-directed channel estimate (esn_channel_track, csrc/esn_chantrack.hip) on the benchmark's chunk:
153 600 estimates at 4x8, N = 128, 16-QAM, isi 8, from the frames of 12 800 Jakes blocks of 12 data symbols, at window 1
and at window 2 (estimate e reads frame e and its successor).  Device events around each launch, 3 warm-ups, median (and
minimum) of the repeats; all in one process, interleaved per repeat:

    track W=1, W=2   the kernel on the detector's X_hat (and, W=1, on the transmitted bits); H, status preallocated
    mmse detect      esn_mmse_detect_count on the same frames with one H per frame and X_hat written: the detector the
                     tracker feeds in baseline_tracking_point
    copy             a device-to-device copy that reads and writes, together, the bytes the W=1 / W=2 launch reads and
                     writes (y rows past the prefix, X_hat, H): the yardstick of a kernel bound by its stores of H

    python tools/time_chan_track.py [--blocks 12800] [--frames 12] [--repeats 9] [--ebno 21]
"""
import argparse
import dataclasses
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from esn_ofdm_mimo_amd import _lib  # noqa: E402
from esn_ofdm_mimo_amd._lib import check, ptr  # noqa: E402
from esn_ofdm_mimo_amd.montecarlo import FrameSource, LinkParams  # noqa: E402
from time_chan_metrics import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=12800)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--ebno", type=float, default=21.0)
    a = ap.parse_args()
    lib = _lib.load()
    prm = dataclasses.replace(LinkParams(), coherence_fixed=a.frames, fading="jakes", f_d=100.0)
    fs = FrameSource(prm, seed=3)
    dev, G, F, N = fs.device, a.blocks, a.frames, prm.n_sub
    B = G * F
    d = fs.blocks_fast(a.ebno, 0, 0, G, F, with_ls_pilot=True)
    H0 = fs.estimate_channel(d["pilot_bits"], d["pilot_y_ls"], a.ebno).repeat_interleave(F, dim=0).contiguous()
    y, bits = d["data_y"], d["data_bits"]
    _, _, xh = fs.mmse_detect_count(H0, y, bits, 1, a.ebno, want_xhat=True)
    pair = lambda t: torch.stack([t, t.roll(-1, 0)], dim=1).reshape(2 * B, *t.shape[1:]).contiguous()
    y2, xh2 = pair(y), pair(xh)
    p_i = torch.full((B,), prm.p_i(a.ebno), dtype=torch.float64, device=dev)
    reg = torch.tensor(fs.track_prior(a.ebno), dtype=torch.float64, device=dev).repeat(B, 1).contiguous()
    H = torch.empty((B, N, prm.n_r, prm.n_t), dtype=torch.complex128, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    xo = torch.empty_like(xh)
    err = torch.zeros(B, dtype=torch.int64, device=dev)
    nb = torch.zeros(B, dtype=torch.int64, device=dev)
    st = _lib.stream_handle()
    moved = {w: B * 16 * (w * N * (prm.n_r + prm.n_t) + N * prm.n_r * prm.n_t) for w in (1, 2)}
    src = {w: torch.empty(moved[w] // 2, dtype=torch.uint8, device=dev) for w in (1, 2)}
    dst = {w: torch.empty_like(src[w]) for w in (1, 2)}

    def track(yy, w, x=None, b=None):
        check(lib.esn_channel_track(ptr(yy), ptr(x), ptr(b), B, w, 1, N, prm.cp, prm.n_t, prm.n_r, prm.isi, prm.m,
                                    ptr(p_i), ptr(reg), None, ptr(H), ptr(status), st), "esn_channel_track")

    def mmse():
        check(lib.esn_mmse_detect_count(B, 1, N, prm.cp, prm.n_t, prm.n_r, prm.m, ptr(p_i), prm.no, ptr(H0), ptr(y),
                                        ptr(bits), ptr(err), ptr(nb), ptr(xo), st), "esn_mmse_detect_count")

    ms = timed({"track W=1 (X_hat)": lambda: track(y, 1, x=xh), "track W=1 (bits)": lambda: track(y, 1, b=bits),
                "track W=2 (X_hat)": lambda: track(y2, 2, x=xh2), "mmse detect, H per frame": mmse,
                "copy, bytes of W=1": lambda: dst[1].copy_(src[1]), "copy, bytes of W=2": lambda: dst[2].copy_(src[2])},
               warmup=3, repeats=a.repeats)
    print(f"device {_lib.device_info()['arch']}  {prm.n_t}x{prm.n_r}  N {N}  isi {prm.isi}  {prm.m} bits/symbol  "
          f"{G} blocks x {F} symbols = {B} estimates  Eb/No {a.ebno} dB  repeats {a.repeats} (median [min])")
    print(f"bytes read + written per launch: W=1 {moved[1] / 2**30:.2f} GiB, W=2 {moved[2] / 2**30:.2f} GiB; "
          f"flagged estimates in the last launch: {int((status != 0).sum())}")
    for k, v in ms.items():
        med = v[len(v) // 2]
        w = 2 if "W=2" in k else 1
        rate = "" if k.startswith("mmse") else f"  {moved[w] / med / 1e6:8.1f} GB/s"
        print(f"  {k:26s} {med:8.3f} ms [{v[0]:8.3f}]{rate}")
    t1, md = ms["track W=1 (X_hat)"], ms["mmse detect, H per frame"]
    print(f"tracker / detector (medians): W=1 {t1[len(t1) // 2] / md[len(md) // 2]:.2f}, "
          f"W=2 {ms['track W=2 (X_hat)'][len(t1) // 2] / md[len(md) // 2]:.2f}")


if __name__ == "__main__":
    main()
