#!/usr/bin/env python3
"""Time of the channel-metrics kernel (esn_channel_metrics, csrc/esn_chanstat.hip) at the size of a published run:
5 120 coherence blocks x 512 subcarriers, at 4x8 and at 2x2.  Device events around each launch, warm-up first, median
(and minimum) of the repeats; all in one process, interleaved per repeat:

    metrics      the kernel, outputs preallocated (with and without the optional S output)
    copy         a device-to-device copy of the same H buffer: the yardstick for a kernel that must read H once
    perfect-ZF   esn_zf_detect_count over one data symbol of each of the same blocks: the neighbouring per-subcarrier kernel

    python tools/time_chan_metrics.py [--blocks 5120] [--n-sub 512] [--repeats 9]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from esn_ofdm_mimo_amd import _lib  # noqa: E402
from esn_ofdm_mimo_amd._lib import check, ptr  # noqa: E402
from esn_ofdm_mimo_amd.montecarlo import FrameSource, LinkParams  # noqa: E402


def timed(fns, warmup, repeats):
    """{name: sorted ms list}; the candidates alternate inside every repeat."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        ev = {}
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); f(); b.record()
            ev[k] = (a, b)
        torch.cuda.synchronize()
        for k, (a, b) in ev.items():
            ms[k].append(a.elapsed_time(b))
    return {k: sorted(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5120)
    ap.add_argument("--n-sub", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--ebno", type=float, default=12.0)
    a = ap.parse_args()
    lib = _lib.load()
    print(f"device {_lib.device_info()['arch']}  blocks {a.blocks}  subcarriers {a.n_sub}  Eb/No {a.ebno} dB  "
          f"repeats {a.repeats} (median [min])")
    for n_t, n_r in ((4, 8), (2, 2)):
        prm = LinkParams.block_fading(n_t, n_r, a.n_sub)
        fs = FrameSource(prm, seed=3)
        dev, G, N = fs.device, a.blocks, a.n_sub
        taps = fs.taps(G, 0, 0)
        H = fs.true_channel(taps)
        Hc = torch.empty_like(H)
        bits, _, dy = fs.frames(taps, 1, a.ebno, 0, 0, 1)
        p_i = torch.full((G,), prm.p_i(a.ebno), dtype=torch.float64, device=dev)
        cond = torch.empty((G, N), dtype=torch.float64, device=dev)
        rank = torch.empty((G, N), dtype=torch.uint8, device=dev)
        cap = torch.empty((G,), dtype=torch.float64, device=dev)
        S = torch.empty((G, N, min(n_t, n_r)), dtype=torch.float64, device=dev)
        err = torch.zeros(G, dtype=torch.int64, device=dev)
        nb = torch.zeros(G, dtype=torch.int64, device=dev)
        st = _lib.stream_handle()

        def metrics(s=None):
            check(lib.esn_channel_metrics(G, N, n_t, n_r, ptr(H), ptr(p_i), prm.no, ptr(s), ptr(cond), ptr(rank),
                                          ptr(cap), st), "esn_channel_metrics")

        def zf():
            check(lib.esn_zf_detect_count(G, 1, N, prm.cp, n_t, n_r, prm.m, ptr(p_i), ptr(H), ptr(dy), ptr(bits),
                                          ptr(err), ptr(nb), None, st), "esn_zf_detect_count")

        ms = timed({"metrics": metrics, "metrics + S": lambda: metrics(S), "copy of H": lambda: Hc.copy_(H),
                    "perfect-ZF, 1 symbol": zf}, warmup=3, repeats=a.repeats)
        hb = H.numel() * 16
        print(f"{n_t}x{n_r} (n_t x n_r): {G * N} matrices, H {hb / 2**20:.1f} MiB")
        for k, v in ms.items():
            med = v[len(v) // 2]
            rate = f"  H bytes / time {hb / med / 1e6:8.1f} GB/s" if k != "perfect-ZF, 1 symbol" else ""
            extra = f"  ({G * N / med / 1e3:.1f} M matrices/s)" if k.startswith("metrics") else ""
            print(f"  {k:22s} {med:8.3f} ms [{v[0]:8.3f}]{rate}{extra}")
        full = float(rank.ge(min(n_t, n_r)).double().mean())
        print(f"  full-rank fraction {full:.4f}  mean capacity {float(cap.mean()):.4f} bit/subcarrier  "
              f"median cond {float(cond.median()):.3f}")
        del H, Hc, dy, bits, S, cond
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
