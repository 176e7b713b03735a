#!/usr/bin/env python3
"""Time of the fused windowed-ELM prediction (esn_elm_predict, csrc/esn_elm.hip) on the benchmark's chunk: 153 600 data
frames of 12 800 blocks at 4x8, N = 128 (T = 138 rows, 16 inputs, 8 outputs), 512 hidden units over a window of 8 rows,
beside the ESN's prediction of the same frames.  Device events around each launch, 3 warm-ups, median (and minimum) of
the repeats; all in one process, interleaved per repeat:

    elm f16, elm f64   esn_elm_predict on the frames, read-out fitted on the blocks' pilots, Y preallocated
    esn f16            esn_predict_batch (N_res 512, fp16, counter noise) on the same frames: what bench.py times
    copy               a device-to-device copy that reads and writes, together, the bytes a prediction reads (U) and
                       writes (Y): the yardstick of a kernel bound by its frames

    python tools/time_elm.py [--blocks 12800] [--frames 12] [--repeats 9] [--ebno 21] [--hidden 512] [--window 8]
"""
import argparse
import dataclasses
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from esn_ofdm_mimo_amd import _lib  # noqa: E402
from esn_ofdm_mimo_amd.elm import ElmBank  # noqa: E402
from esn_ofdm_mimo_amd.montecarlo import DetectorSweep, LinkParams, _view_real  # noqa: E402
from esn_ofdm_mimo_amd.points import elm_weights  # noqa: E402
from time_chan_metrics import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=12800)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--ebno", type=float, default=21.0)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--gain", type=float, default=0.05)
    a = ap.parse_args()
    prm = dataclasses.replace(LinkParams(), coherence_fixed=a.frames)
    sweep = DetectorSweep(prm, n_reservoir=512, noise=0.001, seed=1234, precision="f16", fit_precision="f16")
    dev, G, F = sweep.device, a.blocks, a.frames
    B, T, n_in, n_out = G * F, prm.t_frame + prm.delay, 2 * prm.n_r, 2 * prm.n_t
    data = sweep.src.blocks_fast(a.ebno, 0, 0, G, F)
    sweep.set_snr(a.ebno, G)
    sweep.train(data["pilot_y"], data["pilot_x"], seed=1)
    U = _view_real(data["data_y"]).reshape(B, prm.t_frame, n_in)
    y_esn = torch.empty((B, prm.n_sub, n_out), dtype=torch.float64, device=dev)

    W_in, b = elm_weights(a.hidden, a.window * n_in, a.gain, 0)
    bank = ElmBank(n_in, n_out, a.hidden, a.window, W_in, b, n_groups=G)
    scale = 1.0 / np.sqrt(prm.var_x(a.ebno))
    bank.set_scaling(torch.full((G, n_in), scale, dtype=torch.float64, device=dev), None,
                     torch.full((G, n_out), scale, dtype=torch.float64, device=dev), None)
    Up = torch.zeros((G, T, n_in), dtype=torch.float64, device=dev)
    Dp = torch.zeros((G, T, n_out), dtype=torch.float64, device=dev)
    Up[:, :prm.t_frame] = _view_real(data["pilot_y"])
    Dp[:, prm.delay:] = _view_real(data["pilot_x"])
    bank.fit(Up, Dp, transient=max(prm.forget, a.window - 1), method="auto")
    y_elm = {p: torch.empty((B, prm.n_sub, n_out), dtype=torch.float64, device=dev) for p in ("f16", "f64")}
    moved = U.numel() * 8 + y_esn.numel() * 8
    src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)

    def elm(p):
        bank.predict(U, F, T=T, transient=prm.forget, precision=p, out=y_elm[p])

    def esn():
        sweep.bank.predict(U, F, T=T, transient=prm.forget, precision="f16", noise_mode="counter", seed=1, out=y_esn)

    ms = timed({"elm f16": lambda: elm("f16"), "elm f64": lambda: elm("f64"), "esn f16": esn,
                "copy, bytes of U + Y": lambda: dst.copy_(src)}, warmup=3, repeats=a.repeats)
    rel = float((y_elm["f16"] - y_elm["f64"]).abs().max() / y_elm["f64"].abs().max())
    flop = 2.0 * T * (a.window * n_in * a.hidden + (a.hidden + 1) * n_out) * B
    print(f"device {_lib.device_info()['arch']}  {prm.n_t}x{prm.n_r}  N {prm.n_sub}  T {T}  {G} blocks x {F} frames = {B} "
          f"frames  hidden {a.hidden}  window {a.window}  Eb/No {a.ebno} dB  repeats {a.repeats} (median [min])")
    print(f"bytes read + written per launch (U + Y): {moved / 2**30:.2f} GiB; ELM {flop / B / 1e6:.1f} MFLOP per frame; "
          f"max |Y f16 - Y f64| / max |Y f64| = {rel:.2e}")
    med = {k: v[len(v) // 2] for k, v in ms.items()}
    for k, v in ms.items():
        rate = f"  {flop / med[k] / 1e9:8.1f} TFLOP/s" if k.startswith("elm") else ""
        print(f"  {k:22s} {med[k]:9.3f} ms [{v[0]:9.3f}]  {moved / med[k] / 1e6:8.1f} GB/s{rate}")
    print(f"elm f16 / esn f16 (medians): {med['elm f16'] / med['esn f16']:.3f};  elm f16 / copy: "
          f"{med['elm f16'] / med['copy, bytes of U + Y']:.2f};  elm f64 / elm f16: {med['elm f64'] / med['elm f16']:.1f}")


if __name__ == "__main__":
    main()
