#!/usr/bin/env python3
"""Times of the windowed CNN (esn_cnn_train / esn_cnn_predict, csrc/esn_cnn.hip) at 4x8, N = 128 (T = 138 rows, 16
inputs, 8 outputs), channels 32 and 64, kernel 5, 50 epochs, beside the windowed FNN on the same pilots.  Device events
around each launch, 3 warm-ups, median (and minimum) of the repeats; all in one process, interleaved per repeat.

Training, the benchmark's 2048 pilots:
    cnn train          esn_cnn_train, one launch
    fnn train          esn_fnn_train of the same pilots (100 hidden units, window 8), one launch
    copy               a device-to-device copy of the bytes the training reads (U + D)
  with the model TFLOP/s of both: the CNN's FLOP count per epoch and pilot is 2 T (2 sum_l K_l c_l + K_2 c_2 + K_3 c_3),
  K_l = k c_{l-1} (forward and weight gradients of all layers, input gradients of layers 2 and 3); the FNN's is
  |R| (4 K H + 6 H n_out).
Prediction, the 153 600 data frames of 12 800 blocks (block b reads trained set b mod pilots):
    cnn f64            esn_cnn_predict
    fnn f64            esn_fnn_predict
    copy               a device-to-device copy of the bytes of the frames

    python tools/time_cnn.py [--pilots 2048] [--blocks 12800] [--frames 12] [--repeats 9] [--ebno 21] [--epochs 50]
                             [--out profiles/cnn_time.txt]
"""
import argparse
import dataclasses
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from esn_ofdm_mimo_amd import _lib  # noqa: E402
from esn_ofdm_mimo_amd.cnn import NAMES, CnnBank  # noqa: E402
from esn_ofdm_mimo_amd import fnn as fnn_mod  # noqa: E402
from esn_ofdm_mimo_amd.fnn import FnnBank  # noqa: E402
from esn_ofdm_mimo_amd.montecarlo import FrameSource, LinkParams, _view_real  # noqa: E402
from esn_ofdm_mimo_amd.points import cnn_weights, fnn_weights  # noqa: E402
from time_chan_metrics import timed  # noqa: E402

F64_MATRIX_PEAK = 78.6e12
CHANNELS, KERNEL, HIDDEN, WINDOW = (32, 64), 5, 100, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pilots", type=int, default=2048)
    ap.add_argument("--blocks", type=int, default=12800)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--ebno", type=float, default=21.0)
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cnn_time.txt"))
    a = ap.parse_args()
    prm = dataclasses.replace(LinkParams(), coherence_fixed=a.frames)
    src = FrameSource(prm, seed=1234)
    dev, G, F, P = src.device, a.blocks, a.frames, min(a.pilots, a.blocks)
    B, T, n_in, n_out = G * F, prm.t_frame + prm.delay, 2 * prm.n_r, 2 * prm.n_t
    data = src.blocks_fast(a.ebno, 0, 0, G, F)
    U = _view_real(data["data_y"]).reshape(B, prm.t_frame, n_in)
    Ut = torch.zeros((P, T, n_in), dtype=torch.float64, device=dev)
    Dt = torch.zeros((P, T, n_out), dtype=torch.float64, device=dev)
    Ut[:, :prm.t_frame] = _view_real(data["pilot_y"])[:P]
    Dt[:, prm.delay:] = _view_real(data["pilot_x"])[:P]
    scale = 1.0 / np.sqrt(prm.var_x(a.ebno))

    def scaled(bank, g):
        bank.set_scaling(torch.full((g, n_in), scale, dtype=torch.float64, device=dev), None,
                         torch.full((g, n_out), scale, dtype=torch.float64, device=dev), None)
        return bank

    # ---- training of P pilots
    cnn = scaled(CnnBank(n_in, n_out, CHANNELS, KERNEL, n_groups=P), P)
    fnn = scaled(FnnBank(n_in, n_out, HIDDEN, WINDOW, n_groups=P), P)
    c_init = cnn_weights(CHANNELS, KERNEL, n_in, n_out, 0)
    f_init = fnn_weights(HIDDEN, WINDOW * n_in, n_out, 0)
    f_tr = max(prm.forget, WINDOW - 1)
    moved_t = (Ut.numel() + Dt.numel()) * 8
    src_t = torch.empty(moved_t // 2, dtype=torch.uint8, device=dev)
    dst_t = torch.empty_like(src_t)
    ms_t = timed({"cnn train": lambda: cnn.train(Ut, Dt, c_init, transient=prm.forget, epochs=a.epochs),
                  "fnn train": lambda: fnn.train(Ut, Dt, f_init, transient=f_tr, epochs=a.epochs),
                  "copy, bytes of U + D": lambda: dst_t.copy_(src_t)}, warmup=3, repeats=a.repeats)
    c = (n_in,) + CHANNELS + (n_out,)
    mac = [KERNEL * c[l] * c[l + 1] for l in range(3)]
    flop = {"cnn train": float(P) * a.epochs * 2.0 * T * (2.0 * sum(mac) + mac[1] + mac[2]),
            "fnn train": float(P) * a.epochs * (T - f_tr) * (4.0 * WINDOW * n_in * HIDDEN + 6.0 * HIDDEN * n_out)}

    # ---- prediction of B frames, block b reading set b mod P
    idx = torch.arange(G, device=dev) % P
    big_c = scaled(CnnBank(n_in, n_out, CHANNELS, KERNEL, n_groups=G), G)
    big_c.set_weights(*[getattr(cnn, n)[idx] for n in NAMES])
    big_f = scaled(FnnBank(n_in, n_out, HIDDEN, WINDOW, n_groups=G), G)
    big_f.set_weights(*[getattr(fnn, n)[idx] for n in fnn_mod.NAMES])
    Yc = torch.empty((B, prm.n_sub, n_out), dtype=torch.float64, device=dev)
    Yf = torch.empty_like(Yc)
    src_p = torch.empty(U.numel() * 8 // 2, dtype=torch.uint8, device=dev)
    dst_p = torch.empty_like(src_p)
    ms_p = timed({"cnn f64": lambda: big_c.predict(U, F, T=T, transient=prm.forget, out=Yc),
                  "fnn f64": lambda: big_f.predict(U, F, T=T, transient=prm.forget, out=Yf),
                  "copy, bytes of the frames": lambda: dst_p.copy_(src_p)}, warmup=3, repeats=a.repeats)
    flop_p = float(B) * 2.0 * T * sum(mac)

    med_t = {k: v[len(v) // 2] for k, v in ms_t.items()}
    med_p = {k: v[len(v) // 2] for k, v in ms_p.items()}
    rate = {k: flop[k] / med_t[k] / 1e9 for k in flop}
    lines = [f"device {_lib.device_info()['arch']}  {prm.n_t}x{prm.n_r}  N {prm.n_sub}  T {T}  channels {CHANNELS}  "
             f"kernel {KERNEL}  epochs {a.epochs}  Eb/No {a.ebno} dB  repeats {a.repeats} (median [min])",
             f"training of {P} pilots: CNN {flop['cnn train'] / 1e9:.1f} GFLOP, "
             f"{flop['cnn train'] / F64_MATRIX_PEAK * 1e3:.3f} ms at the float64 matrix-pipe peak "
             f"({F64_MATRIX_PEAK / 1e12:.1f} TFLOP/s); FNN ({HIDDEN} units, window {WINDOW}) "
             f"{flop['fnn train'] / 1e9:.1f} GFLOP; {moved_t / 2 ** 20:.1f} MiB of U + D"]
    for k, v in ms_t.items():
        lines.append(f"  {k:28s} {med_t[k]:9.3f} ms [{v[0]:9.3f}]" + (f"  {rate[k]:8.2f} TFLOP/s" if k in rate else ""))
    lines.append(f"cnn TFLOP/s / fnn TFLOP/s: {rate['cnn train'] / rate['fnn train']:.2f};  cnn train / time at the "
                 f"matrix-pipe peak: {med_t['cnn train'] / (flop['cnn train'] / F64_MATRIX_PEAK * 1e3):.1f};  "
                 f"cnn train / fnn train: {med_t['cnn train'] / med_t['fnn train']:.2f}")
    lines.append(f"prediction of {G} blocks x {F} frames = {B} frames: CNN {flop_p / 1e9:.1f} GFLOP, "
                 f"{U.numel() * 8 / 2 ** 20:.1f} MiB of frames")
    for k, v in ms_p.items():
        lines.append(f"  {k:28s} {med_p[k]:9.3f} ms [{v[0]:9.3f}]"
                     + (f"  {flop_p / med_p[k] / 1e9:8.2f} TFLOP/s" if k == "cnn f64" else ""))
    lines.append(f"cnn / fnn: {med_p['cnn f64'] / med_p['fnn f64']:.2f};  cnn / copy: "
                 f"{med_p['cnn f64'] / med_p['copy, bytes of the frames']:.1f}")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
