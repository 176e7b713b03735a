#!/usr/bin/env python3
"""Times of the LSTM comparator (esn_lstm_train / esn_lstm_predict, csrc/esn_lstm.hip) at 4x8, N = 128 (T = 138 rows, 16
inputs, 8 outputs), 100 hidden units, 50 epochs, beside the windowed CNN and FNN on the same pilots and the reference's
own training loop.  Device events around each launch, 3 warm-ups, median (and minimum) of the repeats; all in one
process, interleaved per repeat.

Training, the benchmark's 2048 pilots:
    lstm train         esn_lstm_train, one launch
    cnn train          esn_cnn_train of the same pilots (channels 32 and 64, kernel 5), one launch
    fnn train          esn_fnn_train of the same pilots (100 hidden units, window 8), one launch
    torch loop         the reference's loop (:93-113) -- torch.nn.LSTM + Linear + optim.Adam, 50 epochs, MSE -- in float64
                       on the same device over --torch-pilots of the same pilots one after another (one warm-up pilot,
                       host clock around a synchronise), scaled to the 2048
  The pass / fail reading: lstm train for 2048 pilots below 2048 x the torch loop's time per pilot.  Recorded beside it:
  the model TFLOP/s with FLOPs = 6 . 4H (H + n_in + 1) T + 6 H n_out T per group and epoch, and the microseconds per serial
  step = time / (waves of workgroups x epochs x 2 T), waves = ceil(pilots / CUs) (one workgroup per CU).
Prediction, the 153 600 data frames of 12 800 blocks (block b reads trained set b mod pilots):
    lstm f64           esn_lstm_predict
    cnn f64            esn_cnn_predict
    fnn f64            esn_fnn_predict
    copy               a device-to-device copy of the bytes of the frames
  and the time the LSTM's 2 . 4H (H + n_in + 1) T + 2 H n_out T FLOPs per frame take at the float64 matrix-pipe peak.

    python tools/time_lstm.py [--pilots 2048] [--blocks 12800] [--frames 12] [--repeats 9] [--ebno 21] [--epochs 50]
                              [--torch-pilots 4] [--out profiles/lstm_time.txt]
"""
import argparse
import dataclasses
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from esn_ofdm_mimo_amd import _lib  # noqa: E402
from esn_ofdm_mimo_amd import cnn as cnn_mod  # noqa: E402
from esn_ofdm_mimo_amd import fnn as fnn_mod  # noqa: E402
from esn_ofdm_mimo_amd import lstm as lstm_mod  # noqa: E402
from esn_ofdm_mimo_amd.cnn import CnnBank  # noqa: E402
from esn_ofdm_mimo_amd.fnn import FnnBank  # noqa: E402
from esn_ofdm_mimo_amd.lstm import LstmBank  # noqa: E402
from esn_ofdm_mimo_amd.montecarlo import FrameSource, LinkParams, _view_real  # noqa: E402
from esn_ofdm_mimo_amd.points import cnn_weights, fnn_weights, lstm_weights  # noqa: E402
from time_chan_metrics import timed  # noqa: E402

F64_MATRIX_PEAK = 78.6e12
H, CHANNELS, KERNEL, HIDDEN, WINDOW = 100, (32, 64), 5, 100, 8


def torch_loop(x, d, init, epochs, lr=0.01):
    """The reference's training of one pilot (:93-113) in float64 on x's device: x [T, n_in] and d [T, n_out] scaled."""
    n_in, n_out = x.shape[1], d.shape[1]
    net = torch.nn.LSTM(n_in, H, batch_first=True).double().to(x.device)
    fc = torch.nn.Linear(H, n_out).double().to(x.device)
    prm = [net.weight_ih_l0, net.weight_hh_l0, net.bias_ih_l0, net.bias_hh_l0, fc.weight, fc.bias]
    with torch.no_grad():
        for t, a in zip(prm, init):
            t.copy_(torch.as_tensor(a, device=x.device))
    opt = torch.optim.Adam(prm, lr=lr)
    loss_fn = torch.nn.MSELoss()
    for _ in range(epochs):
        opt.zero_grad()
        loss = loss_fn(fc(net(x[None])[0]), d[None])
        loss.backward()
        opt.step()
    return prm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pilots", type=int, default=2048)
    ap.add_argument("--blocks", type=int, default=12800)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--ebno", type=float, default=21.0)
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--torch-pilots", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_time.txt"))
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
    lstm = scaled(LstmBank(n_in, n_out, H, n_groups=P), P)
    cnn = scaled(CnnBank(n_in, n_out, CHANNELS, KERNEL, n_groups=P), P)
    fnn = scaled(FnnBank(n_in, n_out, HIDDEN, WINDOW, n_groups=P), P)
    l_init = lstm_weights(H, n_in, n_out, 0)
    c_init = cnn_weights(CHANNELS, KERNEL, n_in, n_out, 0)
    f_init = fnn_weights(HIDDEN, WINDOW * n_in, n_out, 0)
    f_tr = max(prm.forget, WINDOW - 1)
    ms_t = timed({"lstm train": lambda: lstm.train(Ut, Dt, l_init, transient=prm.forget, epochs=a.epochs),
                  "cnn train": lambda: cnn.train(Ut, Dt, c_init, transient=prm.forget, epochs=a.epochs),
                  "fnn train": lambda: fnn.train(Ut, Dt, f_init, transient=f_tr, epochs=a.epochs)},
                 warmup=3, repeats=a.repeats)
    # the reference's loop, a pilot at a time (its loss runs over every row: the same work per step)
    per_pilot = []
    for g in range(a.torch_pilots + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch_loop(Ut[g % P] * scale, Dt[g % P] * scale, l_init, a.epochs)
        torch.cuda.synchronize()
        per_pilot.append((time.perf_counter() - t0) * 1e3)
    per_pilot = sorted(per_pilot[1:])                       # the first is the warm-up
    torch_ms = per_pilot[len(per_pilot) // 2]
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    waves = -(-P // cus)
    flop_l = float(P) * a.epochs * (6.0 * 4 * H * (H + n_in + 1) * T + 6.0 * H * n_out * T)

    # ---- prediction of B frames, block b reading set b mod P
    idx = torch.arange(G, device=dev) % P
    big_l = scaled(LstmBank(n_in, n_out, H, n_groups=G), G)
    big_l.set_weights(*[getattr(lstm, n)[idx] for n in lstm_mod.NAMES])
    big_c = scaled(CnnBank(n_in, n_out, CHANNELS, KERNEL, n_groups=G), G)
    big_c.set_weights(*[getattr(cnn, n)[idx] for n in cnn_mod.NAMES])
    big_f = scaled(FnnBank(n_in, n_out, HIDDEN, WINDOW, n_groups=G), G)
    big_f.set_weights(*[getattr(fnn, n)[idx] for n in fnn_mod.NAMES])
    Y = [torch.empty((B, prm.n_sub, n_out), dtype=torch.float64, device=dev) for _ in range(3)]
    src_p = torch.empty(U.numel() * 8 // 2, dtype=torch.uint8, device=dev)
    dst_p = torch.empty_like(src_p)
    ms_p = timed({"lstm f64": lambda: big_l.predict(U, F, T=T, transient=prm.forget, out=Y[0]),
                  "cnn f64": lambda: big_c.predict(U, F, T=T, transient=prm.forget, out=Y[1]),
                  "fnn f64": lambda: big_f.predict(U, F, T=T, transient=prm.forget, out=Y[2]),
                  "copy, bytes of the frames": lambda: dst_p.copy_(src_p)}, warmup=3, repeats=a.repeats)
    flop_p = float(B) * (2.0 * 4 * H * (H + n_in + 1) * T + 2.0 * H * n_out * T)

    med_t = {k: v[len(v) // 2] for k, v in ms_t.items()}
    med_p = {k: v[len(v) // 2] for k, v in ms_p.items()}
    lt = med_t["lstm train"]
    lines = [f"device {_lib.device_info()['arch']} ({cus} CUs)  {prm.n_t}x{prm.n_r}  N {prm.n_sub}  T {T}  hidden {H}  "
             f"epochs {a.epochs}  Eb/No {a.ebno} dB  repeats {a.repeats} (median [min])",
             f"training of {P} pilots: LSTM {flop_l / 1e9:.1f} GFLOP, {flop_l / F64_MATRIX_PEAK * 1e3:.3f} ms at the float64 "
             f"matrix-pipe peak ({F64_MATRIX_PEAK / 1e12:.1f} TFLOP/s)"]
    for k, v in ms_t.items():
        lines.append(f"  {k:28s} {med_t[k]:10.3f} ms [{v[0]:10.3f}]"
                     + (f"  {flop_l / lt / 1e9:8.2f} TFLOP/s" if k == "lstm train" else ""))
    lines.append(f"  {'torch loop, per pilot':28s} {torch_ms:10.3f} ms [{per_pilot[0]:10.3f}]  ({a.torch_pilots} pilots one "
                 f"after another, float64, same device)  x {P} = {torch_ms * P:.0f} ms")
    lines.append(f"lstm train / ({P} x torch loop per pilot): {lt / (torch_ms * P):.5f}  -> "
                 + ("PASS: the batched kernel beats the reference's loop" if lt < torch_ms * P else "FAIL: it loses to it")
                 + f";  lstm train / cnn train: {lt / med_t['cnn train']:.2f};  lstm train / fnn train: "
                   f"{lt / med_t['fnn train']:.2f}")
    lines.append(f"serial step: {lt * 1e3 / (waves * a.epochs * 2 * T):.3f} us = time / ({waves} waves of workgroups x "
                 f"{a.epochs} epochs x {2 * T} steps)")
    lines.append(f"prediction of {G} blocks x {F} frames = {B} frames: LSTM {flop_p / 1e9:.1f} GFLOP, "
                 f"{flop_p / F64_MATRIX_PEAK * 1e3:.3f} ms at the float64 matrix-pipe peak; {U.numel() * 8 / 2 ** 20:.1f} MiB "
                 f"of frames")
    for k, v in ms_p.items():
        lines.append(f"  {k:28s} {med_p[k]:10.3f} ms [{v[0]:10.3f}]"
                     + (f"  {flop_p / med_p[k] / 1e9:8.2f} TFLOP/s" if k == "lstm f64" else ""))
    lines.append(f"lstm / cnn: {med_p['lstm f64'] / med_p['cnn f64']:.2f};  lstm / fnn: "
                 f"{med_p['lstm f64'] / med_p['fnn f64']:.2f};  lstm / copy: "
                 f"{med_p['lstm f64'] / med_p['copy, bytes of the frames']:.1f};  lstm / time at the matrix-pipe peak: "
                 f"{med_p['lstm f64'] / (flop_p / F64_MATRIX_PEAK * 1e3):.1f}")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
