#!/usr/bin/env python3
"""Times of the windowed FNN (esn_fnn_train, csrc/esn_fnn.hip; esn_fnn_predict, the ReLU instantiations of
csrc/esn_elm.hip) at 4x8, N = 128 (T = 138 rows, 16 inputs, 8 outputs, K = 128), 100 hidden units, 50 epochs.  Device
events around each launch, 3 warm-ups, median (and minimum) of the repeats; all in one process, interleaved per repeat.

Training, the benchmark's 2048 pilots:
    fnn train          esn_fnn_train, one launch
    elm fit            ElmBank.fit (features + chol) of the same pilots at --elm-hidden units
    copy               a device-to-device copy of the bytes the training reads (U + D)
  beside the time the training's FLOP count (|R| (4 K H + 6 H n_out) per epoch and pilot) takes at the float64
  matrix-pipe peak, 78.6 TFLOP/s.
Prediction, the 153 600 data frames of 12 800 blocks (every block its own trained set):
    fnn f64, fnn f16   esn_fnn_predict
    elm f64, elm f16   ElmBank.predict at the same n_hidden (one shared W_in, one read-out per block)
    elm/blk f64, f16   ElmBank.predict with one W_in per block as well (the FNN's own W1, b1 and [W2 | b2]): the same
                       bytes and the same launch shape as the FNN, tanh for ReLU

    python tools/time_fnn.py [--pilots 2048] [--blocks 12800] [--frames 12] [--repeats 9] [--ebno 21] [--hidden 100]
                             [--elm-hidden 512] [--window 8] [--epochs 50] [--out profiles/fnn_time.txt]
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
from esn_ofdm_mimo_amd.elm import ElmBank  # noqa: E402
from esn_ofdm_mimo_amd.fnn import FnnBank  # noqa: E402
from esn_ofdm_mimo_amd.montecarlo import FrameSource, LinkParams, _view_real  # noqa: E402
from esn_ofdm_mimo_amd.points import elm_weights, fnn_weights  # noqa: E402
from time_chan_metrics import timed  # noqa: E402

F64_MATRIX_PEAK = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pilots", type=int, default=2048)
    ap.add_argument("--blocks", type=int, default=12800)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--ebno", type=float, default=21.0)
    ap.add_argument("--hidden", type=int, default=100)
    ap.add_argument("--elm-hidden", type=int, default=512)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--gain", type=float, default=0.05)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fnn_time.txt"))
    a = ap.parse_args()
    prm = dataclasses.replace(LinkParams(), coherence_fixed=a.frames)
    src = FrameSource(prm, seed=1234)
    dev, G, F, P = src.device, a.blocks, a.frames, min(a.pilots, a.blocks)
    B, T, n_in, n_out, K = G * F, prm.t_frame + prm.delay, 2 * prm.n_r, 2 * prm.n_t, a.window * 2 * prm.n_r
    transient = max(prm.forget, a.window - 1)
    data = src.blocks_fast(a.ebno, 0, 0, G, F)
    U = _view_real(data["data_y"]).reshape(B, prm.t_frame, n_in)
    Up = torch.zeros((G, T, n_in), dtype=torch.float64, device=dev)
    Dp = torch.zeros((G, T, n_out), dtype=torch.float64, device=dev)
    Up[:, :prm.t_frame] = _view_real(data["pilot_y"])
    Dp[:, prm.delay:] = _view_real(data["pilot_x"])
    scale = 1.0 / np.sqrt(prm.var_x(a.ebno))

    def scaled(bank, g):
        bank.set_scaling(torch.full((g, n_in), scale, dtype=torch.float64, device=dev), None,
                         torch.full((g, n_out), scale, dtype=torch.float64, device=dev), None)
        return bank

    # ---- training of P pilots
    init = fnn_weights(a.hidden, K, n_out, 0)
    trainee = scaled(FnnBank(n_in, n_out, a.hidden, a.window, n_groups=P), P)
    W_fit, b_fit = elm_weights(a.elm_hidden, K, a.gain, 0)
    fitter = scaled(ElmBank(n_in, n_out, a.elm_hidden, a.window, W_fit, b_fit, n_groups=P), P)
    Ut, Dt = Up[:P].contiguous(), Dp[:P].contiguous()
    moved_t = (Ut.numel() + Dt.numel()) * 8
    src_t = torch.empty(moved_t // 2, dtype=torch.uint8, device=dev)
    dst_t = torch.empty_like(src_t)
    ms_t = timed({"fnn train": lambda: trainee.train(Ut, Dt, init, transient=transient, epochs=a.epochs),
                  f"elm fit, {a.elm_hidden} units": lambda: fitter.fit(Ut, Dt, transient=transient, method="chol",
                                                                      repair=False),
                  "copy, bytes of U + D": lambda: dst_t.copy_(src_t)}, warmup=3, repeats=a.repeats)
    n_rows = T - transient
    flop_t = float(P) * a.epochs * n_rows * (4.0 * K * a.hidden + 6.0 * a.hidden * n_out)

    # ---- prediction of B frames, every block its own set
    fnn = scaled(FnnBank(n_in, n_out, a.hidden, a.window, n_groups=G), G)
    fnn.train(Up, Dp, init, transient=transient, epochs=a.epochs)
    W_in, b = elm_weights(a.hidden, K, a.gain, 0)
    elm = scaled(ElmBank(n_in, n_out, a.hidden, a.window, W_in, b, n_groups=G), G)
    elm.fit(Up, Dp, transient=transient, method="auto")
    per_block = scaled(ElmBank(n_in, n_out, a.hidden, a.window, fnn.W1, fnn.b1, n_groups=G), G)
    per_block.set_readout(torch.cat([fnn.W2, fnn.b2[:, :, None]], dim=2))
    banks = {"fnn": fnn, "elm": elm, "elm/blk": per_block}
    names = [f"{m} {p}" for p in ("f64", "f16") for m in banks]
    Y = {k: torch.empty((B, prm.n_sub, n_out), dtype=torch.float64, device=dev) for k in names}
    fns = {}
    for k in names:
        bank, p = banks[k.split()[0]], k.split()[1]
        fns[k] = (lambda bank=bank, p=p, k=k: bank.predict(U, F, T=T, transient=prm.forget, precision=p, out=Y[k]))
    ms_p = timed(fns, warmup=3, repeats=a.repeats)
    rel = float((Y["fnn f16"] - Y["fnn f64"]).abs().max() / Y["fnn f64"].abs().max())

    med_t = {k: v[len(v) // 2] for k, v in ms_t.items()}
    med_p = {k: v[len(v) // 2] for k, v in ms_p.items()}
    lines = [f"device {_lib.device_info()['arch']}  {prm.n_t}x{prm.n_r}  N {prm.n_sub}  T {T}  K {K}  hidden {a.hidden}  "
             f"window {a.window}  epochs {a.epochs}  Eb/No {a.ebno} dB  repeats {a.repeats} (median [min])",
             f"training of {P} pilots: {flop_t / 1e9:.1f} GFLOP, {flop_t / F64_MATRIX_PEAK * 1e3:.3f} ms at the float64 "
             f"matrix-pipe peak ({F64_MATRIX_PEAK / 1e12:.1f} TFLOP/s); {moved_t / 2 ** 20:.1f} MiB of U + D"]
    for k, v in ms_t.items():
        rate = f"  {flop_t / med_t[k] / 1e9:8.2f} TFLOP/s" if k == "fnn train" else ""
        lines.append(f"  {k:24s} {med_t[k]:9.3f} ms [{v[0]:9.3f}]{rate}")
    lines.append(f"fnn train / time at the matrix-pipe peak: {med_t['fnn train'] / (flop_t / F64_MATRIX_PEAK * 1e3):.1f};  "
                 f"fnn train / elm fit: {med_t['fnn train'] / med_t[f'elm fit, {a.elm_hidden} units']:.2f};  "
                 f"fnn train / copy: {med_t['fnn train'] / med_t['copy, bytes of U + D']:.0f}")
    lines.append(f"prediction of {G} blocks x {F} frames = {B} frames, {a.hidden} units; max |Y f16 - Y f64| / max |Y f64| "
                 f"of the FNN = {rel:.2e}")
    for k, v in ms_p.items():
        lines.append(f"  {k:24s} {med_p[k]:9.3f} ms [{v[0]:9.3f}]")
    lines.append(f"fnn / elm (medians): f64 {med_p['fnn f64'] / med_p['elm f64']:.3f};  f16 "
                 f"{med_p['fnn f16'] / med_p['elm f16']:.3f};  fnn / elm with one W_in per block: f64 "
                 f"{med_p['fnn f64'] / med_p['elm/blk f64']:.3f};  f16 {med_p['fnn f16'] / med_p['elm/blk f16']:.3f}")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
