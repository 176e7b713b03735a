#!/usr/bin/env python3
"""Time of the hold-out scoring launch (esn_readout_holdout_score_f32, csrc/esn_holdout.hip) on the benchmark's chunk of
2048 groups at the headline shape (cols 528, 128 held-out rows, 8 outputs), beside the multi-lambda Cholesky solve that
feeds it (esn_readout_solve_chol_ridge_batch_f32 over the (P - 1) x 128 stacked rows of the other pilots) and beside a
device-to-device copy that reads and writes, together, the bytes the scoring launch reads (W, E, D).  Device events
around each launch, 3 warm-ups, median (and minimum) of the repeats; all in one process, interleaved per repeat.
Random inputs: neither kernel's time depends on the values.

    python tools/time_holdout.py [--groups 2048] [--pilots 4] [--candidates 16] [--repeats 9] [--out profiles/holdout_time.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from esn_ofdm_mimo_amd import _lib  # noqa: E402
from esn_ofdm_mimo_amd._lib import check, ptr  # noqa: E402
from time_chan_metrics import timed  # noqa: E402


COPY = "copy of the bytes the score reads"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=2048)
    ap.add_argument("--pilots", type=int, default=4)
    ap.add_argument("--candidates", type=int, default=16)
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--cols", type=int, default=528)
    ap.add_argument("--n-out", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib, dev = _lib.load(), torch.device("cuda")
    G, L, rows, cols, n_out = a.groups, a.candidates, a.rows, a.cols, a.n_out
    fit_rows = (a.pilots - 1) * rows
    gen = torch.Generator(device=dev).manual_seed(1)
    E_fit = torch.randn((G, fit_rows, cols), generator=gen, device=dev, dtype=torch.float32)
    D_fit = torch.randn((G, fit_rows, n_out), generator=gen, device=dev, dtype=torch.float64)
    E_val = torch.randn((G, rows, cols), generator=gen, device=dev, dtype=torch.float32)
    D_val = torch.randn((G, rows, n_out), generator=gen, device=dev, dtype=torch.float64)
    lam = torch.logspace(-4, 1, L, dtype=torch.float64, device=dev).expand(G, L).contiguous() * float(cols)
    W = torch.empty((G, L, n_out, cols), dtype=torch.float64, device=dev)
    status = torch.empty((G, L), dtype=torch.int32, device=dev)
    score = torch.empty((G, L), dtype=torch.float64, device=dev)
    choice = torch.empty((G,), dtype=torch.int32, device=dev)
    wbytes = lib.esn_readout_chol_ridge_workspace_bytes(G, L, fit_rows, cols)
    ws = torch.empty(max(wbytes, 16), dtype=torch.uint8, device=dev)
    st = _lib.stream_handle()
    read = W.numel() * 8 + E_val.numel() * 4 + D_val.numel() * 8
    src = torch.empty(read // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)

    def solve():
        check(lib.esn_readout_solve_chol_ridge_batch_f32(ptr(E_fit), ptr(D_fit), G, fit_rows, 0, cols, n_out, None, None,
                                                         ptr(lam), L, ptr(W), ptr(status), ptr(ws), wbytes, st),
              "esn_readout_solve_chol_ridge_batch_f32")

    def holdout():
        check(lib.esn_readout_holdout_score_f32(ptr(E_val), ptr(D_val), ptr(W), G, rows, 0, cols, n_out, None, None, L,
                                                ptr(status), ptr(score), ptr(choice), st), "esn_readout_holdout_score_f32")

    ms = timed({"multi-lambda Cholesky solve": solve, "hold-out score": holdout, COPY: lambda: dst.copy_(src)},
               warmup=3, repeats=a.repeats)
    med = {k: v[len(v) // 2] for k, v in ms.items()}
    flops = 2.0 * G * rows * cols * L * n_out
    lines = [f"device {_lib.device_info()['arch']}  {G} groups  {a.pilots} pilots x {rows} rows  cols {cols}  n_out {n_out}  "
             f"{L} candidates  float32 E  repeats {a.repeats} (median [min])",
             f"the score reads {read / 2**30:.2f} GiB (W {W.numel() * 8 / 2**30:.2f}, E {E_val.numel() * 4 / 2**30:.2f}) and does "
             f"{flops / 1e9:.1f} GFLOP; the solve's workspace is {wbytes / 2**30:.2f} GiB; flagged solves {int((status != 0).sum())}, "
             f"groups without a choice {int((choice < 0).sum())}"]
    for k, v in ms.items():
        extra = f"  {read / med[k] / 1e6:8.1f} GB/s" if not k.startswith("multi") else ""
        extra += f"  {flops / med[k] / 1e9:6.2f} TFLOP/s" if k.startswith("hold") else ""
        lines.append(f"  {k:30s} {med[k]:9.3f} ms [{v[0]:9.3f}]{extra}")
    lines.append(f"score / solve {med['hold-out score'] / med['multi-lambda Cholesky solve']:.3f}, "
                 f"score / copy {med['hold-out score'] / med[COPY]:.2f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
