#!/usr/bin/env python3
"""Time of the two launches of the running normal equations (csrc/esn_gram.hip) on the benchmark's chunk of 2048 groups
at the headline shape (128 rows, cols 528, 8 outputs, float32 E):

    esn_gram_accumulate_f32 with decay 1 (it reads and writes the whole state) and with decay 0 (it only writes it), beside
        a device-to-device copy that reads and writes the state's bytes (Gm and Cm once each way)
    esn_gram_solve at 1 and at 16 candidates per group, beside esn_readout_solve_chol_ridge_batch_f32 on 384 stacked rows
        with the same candidates -- the launch it replaces in the hold-out fit of four pilots (profiles/holdout_time.txt)

Device events around each launch, 2 warm-ups, median (and minimum) of the repeats; all variants in one process,
interleaved per repeat.  Random inputs: no kernel's time depends on the values (lambda is large enough that no pivot
is rejected).

    python tools/time_gram.py [--groups 2048] [--repeats 9] [--out profiles/gram_time.txt]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=2048)
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--stacked-rows", type=int, default=384)
    ap.add_argument("--cols", type=int, default=528)
    ap.add_argument("--n-out", type=int, default=8)
    ap.add_argument("--candidates", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib, dev = _lib.load(), torch.device("cuda")
    G, L, rows, srows, cols, n_out = a.groups, a.candidates, a.rows, a.stacked_rows, a.cols, a.n_out
    gen = torch.Generator(device=dev).manual_seed(1)
    E = torch.randn((G, rows, cols), generator=gen, device=dev, dtype=torch.float32)
    D = torch.randn((G, rows, n_out), generator=gen, device=dev, dtype=torch.float64)
    E_st = torch.randn((G, srows, cols), generator=gen, device=dev, dtype=torch.float32)
    D_st = torch.randn((G, srows, n_out), generator=gen, device=dev, dtype=torch.float64)
    Gm = torch.empty((G, cols, cols), dtype=torch.float64, device=dev)
    Cm = torch.empty((G, n_out, cols), dtype=torch.float64, device=dev)
    lam = torch.logspace(-4, 1, L, dtype=torch.float64, device=dev).expand(G, L).contiguous() * float(cols)
    lam1 = lam[:, L // 2:L // 2 + 1].contiguous()
    W = torch.empty((G, L, n_out, cols), dtype=torch.float64, device=dev)
    status = torch.empty((G, L), dtype=torch.int32, device=dev)
    gbytes = lib.esn_gram_solve_workspace_bytes(G, L, cols)
    cbytes = lib.esn_readout_chol_ridge_workspace_bytes(G, L, srows, cols)
    ws = torch.empty(max(gbytes, cbytes, 16), dtype=torch.uint8, device=dev)
    st = _lib.stream_handle()
    state_bytes = (Gm.numel() + Cm.numel()) * 8
    src = torch.empty(state_bytes, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)

    def accumulate(decay):
        check(lib.esn_gram_accumulate_f32(ptr(E), ptr(D), G, rows, 0, cols, n_out, None, None, decay, ptr(Gm), ptr(Cm), st),
              "esn_gram_accumulate_f32")

    def gram_solve(l, n_l):
        check(lib.esn_gram_solve(ptr(Gm), ptr(Cm), G, cols, n_out, ptr(l), n_l, ptr(W), ptr(status), ptr(ws), gbytes, st),
              "esn_gram_solve")

    def chol(l, n_l):
        check(lib.esn_readout_solve_chol_ridge_batch_f32(ptr(E_st), ptr(D_st), G, srows, 0, cols, n_out, None, None, ptr(l),
                                                         n_l, ptr(W), ptr(status), ptr(ws), cbytes, st),
              "esn_readout_solve_chol_ridge_batch_f32")

    accumulate(0.0)                     # a state for the solves: three segments, as the hold-out fit of four pilots
    accumulate(1.0)
    accumulate(1.0)
    gram_solve(lam, L)
    flagged = int((status != 0).sum())
    names = {"acc1": "accumulate, decay 1 (state read and written)", "acc0": "accumulate, decay 0 (state written)",
             "copy": "copy of the state's bytes (read + write)", "g1": "gram solve, 1 candidate",
             "c1": f"Cholesky ridge solve {srows} x {cols}, 1 candidate", "gL": f"gram solve, {L} candidates",
             "cL": f"Cholesky ridge solve {srows} x {cols}, {L} candidates"}
    ms = timed({"acc1": lambda: accumulate(1.0), "acc0": lambda: accumulate(0.0), "copy": lambda: dst.copy_(src),
                "g1": lambda: gram_solve(lam1, 1), "c1": lambda: chol(lam1, 1), "gL": lambda: gram_solve(lam, L),
                "cL": lambda: chol(lam, L)}, warmup=2, repeats=a.repeats)
    med = {k: v[len(v) // 2] for k, v in ms.items()}
    np_ = (cols + 15) // 16 * 16
    lines = [f"device {_lib.device_info()['arch']}  {G} groups  {rows} rows  cols {cols}  n_out {n_out}  float32 E  repeats "
             f"{a.repeats} (median [min])  commit {a.commit}",
             f"the state holds {state_bytes / 2**30:.2f} GiB ({state_bytes / G / 1e6:.2f} MB per group); E {E.numel() * 4 / 2**30:.2f} "
             f"GiB; gram solve workspace {gbytes / 2**30:.2f} GiB for any number of candidates, the Cholesky ridge solve's "
             f"{cbytes / 2**30:.2f} GiB at {L}; flagged gram solves {flagged}",
             f"FLOP per group: Gram update {2.0 * rows * cols * (cols + n_out) / 2 / 1e6:.1f} M (lower half), factorisation "
             f"{np_ ** 3 / 3 / 1e6:.1f} M per candidate"]
    for k, v in ms.items():
        extra = ""
        if k in ("acc1", "copy"):
            extra = f"  {2 * state_bytes / med[k] / 1e6:8.1f} GB/s"
        if k == "acc0":
            extra = f"  {state_bytes / med[k] / 1e6:8.1f} GB/s"
        lines.append(f"  {names[k]:52s} {med[k]:9.3f} ms [{v[0]:9.3f}]{extra}")
    lines.append(f"accumulate (decay 1) / copy {med['acc1'] / med['copy']:.2f}; gram / Cholesky solve at 1 candidate "
                 f"{med['g1'] / med['c1']:.2f}, at {L} candidates {med['gL'] / med['cL']:.2f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
